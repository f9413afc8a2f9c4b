// mod_chain.cpp -- the 802.11a modulation graph built from the adapters of include/sora_brick.hpp and EXECUTED on the GPU (tests/test_gpu_mod_hosts.py), sink first and in
// the order of kernel/bb/demod11/fb11amod_config.hpp:74-109:
//   data:     source pin -> THip11aSc -> THipConvEncode<CR> -> THip11aInterleave<N_BPSC> -> THipMap11a<N_BPSC> -+
//   SIGNAL:   source pin ----------------> THipConvEncode<1/2> -> THip11aInterleave<1> ----> THipMap11a<1> -----+-> THip11aAddPilot -> THipIFFTx -> [THipUpsample40MTo44M]
//   preamble: sora_hip_preamble11a -> [THipUpsample40MTo44M, one burst of four blocks] -> THipPackSample16to8 -> sink                   -> THipPackSample16to8 -> sink
// The two branches share the bricks from T11aAddPilot on, as the reference's TBB11aMRSelect branches do; one symbol per burst, so the scrambler's register, the
// encoder's register and the pilot index all cross burst boundaries.  The host plays TBB11aSrc (PHY_11a.hpp:111-202): SIGNAL bytes, SERVICE + MPDU + FCS + tail + pad.
// Rates whose symbol is a whole number of bytes: every rate but 9 Mbps (36 bits per symbol; the byte-wide bricks' bursts do not end on its symbols).
// usage: mod_chain <rate_kbps> <seed> <mpdu.bin> <out.bin> [44]        out.bin: COMPLEX8, what sora_hip_tx11a / sora_hip_tx11a44 write for the frame
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <vector>
#include "sora_brick.hpp"

using namespace sora_brick;

// TModSink stand-in: appends every burst to a host vector
template <size_t BURST>
class TCollect {
public:
    TCollect(CF_Error&, std::vector<sora_complex8>& host) : host_(host) {}
    void Reset() {}
    void Flush() {}
    template <class T_IPIN> bool Process(T_IPIN& ipin)
    {
        while (ipin.check_read()) {
            const size_t at = host_.size();
            host_.resize(at + BURST);
            if (sora_hip_stream_synchronize(nullptr) != SORA_OK || sora_hip_memcpy_d2h(host_.data() + at, ipin.peek(), BURST * sizeof(sora_complex8)) != SORA_OK) return false;
            ipin.pop();
        }
        return true;
    }
private:
    std::vector<sora_complex8>& host_;
};

static uint32_t crc32_of(const uint8_t* p, size_t n)
{
    uint32_t c = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; i++) { c ^= p[i]; for (int k = 0; k < 8; k++) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1u))); }
    return ~c;
}

template <class T> static T* dmalloc(size_t count)
{
    T* p = (T*)sora_hip_malloc(count * sizeof(T));
    if (!p) { fprintf(stderr, "device memory: %s\n", sora_hip_last_error()); exit(1); }
    return p;
}

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "%s failed: error_code %08x (%s)\n", #x, ctx.error_code, sora_hip_last_error()); return 1; } } while (0)

template <int NB, int CR, int ND, int RATE_CODE, bool UP44>
static int run(const std::vector<uint8_t>& mpdu, uint8_t seed, const char* outp)
{
    static_assert(ND % 8 == 0, "a symbol of whole bytes");
    constexpr size_t SYM_IN = ND / 8, SYM_CODED = 6 * NB, SYM_OUT = UP44 ? 176 : 160;
    CF_Error ctx;
    std::vector<sora_complex8> host;

    // TBB11aSrc::Process
    uint32_t sig = (uint32_t)RATE_CODE | (uint32_t)((mpdu.size() + 4) << 5);
    sig |= (uint32_t)(__builtin_popcount(sig) & 1) << 17;
    const uint8_t sigb[3] = { (uint8_t)sig, (uint8_t)(sig >> 8), (uint8_t)(sig >> 16) };
    const size_t dbytes = 2 + mpdu.size() + 4 + 1, rem = dbytes * 8 % ND;
    const size_t nbytes = dbytes + ((rem ? ND - rem : 0) + 7) / 8, nsym = nbytes * 8 / ND;
    std::vector<uint8_t> data(nbytes, 0);
    memcpy(data.data() + 2, mpdu.data(), mpdu.size());
    const uint32_t fcs = crc32_of(mpdu.data(), mpdu.size());
    for (int k = 0; k < 4; k++) data[2 + mpdu.size() + k] = (uint8_t)(fcs >> (8 * k));

    // ---- CreatePreamble11a_40M / _44M
    {
        sora_complex16* d_pre = dmalloc<sora_complex16>(640);
        sora_complex16* d_up = dmalloc<sora_complex16>(704);
        sora_complex8* d_p8 = dmalloc<sora_complex8>(704);
        uint8_t* d_sees = dmalloc<uint8_t>(16);
        const uint8_t sees[4] = { 1, 1, 1, 0 };
        CHECK(sora_hip_memcpy_h2d(d_sees, sees, 4) == SORA_OK);
        TCollect<4 * SYM_OUT> sink(ctx, host);
        THipPackSample16to8<4 * SYM_OUT, CF_Error, decltype(sink)> pack(ctx, &sink, d_p8);
        DevicePin<sora_complex16, 640> src(d_pre);
        CHECK(sora_hip_preamble11a(src.append(), 1, nullptr) == SORA_OK);                  // TTS11aSrc: the whole preamble as one burst
        if constexpr (UP44) {
            THipUpsample40MTo44M<4, CF_Error, decltype(pack)> up(ctx, &pack, d_up, d_sees);
            up.Reset(); CHECK(up.Process(src)); up.Flush();
        } else {
            pack.Reset(); CHECK(pack.Process(src)); pack.Flush();
        }
        sora_hip_free(d_pre); sora_hip_free(d_up); sora_hip_free(d_p8); sora_hip_free(d_sees);
    }

    // ---- CreateModGraph11a_40M / _44M, sink first
    sora_complex8* d_o8 = dmalloc<sora_complex8>(SYM_OUT);
    sora_complex16* d_up = dmalloc<sora_complex16>(176);
    sora_complex16* d_t = dmalloc<sora_complex16>(160);
    sora_complex16* d_bins = dmalloc<sora_complex16>(64);
    sora_complex16* d_car = dmalloc<sora_complex16>(48);
    sora_complex16* d_scar = dmalloc<sora_complex16>(48);
    uint8_t* d_il = dmalloc<uint8_t>(SYM_CODED + 16); uint8_t* d_sil = dmalloc<uint8_t>(16);
    uint8_t* d_sc = dmalloc<uint8_t>(SYM_IN + 16);
    uint8_t* d_tabs = dmalloc<uint8_t>(64);
    uint8_t* d_in = dmalloc<uint8_t>(SYM_IN + 16); uint8_t* d_sin = dmalloc<uint8_t>(16);

    TCollect<SYM_OUT> sink(ctx, host);
    THipPackSample16to8<SYM_OUT, CF_Error, decltype(sink)> pack(ctx, &sink, d_o8);
    THipUpsample40MTo44M<1, CF_Error, decltype(pack)> up(ctx, &pack, d_up);
    using TailNext = std::conditional_t<UP44, decltype(up), decltype(pack)>;
    TailNext* tail_next;
    if constexpr (UP44) tail_next = &up; else tail_next = &pack;
    THipIFFTx<1, CF_Error, TailNext> ifftx(ctx, tail_next, d_t);
    THip11aAddPilot<1, CF_Error, decltype(ifftx)> pilot(ctx, &ifftx, d_bins, d_tabs);
    // the data branch
    THipMap11a<NB, 1, CF_Error, decltype(pilot)> map(ctx, &pilot, d_car);
    THip11aInterleave<NB, 1, CF_Error, decltype(map)> inter(ctx, &map, d_il);
    using Enc = THipConvEncode<CR, SYM_IN, CF_Error, decltype(inter)>;
    uint8_t* d_encw = dmalloc<uint8_t>(Enc::kWorkBytes);
    Enc enc(ctx, &inter, d_encw);
    THip11aSc<SYM_IN, CF_Error, Enc> sc(ctx, &enc, d_sc, d_tabs + 16, seed);
    // the SIGNAL branch: no scrambler (NO_SCRAMBLE), the 6 Mbps path
    THipMap11a<1, 1, CF_Error, decltype(pilot)> smap(ctx, &pilot, d_scar);
    THip11aInterleave<1, 1, CF_Error, decltype(smap)> sinter(ctx, &smap, d_sil);
    using SEnc = THipConvEncode<SORA_CR_12, 3, CF_Error, decltype(sinter)>;
    uint8_t* d_sencw = dmalloc<uint8_t>(SEnc::kWorkBytes);
    SEnc senc(ctx, &sinter, d_sencw);

    sc.Reset(); senc.Reset();                                                             // (both reach the shared bricks: Reset twice is Reset)
    sc.SetTail((uint32_t)(dbytes - 1));
    DevicePin<uint8_t, 3> ssrc(d_sin);
    CHECK(sora_hip_memcpy_h2d(ssrc.append(), sigb, 3) == SORA_OK);
    CHECK(senc.Process(ssrc));
    DevicePin<uint8_t, SYM_IN> src(d_in);
    for (size_t s = 0; s < nsym; s++) {
        CHECK(sora_hip_stream_synchronize(nullptr) == SORA_OK);                            // (the pin's buffer is rewritten: one burst in flight)
        CHECK(sora_hip_memcpy_h2d(src.append(), data.data() + s * SYM_IN, SYM_IN) == SORA_OK);
        CHECK(sc.Process(src));
    }
    sc.Flush();

    FILE* fo = fopen(outp, "wb");
    if (!fo || fwrite(host.data(), sizeof(sora_complex8), host.size(), fo) != host.size()) return 1;
    fclose(fo);
    printf("mod chain: %zu data symbols, %zu samples out\n", nsym, host.size());
    return 0;
}

template <bool UP44>
static int dispatch(int rate, const std::vector<uint8_t>& mpdu, uint8_t seed, const char* outp)
{
    switch (rate) {
    case 6000:  return run<1, SORA_CR_12, 24, 0xB, UP44>(mpdu, seed, outp);
    case 12000: return run<2, SORA_CR_12, 48, 0xA, UP44>(mpdu, seed, outp);
    case 18000: return run<2, SORA_CR_34, 72, 0xE, UP44>(mpdu, seed, outp);
    case 24000: return run<4, SORA_CR_12, 96, 0x9, UP44>(mpdu, seed, outp);
    case 36000: return run<4, SORA_CR_34, 144, 0xD, UP44>(mpdu, seed, outp);
    case 48000: return run<6, SORA_CR_23, 192, 0x8, UP44>(mpdu, seed, outp);
    case 54000: return run<6, SORA_CR_34, 216, 0xC, UP44>(mpdu, seed, outp);
    }
    fprintf(stderr, "rate %d: not one of 6, 12, 18, 24, 36, 48, 54 Mbps\n", rate);
    return 2;
}

int main(int argc, char** argv)
{
    if (argc != 5 && argc != 6) { fprintf(stderr, "usage: %s <rate_kbps> <seed> <mpdu.bin> <out.bin> [44]\n", argv[0]); return 2; }
    FILE* f = fopen(argv[3], "rb");
    if (!f) return 1;
    fseek(f, 0, SEEK_END); const long bytes = ftell(f); fseek(f, 0, SEEK_SET);
    std::vector<uint8_t> mpdu((size_t)bytes);
    if (fread(mpdu.data(), 1, mpdu.size(), f) != mpdu.size()) return 1;
    fclose(f);
    const int rate = atoi(argv[1]); const uint8_t seed = (uint8_t)strtoul(argv[2], nullptr, 0);
    return argc == 6 && atoi(argv[5]) == 44 ? dispatch<true>(rate, mpdu, seed, argv[4]) : dispatch<false>(rate, mpdu, seed, argv[4]);
}
