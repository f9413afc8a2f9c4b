// mod_ht40_chain.cpp -- the joint-coded data graph of the 40 MHz HT 2x2 modulator (include/sora_hip.h: the chains of the sora_hip_*_ht40 stages) for one MCS, built from
// the adapters of include/sora_brick.hpp, sink first:
//   source pin -> THip11aSc -> THipConvEncode<CR> -> THipHt40StreamParser<N_BPSC> -+-> THipHt40Interleave<N_BPSC, 0> -> THipHt40Map -> THipHt40AddPilot -> THipHt40IFFT
//                                                                                  |       -> THipHt40AddGI<GI> -> sink 0
//                                                                                  +-> THipHt40Interleave<N_BPSC, 1> -> THipHt40Map -> THipHt40AddPilot -> THipHt40IFFT
//                                                                                          -> THipHt40AddGI<GI> -> sink 1
// One symbol per burst, so the scrambler's and the encoder's registers cross burst boundaries.  The host plays the source: SERVICE + MPDU + FCS + tail + pad, and turns
// the transmitter's seed (seven bits, bit i = x[-1 - i]) into the scrambler brick's register, the bits reversed and << 1.  MCS whose symbol is a whole number of the
// byte-wide bricks' bursts: 9, 11, 12, 13 (N_DBPS 216, 432, 648, 864 bits = 27, 54, 81, 108 bytes; at MCS 8, 10 and 14 a symbol is 13.5, 40.5 and 121.5 bytes).
// usage: mod_ht40_chain <mcs> <seed> <gi> <mpdu.bin> <out.bin>     out.bin: COMPLEX16, the data symbols of TX chain 0, then those of chain 1 (samples 1600 .. of
// sora_hip_tx_ht40_joint_gi's)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "sora_brick.hpp"

using namespace sora_brick;

// a sink: appends every burst to a host vector
template <size_t BURST>
class TCollect {
public:
    TCollect(CF_Error&, std::vector<sora_complex16>& host) : host_(host) {}
    void Reset() {}
    void Flush() {}
    template <class T_IPIN> bool Process(T_IPIN& ipin)
    {
        while (ipin.check_read()) {
            const size_t at = host_.size();
            host_.resize(at + BURST);
            if (sora_hip_stream_synchronize(nullptr) != SORA_OK || sora_hip_memcpy_d2h(host_.data() + at, ipin.peek(), BURST * sizeof(sora_complex16)) != SORA_OK) return false;
            ipin.pop();
        }
        return true;
    }
private:
    std::vector<sora_complex16>& host_;
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

template <int NB, int CR, int ND, int GI>
static int run(const std::vector<uint8_t>& mpdu, uint8_t seed, const char* outp)
{
    static_assert(ND % 8 == 0 && (ND / 8) % (CR + 1) == 0, "a symbol of whole encoder bursts");
    constexpr size_t SYM_IN = ND / 8, ROW = kRowHt40(NB), SYM_OUT = GI ? 144 : 160;
    static_assert(SYM_IN / (CR + 1) * (CR + 2) == 27 * NB, "the encoder's symbol is the parser's burst");
    CF_Error ctx;
    std::vector<sora_complex16> host[2];

    const size_t ln = mpdu.size() + 4, nsym = (ln * 8 + 16 + 6 + ND - 1) / ND, nbytes = nsym * SYM_IN;
    std::vector<uint8_t> data(nbytes, 0);
    memcpy(data.data() + 2, mpdu.data(), mpdu.size());
    const uint32_t fcs = crc32_of(mpdu.data(), mpdu.size());
    for (int k = 0; k < 4; k++) data[2 + mpdu.size() + k] = (uint8_t)(fcs >> (8 * k));
    uint8_t reg = 0;                                                                       // seed bit i = x[-1 - i] sits at bit 7 - i of the brick's register
    for (int i = 0; i < 7; i++) reg |= (uint8_t)(((seed >> i) & 1u) << (7 - i));

    sora_complex16* d_out[2]; sora_complex16* d_t[2]; sora_complex16* d_bins[2]; sora_complex16* d_car[2]; uint8_t* d_il[2]; uint8_t* d_sp[2];
    for (int s = 0; s < 2; s++) {
        d_out[s] = dmalloc<sora_complex16>(SYM_OUT); d_t[s] = dmalloc<sora_complex16>(128); d_bins[s] = dmalloc<sora_complex16>(128); d_car[s] = dmalloc<sora_complex16>(108);
        d_il[s] = dmalloc<uint8_t>(ROW + 16); d_sp[s] = dmalloc<uint8_t>(ROW + 16);
    }
    uint8_t* d_sc = dmalloc<uint8_t>(SYM_IN + 16);
    uint8_t* d_tabs = dmalloc<uint8_t>(64);
    uint8_t* d_in = dmalloc<uint8_t>(SYM_IN + 16);

    // spatial stream 0 -> TX chain 0
    TCollect<SYM_OUT> sink0(ctx, host[0]);
    THipHt40AddGI<GI, 1, CF_Error, decltype(sink0)> gi0(ctx, &sink0, d_out[0]);
    THipHt40IFFT<1, CF_Error, decltype(gi0)> ifft0(ctx, &gi0, d_t[0]);
    THipHt40AddPilot<1, CF_Error, decltype(ifft0)> pilot0(ctx, &ifft0, d_bins[0], d_tabs);
    THipHt40Map<NB, 1, CF_Error, decltype(pilot0)> map0(ctx, &pilot0, d_car[0]);
    THipHt40Interleave<NB, 0, 1, CF_Error, decltype(map0)> inter0(ctx, &map0, d_il[0]);
    // spatial stream 1 -> TX chain 1 (no cyclic shift)
    TCollect<SYM_OUT> sink1(ctx, host[1]);
    THipHt40AddGI<GI, 1, CF_Error, decltype(sink1)> gi1(ctx, &sink1, d_out[1]);
    THipHt40IFFT<1, CF_Error, decltype(gi1)> ifft1(ctx, &gi1, d_t[1]);
    THipHt40AddPilot<1, CF_Error, decltype(ifft1)> pilot1(ctx, &ifft1, d_bins[1], d_tabs + 16);
    THipHt40Map<NB, 1, CF_Error, decltype(pilot1)> map1(ctx, &pilot1, d_car[1]);
    THipHt40Interleave<NB, 1, 1, CF_Error, decltype(map1)> inter1(ctx, &map1, d_il[1]);
    // the shared front
    THipHt40StreamParser<NB, 1, CF_Error, decltype(inter0), decltype(inter1)> parser(ctx, &inter0, &inter1, d_sp[0], d_sp[1]);
    using Enc = THipConvEncode<CR, SYM_IN, CF_Error, decltype(parser)>;
    uint8_t* d_encw = dmalloc<uint8_t>(Enc::kWorkBytes);
    Enc enc(ctx, &parser, d_encw);
    THip11aSc<SYM_IN, CF_Error, Enc> sc(ctx, &enc, d_sc, d_tabs + 32, reg);

    sc.Reset();
    sc.SetTail((uint32_t)(2 + ln));
    DevicePin<uint8_t, SYM_IN> src(d_in);
    for (size_t s = 0; s < nsym; s++) {
        CHECK(sora_hip_stream_synchronize(nullptr) == SORA_OK);                            // (the pin's buffer is rewritten: one burst in flight)
        CHECK(sora_hip_memcpy_h2d(src.append(), data.data() + s * SYM_IN, SYM_IN) == SORA_OK);
        CHECK(sc.Process(src));
    }
    sc.Flush();

    FILE* fo = fopen(outp, "wb");
    if (!fo) return 1;
    for (int s = 0; s < 2; s++)
        if (fwrite(host[s].data(), sizeof(sora_complex16), host[s].size(), fo) != host[s].size()) return 1;
    fclose(fo);
    printf("mod_ht40 chain: %zu data symbols, %zu samples per chain\n", nsym, host[0].size());
    return 0;
}

template <int NB, int CR, int ND>
static int run_gi(int gi, const std::vector<uint8_t>& mpdu, uint8_t seed, const char* outp)
{
    return gi ? run<NB, CR, ND, 1>(mpdu, seed, outp) : run<NB, CR, ND, 0>(mpdu, seed, outp);
}

int main(int argc, char** argv)
{
    if (argc != 6) { fprintf(stderr, "usage: %s <mcs> <seed> <gi> <mpdu.bin> <out.bin>\n", argv[0]); return 2; }
    FILE* f = fopen(argv[4], "rb");
    if (!f) return 1;
    fseek(f, 0, SEEK_END); const long bytes = ftell(f); fseek(f, 0, SEEK_SET);
    std::vector<uint8_t> mpdu((size_t)bytes);
    if (fread(mpdu.data(), 1, mpdu.size(), f) != mpdu.size()) return 1;
    fclose(f);
    const uint8_t seed = (uint8_t)strtoul(argv[2], nullptr, 0);
    const int gi = atoi(argv[3]);
    if (gi != 0 && gi != 1) { fprintf(stderr, "gi %s: not 0 or 1\n", argv[3]); return 2; }
    switch (atoi(argv[1])) {
    case 9:  return run_gi<2, SORA_CR_12, 216>(gi, mpdu, seed, argv[5]);
    case 11: return run_gi<4, SORA_CR_12, 432>(gi, mpdu, seed, argv[5]);
    case 12: return run_gi<4, SORA_CR_34, 648>(gi, mpdu, seed, argv[5]);
    case 13: return run_gi<6, SORA_CR_23, 864>(gi, mpdu, seed, argv[5]);
    }
    fprintf(stderr, "MCS %s: not one of 9, 11, 12, 13\n", argv[1]);
    return 2;
}
