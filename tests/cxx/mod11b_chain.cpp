// mod11b_chain.cpp -- the 802.11b modulation graph built from the adapters of include/sora_brick.hpp and EXECUTED on the GPU (tests/test_gpu_mod11b_hosts.py), sink
// first and in the order of kernel/bb/demod11/fb11bmod_config.hpp:28-50:
//   source pin -> THip11bSc741<1> -> rate select -+-> THip11bDBPSKSpread<1> -> re-burst 88 -+
//                                                 +-> THip11bDQPSKSpread<1> -> re-burst 44 -+-> THip11bQuickPulseShaper<2> -> THipPackSample16to8<8> -> sink
//                                                 +-> THip11bCCK5Encode<1> --> re-burst 16 -+
//                                                 +-> THip11bCCK11Encode<1> -> re-burst 8 --+
// One byte per burst in front of the shaper and two chips per burst behind it, so the scrambler's register, last_phase, bEven and the shaper's partial sums all cross
// burst boundaries, in the device records the adapters share.  The host plays TBB11bSrc (PHY_11b.hpp:19-206) and TBB11bMRSelect (:208-330): header bytes to the DBPSK
// spreader (behind the short preamble the six PLCP bytes to the DQPSK one), MPDU + FCS to the spreader of the frame's rate.  The re-burst stands for the reference's pin
// queue between a spreader and the shaper: the same device buffer, handed on two chips at a time.
// usage: mod11b_chain <rate_kbps> <preamble kind: 0 long, 1 short> <mpdu.bin> <out.bin>      out.bin: COMPLEX8, what sora_hip_tx11b_pre writes for the frame
#include <cstdio>
#include <cstdlib>
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

// the pin queue between a brick that emits IN items a burst and one that takes OUT: the burst is handed on in place, OUT at a time
template <class T, size_t IN, size_t OUT, class T_NEXT>
class TReburst {
public:
    static_assert(IN % OUT == 0, "whole bursts");
    explicit TReburst(T_NEXT* next) : next_(next) {}
    void Reset() { next_->Reset(); }
    void Flush() { next_->Flush(); }
    template <class T_IPIN> bool Process(T_IPIN& ipin)
    {
        while (ipin.check_read()) {
            for (size_t k = 0; k < IN; k += OUT) {
                DevicePin<T, OUT> sub(const_cast<T*>(ipin.peek()) + k);
                sub.append();
                if (!next_->Process(sub)) return false;
            }
            ipin.pop();
        }
        return true;
    }
private:
    T_NEXT* next_;
};

// TBB11bMRSelect, the host's: byte k of the PPDU goes to the DBPSK spreader while the header lasts (behind the short preamble the six PLCP bytes to the DQPSK one), then
// to the spreader of the frame's rate
template <class B1, class B2, class B5, class B11>
class TRateSelect {
public:
    TRateSelect(B1* b1, B2* b2, B5* b5, B11* b11, size_t hb1, size_t hb, int rate) : b1_(b1), b2_(b2), b5_(b5), b11_(b11), hb1_(hb1), hb_(hb), at_(0), rate_(rate) {}
    void Reset() { at_ = 0; b1_->Reset(); b2_->Reset(); b5_->Reset(); b11_->Reset(); }
    void Flush() { b1_->Flush(); }                                                         // (the four branches meet in one shaper: Flush once)
    template <class T_IPIN> bool Process(T_IPIN& ipin)
    {
        const size_t k = at_++;
        if (k < hb1_ || (k >= hb_ && rate_ == 1000)) return b1_->Process(ipin);
        if (k < hb_ || rate_ == 2000) return b2_->Process(ipin);
        return rate_ == 5500 ? b5_->Process(ipin) : b11_->Process(ipin);
    }
private:
    B1* b1_; B2* b2_; B5* b5_; B11* b11_; size_t hb1_, hb_, at_; int rate_;
};

static uint32_t crc32_of(const uint8_t* p, size_t n)
{
    uint32_t c = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; i++) { c ^= p[i]; for (int k = 0; k < 8; k++) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1u))); }
    return ~c;
}
static uint16_t crc16_of(const uint8_t* p, size_t n)
{
    uint32_t c = 0xFFFFu;
    for (size_t i = 0; i < n; i++) { c ^= p[i]; for (int k = 0; k < 8; k++) c = (c & 1u) ? (c >> 1) ^ 0x8408u : c >> 1; }
    return (uint16_t)~c;
}

template <class T> static T* dmalloc(size_t count)
{
    T* p = (T*)sora_hip_malloc(count * sizeof(T));
    if (!p) { fprintf(stderr, "device memory: %s\n", sora_hip_last_error()); exit(1); }
    return p;
}

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "%s failed: error_code %08x (%s)\n", #x, ctx.error_code, sora_hip_last_error()); return 1; } } while (0)

int main(int argc, char** argv)
{
    if (argc != 5) { fprintf(stderr, "usage: %s <rate_kbps> <preamble kind> <mpdu.bin> <out.bin>\n", argv[0]); return 2; }
    const int rate = atoi(argv[1]), kind = atoi(argv[2]);
    FILE* f = fopen(argv[3], "rb");
    if (!f) return 1;
    fseek(f, 0, SEEK_END); const long bytes = ftell(f); fseek(f, 0, SEEK_SET);
    std::vector<uint8_t> mpdu((size_t)bytes);
    if (fread(mpdu.data(), 1, mpdu.size(), f) != mpdu.size()) return 1;
    fclose(f);
    if (sora_hip_tx11b_pre_samples((uint32_t)mpdu.size(), (uint32_t)rate, (uint32_t)kind) == 0) { fprintf(stderr, "rate, length or preamble kind not accepted\n"); return 2; }

    // TBB11bSrc: SYNC, SFD, SIGNAL, SERVICE, LENGTH, CRC-16, MPDU, FCS
    const size_t size = mpdu.size() + 4;
    uint32_t us, ext = 0;
    if (rate == 1000) us = (uint32_t)size * 8;
    else if (rate == 2000) us = (uint32_t)size * 4;
    else if (rate == 5500) us = ((uint32_t)size * 16 + 10) / 11;
    else { us = ((uint32_t)size * 8 + 10) / 11; ext = us * 11 - (uint32_t)size * 8 >= 8 ? 1u : 0u; }
    std::vector<uint8_t> ppdu(kind ? 7 : 16, kind ? 0x00 : 0xFF);
    const uint16_t sfd = kind ? 0x05CF : 0xF3A0;
    const uint8_t plcp[4] = { (uint8_t)(rate / 100), (uint8_t)(ext << 7), (uint8_t)us, (uint8_t)(us >> 8) };
    const uint16_t hcrc = crc16_of(plcp, 4);
    ppdu.push_back((uint8_t)sfd); ppdu.push_back((uint8_t)(sfd >> 8));
    ppdu.insert(ppdu.end(), plcp, plcp + 4);
    ppdu.push_back((uint8_t)hcrc); ppdu.push_back((uint8_t)(hcrc >> 8));
    const size_t hb = ppdu.size(), hb1 = kind ? 9 : 24;
    ppdu.insert(ppdu.end(), mpdu.begin(), mpdu.end());
    const uint32_t fcs = crc32_of(mpdu.data(), mpdu.size());
    for (int k = 0; k < 4; k++) ppdu.push_back((uint8_t)(fcs >> (8 * k)));

    CF_Error ctx;
    std::vector<sora_complex8> host;
    uint32_t* d_reg = dmalloc<uint32_t>(4);
    sora_mod11b_state* d_phase = dmalloc<sora_mod11b_state>(1);
    sora_shaper11b_state* d_temps = dmalloc<sora_shaper11b_state>(1);
    const sora_mod11b_state fresh = { 0u, 1u, { 0u, 0u } };                                   // last_phase 0: a fresh context; bEven set, so that TCCK11Encode's Reset has to clear it
    sora_shaper11b_state stale;                                                            // and the shaper's Reset its partial sums
    for (auto& row : stale.temps) for (auto& v : row) { v.re = 1234; v.im = -4321; }
    CHECK(sora_hip_memcpy_h2d(d_phase, &fresh, sizeof(fresh)) == SORA_OK && sora_hip_memcpy_h2d(d_temps, &stale, sizeof(stale)) == SORA_OK);
    uint8_t* d_in = dmalloc<uint8_t>(16); uint8_t* d_scr = dmalloc<uint8_t>(16);
    sora_complex8* d_chips = dmalloc<sora_complex8>(88);
    sora_complex16* d_wide = dmalloc<sora_complex16>(32);
    sora_complex8* d_o8 = dmalloc<sora_complex8>(8);
    uint8_t* d_tabs = dmalloc<uint8_t>(16 * 6);

    // sink first
    TCollect<8> sink(ctx, host);
    THipPackSample16to8<8, CF_Error, decltype(sink)> pack(ctx, &sink, d_o8);
    using Shaper = THip11bQuickPulseShaper<2, CF_Error, decltype(pack)>;
    static_assert(Shaper::kFlushBursts == 3, "20 samples of Flush in three bursts of eight: the last one padded");
    Shaper shaper(ctx, &pack, d_wide, d_tabs, d_temps);
    TReburst<sora_complex8, 88, 2, Shaper> q88(&shaper);
    TReburst<sora_complex8, 44, 2, Shaper> q44(&shaper);
    TReburst<sora_complex8, 16, 2, Shaper> q16(&shaper);
    TReburst<sora_complex8, 8, 2, Shaper> q8(&shaper);
    THip11bDBPSKSpread<1, CF_Error, decltype(q88)> dbpsk(ctx, &q88, d_chips, d_tabs + 16, d_phase);
    THip11bDQPSKSpread<1, CF_Error, decltype(q44)> dqpsk(ctx, &q44, d_chips, d_tabs + 32, d_phase);
    THip11bCCK5Encode<1, CF_Error, decltype(q16)> cck5(ctx, &q16, d_chips, d_tabs + 48, d_phase);
    THip11bCCK11Encode<1, CF_Error, decltype(q8)> cck11(ctx, &q8, d_chips, d_tabs + 64, d_phase);
    using Select = TRateSelect<decltype(dbpsk), decltype(dqpsk), decltype(cck5), decltype(cck11)>;
    Select select(&dbpsk, &dqpsk, &cck5, &cck11, hb1, hb, rate);
    THip11bSc741<1, CF_Error, Select> sc(ctx, &select, d_scr, d_tabs + 80, d_reg, kind ? 0x1B : 0x6C);

    sc.Reset();
    CHECK(ctx.error_code == 0);
    DevicePin<uint8_t, 1> src(d_in);
    for (size_t k = 0; k < ppdu.size(); k++) {
        CHECK(sora_hip_stream_synchronize(nullptr) == SORA_OK);                                // (the pin's buffer is rewritten: one burst in flight)
        CHECK(sora_hip_memcpy_h2d(src.append(), &ppdu[k], 1) == SORA_OK);
        CHECK(sc.Process(src));
    }
    sc.Flush();
    CHECK(ctx.error_code == 0);

    FILE* fo = fopen(argv[4], "wb");
    if (!fo || fwrite(host.data(), sizeof(sora_complex8), host.size(), fo) != host.size()) return 1;
    fclose(fo);
    printf("mod11b chain: %zu PPDU bytes, %zu samples out\n", ppdu.size(), host.size());
    return 0;
}
