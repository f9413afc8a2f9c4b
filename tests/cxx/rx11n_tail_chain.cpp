// rx11n_tail_chain.cpp -- the tail of the 802.11n 2x2 receive graph (CreateDemodGraph11n, kernel/bb/demod11/fb11ndemod_config.hpp:199-213) built from the adapters of
// include/sora_brick.hpp, sink first and in the reference's order:
//   source pin (the de-interleaved soft values of spatial stream 0, then 1) -> THip11nStreamJoin<2, NSYM> -> the trellis stage (sora_hip_viterbi11n_ws) -> THip11aDesc
//       -> THip11aFrameSink
// The host plays the transmitter for one MCS 9 frame (QPSK, rate 1/2, N_DBPS 104): SERVICE + a 96-byte payload + FCS, scrambled by the descrambler's own byte walk
// (scramble.hpp:269-355 run forwards), convolutionally encoded (133, 171), stream-parsed bit by bit as TStreamFork does it for BPSK and QPSK; a coded 1 is the soft value 7.
// Prints error_code, crc32 and length of the frame the sink reports.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "sora_brick.hpp"

using namespace sora_brick;

constexpr int kNbpsc = 2, kLength = 100;
constexpr size_t kSym = (8 * (kLength + 2) + 6 + 103) / 104;                       // 8 OFDM symbols

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

// T11aViterbi<5000 * 8, 312, 192, 36> as a brick over the stage entry point: one burst = the whole frame's soft values
template <size_t NSOFT, class T_CTX, class T_NEXT>
class TTrellis11n : public HipFilter<T_CTX, T_NEXT> {
public:
    TTrellis11n(T_CTX& ctx, T_NEXT* next, uint8_t* d_out, uint32_t* d_tab, void* d_ws, size_t ws_bytes)
        : HipFilter<T_CTX, T_NEXT>(ctx, next, nullptr), opin_(d_out), d_tab_(d_tab), d_ws_(d_ws), ws_bytes_(ws_bytes) {}
    template <class T_IPIN> bool Process(T_IPIN& ipin)
    {
        while (ipin.check_read()) {
            const uint32_t tab[4] = { 0u, (uint32_t)NSOFT, (uint32_t)kLength, 0u };               // soft_off, nsoft, frame_len (uint16), out_off
            if (sora_hip_memcpy_h2d(d_tab_, tab, sizeof(tab)) != SORA_OK) return this->raise(SORA_ERR_HARDWARE_FAILED);
            if (!this->raise(sora_hip_viterbi11n_ws(ipin.peek(), NSOFT, d_tab_, d_tab_ + 1, reinterpret_cast<const uint16_t*>(d_tab_ + 2), 0, opin_.append(), d_tab_ + 3, 1,
                                                    d_ws_, ws_bytes_, 0, nullptr))) return false;
            ipin.pop();
            if (this->next_ && !this->next_->Process(opin_)) return false;
        }
        return true;
    }
private:
    DevicePin<uint8_t, kLength + 2> opin_; uint32_t* d_tab_; void* d_ws_; size_t ws_bytes_;
};

int main()
{
    if (sora_hip_device_count() <= 0) { fprintf(stderr, "no HIP device\n"); return 2; }
    // ---- the transmitter's part
    uint8_t dec[kLength + 2] = { 0x5A, 0xB6 };                                     // the scrambled SERVICE field: byte 1 >> 1 is the descrambler's seed
    uint8_t psdu[kLength];
    for (int i = 0; i < kLength - 4; i++) psdu[i] = (uint8_t)(37 * i + 11);
    const uint32_t fcs = crc32_of(psdu, kLength - 4);
    memcpy(psdu + kLength - 4, &fcs, 4);
    uint8_t lut[128];
    for (int i = 0; i < 128; i++) {
        uint8_t x = (uint8_t)(i << 1);
        for (int k = 0; k < 8; k++) { const uint8_t o1 = ((x >> 1) ^ (x >> 4)) & 1; x = (uint8_t)((x >> 1) | (o1 << 7)); }
        lut[i] = x;
    }
    uint8_t reg = dec[1] >> 1;
    for (int i = 0; i < kLength; i++) { reg = lut[reg]; dec[2 + i] = psdu[i] ^ reg; reg >>= 1; }
    constexpr size_t kBits = kSym * 104, kPerStream = kSym * 52 * kNbpsc;
    std::vector<uint8_t> soft(2 * kPerStream);                                      // stream 0's symbols, then stream 1's: the join adapter's input burst
    unsigned sr = 0;
    for (size_t n = 0; n < kBits; n++) {
        const unsigned bit = n < 8 * sizeof(dec) ? (dec[n >> 3] >> (n & 7)) & 1u : 0u;              // tail and pad bits: 0
        sr = (sr >> 1) | (bit << 6);
        soft[n] = (uint8_t)(7 * (__builtin_popcount(sr & 0133) & 1));                              // A to stream 0, B to stream 1
        soft[kPerStream + n] = (uint8_t)(7 * (__builtin_popcount(sr & 0171) & 1));
    }
    // ---- the graph, sink first
    uint8_t* d_in = dmalloc<uint8_t>(soft.size()); uint8_t* d_joined = dmalloc<uint8_t>(soft.size());
    uint8_t* d_dec = dmalloc<uint8_t>(4096); uint8_t* d_mpdu = dmalloc<uint8_t>(4096);
    uint32_t* d_tab = dmalloc<uint32_t>(16); sora_sink11a_rec* d_rec = dmalloc<sora_sink11a_rec>(1);
    const size_t ws_bytes = sora_hip_viterbi11n_workspace_bytes(soft.size(), 1);
    void* d_ws = dmalloc<uint8_t>(ws_bytes + 16);
    if (sora_hip_memcpy_h2d(d_in, soft.data(), soft.size()) != SORA_OK) { fprintf(stderr, "%s\n", sora_hip_last_error()); return 1; }
    CF_Error ctx; CF_11aSink sink_ctx;
    THip11aFrameSink sink(sink_ctx, d_rec, d_tab + 8);
    THip11aDesc<CF_Error, THip11aFrameSink> desc(ctx, &sink, d_mpdu, d_tab + 4);
    TTrellis11n<2 * kPerStream, CF_Error, decltype(desc)> trellis(ctx, &desc, d_dec, d_tab, d_ws, ws_bytes);
    THip11nStreamJoin<kNbpsc, kSym, CF_Error, decltype(trellis)> join(ctx, &trellis, d_joined);
    desc.SetFrame(kLength); sink.SetFrame(kLength);
    DevicePin<uint8_t, 2 * kPerStream> src(d_in);
    src.append();
    const bool more = join.Process(src);                                            // false: the sink has decided, as TBB11aFrameSink's Process returns
    if (ctx.error_code) { fprintf(stderr, "stage error 0x%x: %s\n", ctx.error_code, sora_hip_last_error()); return 1; }
    uint8_t mpdu[kLength];
    if (sora_hip_memcpy_d2h(mpdu, d_mpdu, kLength) != SORA_OK || memcmp(mpdu, psdu, kLength) != 0) { fprintf(stderr, "the descrambled bytes are not the PSDU\n"); return 1; }
    printf("decided=%d error_code=0x%x crc32=0x%08x length=%d\n", more ? 0 : 1, sink_ctx.error_code, crc32_of(mpdu, kLength - 4), kLength);
    if (sink_ctx.frame_crc32 != fcs) { fprintf(stderr, "frame_crc32 0x%08x is not the FCS 0x%08x\n", sink_ctx.frame_crc32, fcs); return 1; }
    for (void* p : { (void*)d_in, (void*)d_joined, (void*)d_dec, (void*)d_mpdu, (void*)d_tab, (void*)d_rec, d_ws }) sora_hip_free(p);
    return 0;
}
