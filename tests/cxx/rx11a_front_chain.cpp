// rx11a_front_chain.cpp -- the front of the 802.11a receive graph (CreateDemodGraph11a_40M, kernel/bb/demod11/fb11ademod_config.hpp:169-232) over ONE capture, built from
// the adapters of include/sora_brick.hpp:
//   source pin (bursts of 4 at the 20 MHz rate) -> THip11aDCRemoveEx<1> -> THip11aCCA<1> -> THip11aDCEstimator<1> (its DC back into the remover)      carrier sense
//   144 samples -> sora_hip_lts11a                                                                                                                 T11aLTS
//   80 samples -> THip11aDataSymbol<1> -> the symbol stages (freq_comp11a, fft64, equalize11a, phase_comp11a, pilot11a, demap11a(1), deinterleave11a(1))
//       -> THip11aViterbiSig<1> -> THip11aPLCPParser                                                                                               the SIGNAL symbol
// The host plays TMemSamples' 14-sample source calls and RxThread: a time-out stands until the end of its source call, then both bricks are Reset.
// usage: rx11a_front_chain <file of int16 re, im pairs at the 20 MHz rate>.  Prints the detection point and the parsed SIGNAL fields.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "sora_brick.hpp"

using namespace sora_brick;

template <class T> static T* dmalloc(size_t count)
{
    T* p = (T*)sora_hip_malloc(count * sizeof(T));
    if (!p) { fprintf(stderr, "device memory: %s\n", sora_hip_last_error()); exit(1); }
    return p;
}

// TFreqCompensation .. T11aDeinterleaveBPSK on one symbol, through the stage entry points that exist since the symbol chain was split
template <class T_NEXT>
struct SignalChain {
    const sora_lts11a_ctx* d_ctx; sora_track11a_state* d_trk; uint32_t* d_tab; sora_complex16* d_a; sora_complex16* d_b; uint8_t* d_s; uint8_t* d_soft; T_NEXT* next;
    void Reset() {}
    void Flush() {}
    template <class T_IPIN> bool Process(T_IPIN& ipin)
    {
        const uint32_t tab[2] = { 0u, 1u };
        int rc = sora_hip_memcpy_h2d(d_tab, tab, sizeof(tab));
        if (rc == SORA_OK) rc = sora_hip_freq_comp11a(ipin.peek(), d_ctx, nullptr, d_a, 1, nullptr);
        if (rc == SORA_OK) rc = sora_hip_fft64(d_a, d_b, 1, nullptr);
        if (rc == SORA_OK) rc = sora_hip_equalize11a(d_b, d_ctx, nullptr, d_a, 1, nullptr);
        if (rc == SORA_OK) rc = sora_hip_phase_comp11a(d_a, d_trk, nullptr, d_b, 1, nullptr);
        if (rc == SORA_OK) rc = sora_hip_pilot11a(d_b, d_tab, d_tab + 1, d_trk, d_a, 1, nullptr);
        if (rc == SORA_OK) rc = sora_hip_demap11a(d_a, d_s, 1, 1, nullptr);
        if (rc == SORA_OK) rc = sora_hip_deinterleave11a(d_s, d_soft, 1, 1, nullptr);
        ipin.pop();
        if (rc != SORA_OK) { fprintf(stderr, "symbol chain: %s\n", sora_hip_last_error()); return false; }
        DevicePin<uint8_t, 48> soft(d_soft); soft.append();
        return next->Process(soft);
    }
};

int main(int argc, char** argv)
{
    if (argc < 2) { fprintf(stderr, "usage: %s capture.i16\n", argv[0]); return 2; }
    if (sora_hip_device_count() <= 0) { fprintf(stderr, "no HIP device\n"); return 2; }
    FILE* fh = fopen(argv[1], "rb");
    if (!fh) { perror(argv[1]); return 2; }
    std::vector<sora_complex16> x;
    sora_complex16 buf[1024]; size_t got;
    while ((got = fread(buf, sizeof(sora_complex16), 1024, fh)) > 0) x.insert(x.end(), buf, buf + got);
    fclose(fh);
    const uint32_t n20 = (uint32_t)x.size();
    sora_complex16* d_x = dmalloc<sora_complex16>(n20 + 16);
    if (sora_hip_memcpy_h2d(d_x, x.data(), n20 * sizeof(sora_complex16)) != SORA_OK) { fprintf(stderr, "%s\n", sora_hip_last_error()); return 1; }
    // ---- carrier sense, sink first
    uint32_t* d_tab = dmalloc<uint32_t>(64);
    sora_complex16* d_pi = dmalloc<sora_complex16>(16); sora_complex16* d_gated = dmalloc<sora_complex16>(16);
    sora_cca11a_state* d_cca = dmalloc<sora_cca11a_state>(1); sora_dcest11a_state* d_est = dmalloc<sora_dcest11a_state>(1);
    CF_Error err; CF_11aCCA cca_ctx;
    THip11aCCA<1> cca(cca_ctx, d_cca, d_gated, d_tab + 8);
    THip11aDCEstimator<1> est(d_est, d_tab + 16);
    // TCCA11a -> TDCEstimator behind the remover, and the estimate's way back into it (the remover's next brick names the remover: the knot is tied through a pointer)
    THip11aDCRemoveEx<1, CF_Error, struct Knot>* remover_ptr = nullptr;
    struct Knot {
        THip11aCCA<1>& cca; THip11aDCEstimator<1>& est; THip11aDCRemoveEx<1, CF_Error, Knot>** remover;
        void Reset() {}
        void Flush() {}
        bool Process(DevicePin<sora_complex16, 4>& ipin)
        {
            if (!cca.Process(ipin)) return false;
            if (cca.npass()) { if (!est.Process(cca.opin(), cca.npass())) return false; (*remover)->SetDC(est.DC()); }
            else cca.opin().clear();
            return true;
        }
    } knot{ cca, est, &remover_ptr };
    THip11aDCRemoveEx<1, CF_Error, Knot> remover(err, &knot, d_pi, d_tab);
    remover_ptr = &remover;
    uint32_t p = 0; bool detected = false;
    while (p + 4 <= n20) {
        DevicePin<sora_complex16, 4> src(d_x + p); src.append();
        if (!remover.Process(src) || err.error_code) { fprintf(stderr, "carrier sense: 0x%x %s\n", err.error_code | cca_ctx.error_code, sora_hip_last_error()); return 1; }
        p += 4;
        if (cca_ctx.cca_state == 1) { detected = true; break; }
        if (p + 4 > (p + 13) / 14 * 14 && cca_ctx.error_code == (uint32_t)SORA_E_CS_TIMEOUT) {      // RxThread at the end of the source call
            if (!cca.Reset() || !est.Reset()) { fprintf(stderr, "reset: %s\n", sora_hip_last_error()); return 1; }
        }
    }
    if (!detected || p + 224 > n20) { printf("detected=0\n"); return 0; }
    // ---- T11aLTS, then the SIGNAL symbol
    sora_lts11a_ctx* d_ctx = dmalloc<sora_lts11a_ctx>(1); sora_track11a_state* d_trk = dmalloc<sora_track11a_state>(1);
    sora_track11a_state trk; memset(&trk, 0, sizeof(trk));
    trk.symbol_count = 127; for (auto& c : trk.comp) c.re = 0x7FFF;                     // CF_PhaseCompensate / CF_PilotTrack after Reset (pilot.hpp:143-152)
    sora_lts11a_ctx ctx;
    if (sora_hip_lts11a(d_x + p, d_ctx, 1, nullptr) != SORA_OK || sora_hip_memcpy_h2d(d_trk, &trk, sizeof(trk)) != SORA_OK || sora_hip_stream_synchronize(nullptr) != SORA_OK ||
        sora_hip_memcpy_d2h(&ctx, d_ctx, sizeof(ctx)) != SORA_OK) { fprintf(stderr, "lts: %s\n", sora_hip_last_error()); return 1; }
    sora_complex16* d_sym = dmalloc<sora_complex16>(64); sora_complex16* d_a = dmalloc<sora_complex16>(64); sora_complex16* d_b = dmalloc<sora_complex16>(64);
    uint8_t* d_s = dmalloc<uint8_t>(64); uint8_t* d_soft = dmalloc<uint8_t>(64); uint32_t* d_sig = dmalloc<uint32_t>(4); sora_plcp11a_rec* d_rec = dmalloc<sora_plcp11a_rec>(1);
    CF_11aPLCP plcp;
    THip11aPLCPParser parser(plcp, d_rec);
    THip11aViterbiSig<1, CF_Error, THip11aPLCPParser> vit(err, &parser, d_sig);
    SignalChain<decltype(vit)> chain{ d_ctx, d_trk, d_tab + 24, d_a, d_b, d_s, d_soft, &vit };
    THip11aDataSymbol<1, CF_Error, decltype(chain)> symbol(err, &chain, d_sym, d_tab + 32);
    DevicePin<sora_complex16, 80> sig(d_x + p + 144); sig.append();
    if (!symbol.Process(sig) || err.error_code) { fprintf(stderr, "SIGNAL: 0x%x %s\n", err.error_code, sora_hip_last_error()); return 1; }
    printf("detected=1 start=%u cfo_est=%d error_code=0x%x rate_kbps=%u length=%u code_rate=%u total_symbols=%u remain_symbols=%u plcp_state=%u peak_index=%u\n", p, (int)ctx.cfo_est,
           plcp.error_code, plcp.data_rate_kbps, plcp.frame_length, plcp.code_rate, plcp.total_symbols, plcp.remain_symbols, plcp.plcp_state, cca_ctx.cca_peak_index);
    return 0;
}
