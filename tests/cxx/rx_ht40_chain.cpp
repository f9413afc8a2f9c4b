// rx_ht40_chain.cpp -- the data field of ONE described 40 MHz HT two-stream frame (per-stream coding; what sora_ht40_process_dev decodes), built from the adapters of
// include/sora_brick.hpp over the stage entry points:
//   HT-LTF 1 / 2:  sora_hip_freq_comp11n -> THipHt40DataSymbol<2> -> THipFFT128<4> -> THipHt40MimoEst
//   each symbol:   sora_hip_freq_comp11n -> THipHt40DataSymbol<1> -> THipFFT128<2> -> THipHt40MimoComp<1> -> THipHt40PilotTrack<1>     (theta of symbol d rotates symbol d + 1)
//   each stream:   THipHt40Demap<NB, 1> -> THipHt40Deinterleave<NB, s, 1> per symbol, then sora_hip_viterbi11n_ws -> sora_hip_desc11a -> sora_hip_frame_sink11a
// usage: rx_ht40_chain <file: chain 0's int16 re, im pairs from the first sample of HT-LTF 1 to the frame's end, then chain 1's> n_bpsc code_rate len0 len1 cfo noise_var
// Prints theta after the last symbol, both rows' error code and FCS, and a checksum of the de-interleaved soft bytes.
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
static void must(int rc, const char* what) { if (rc != SORA_OK) { fprintf(stderr, "%s: %s\n", what, sora_hip_last_error()); exit(1); } }
template <class T> static void up(T* d, const T* h, size_t n) { must(sora_hip_memcpy_h2d(d, h, n * sizeof(T)), "upload"); }

// one symbol's demapped, de-interleaved bytes of both streams appended at soft[s] + at
template <int NB>
static void demap_symbol(CF_Error& err, const sora_complex16* d_xs, uint8_t* d_raw, uint8_t* const d_soft[2], size_t at)
{
    for (int s = 0; s < 2; s++) {
        using Deint0 = THipHt40Deinterleave<NB, 0, 1, CF_Error, TDrop<CF_Error>>; using Deint1 = THipHt40Deinterleave<NB, 1, 1, CF_Error, TDrop<CF_Error>>;
        DevicePin<sora_complex16, 128> pin(const_cast<sora_complex16*>(d_xs) + 128 * s); pin.append();
        bool ok;
        if (s == 0) { Deint0 de(err, nullptr, d_soft[0] + at); THipHt40Demap<NB, 1, CF_Error, Deint0> dm(err, &de, d_raw); ok = dm.Process(pin); }
        else { Deint1 de(err, nullptr, d_soft[1] + at); THipHt40Demap<NB, 1, CF_Error, Deint1> dm(err, &de, d_raw); ok = dm.Process(pin); }
        if (!ok || err.error_code) { fprintf(stderr, "demap / de-interleave: %s\n", sora_hip_last_error()); exit(1); }
    }
}

int main(int argc, char** argv)
{
    if (argc < 8) { fprintf(stderr, "usage: %s frame.i16 n_bpsc code_rate len0 len1 cfo noise_var\n", argv[0]); return 2; }
    if (sora_hip_device_count() <= 0) { fprintf(stderr, "no HIP device\n"); return 2; }
    const int nb = atoi(argv[2]), cr = atoi(argv[3]); const uint32_t len[2] = { (uint32_t)atoi(argv[4]), (uint32_t)atoi(argv[5]) };
    const int cfo = atoi(argv[6]); const float noise_var = (float)atof(argv[7]);
    const uint32_t nsym = sora_ht40_symbols(len[0], len[1], (uint32_t)nb, (uint32_t)cr);
    if (nsym == 0) { fprintf(stderr, "bad descriptor\n"); return 2; }
    FILE* fh = fopen(argv[1], "rb");
    if (!fh) { perror(argv[1]); return 2; }
    std::vector<sora_complex16> x;
    sora_complex16 buf[1024]; size_t got;
    while ((got = fread(buf, sizeof(sora_complex16), 1024, fh)) > 0) x.insert(x.end(), buf, buf + got);
    fclose(fh);
    const uint32_t n = (uint32_t)(x.size() / 2);
    if (n < 160 * (2 + nsym)) { fprintf(stderr, "the file is shorter than the frame\n"); return 2; }
    // both chains in ONE buffer, chain 1 behind chain 0: a symbol of both chains is then the adapters' "two halves" burst after one copy
    sora_complex16* d_x = dmalloc<sora_complex16>(2 * n); up(d_x, x.data(), 2 * (size_t)n);
    sora_complex16* d_c = dmalloc<sora_complex16>(2 * n);                        // TFreqComp_11n's output, the same layout
    sora_complex16* d_sym = dmalloc<sora_complex16>(2 * 320);                    // up to two symbols of both chains: chain 0's, then chain 1's
    sora_complex16* d_y = dmalloc<sora_complex16>(512); sora_complex16* d_f = dmalloc<sora_complex16>(512);
    sora_complex16* d_w = dmalloc<sora_complex16>(512); sora_complex16* d_h = dmalloc<sora_complex16>(512); sora_complex16* d_xs = dmalloc<sora_complex16>(256);
    uint32_t* d_tab = dmalloc<uint32_t>(64); int16_t* d_state = dmalloc<int16_t>(24); int16_t* d_theta = dmalloc<int16_t>(4); float* d_nv = dmalloc<float>(1);
    const size_t per = (size_t)nsym * 108 * nb;
    uint8_t* d_raw = dmalloc<uint8_t>(648); uint8_t* d_soft_all = dmalloc<uint8_t>(2 * per + 64); uint8_t* const d_soft[2] = { d_soft_all, d_soft_all + per };
    int16_t st[24];
    for (int k = 0; k < 8; k++) { st[k] = (int16_t)(k * cfo); st[8 + k] = (int16_t)(8 * cfo); st[16 + k] = 0; }
    up(d_state, st, 24); up(d_nv, &noise_var, 1);
    CF_Error err;
    // TFreqComp_11n over `bursts` bursts of 8 samples from sample `first` of both chains, then the symbols' samples of chain 0 and of chain 1 side by side in d_sym
    auto comp = [&](uint32_t first, uint32_t bursts) {
        const uint32_t t[2] = { first, bursts };
        up(d_tab + 32, t, 2);
        must(sora_hip_freq_comp11n(d_x, d_x + n, d_c, d_c + n, d_tab + 32, d_tab + 33, d_state, 1, bursts, nullptr), "freq_comp11n");
        must(sora_hip_memcpy_d2d(d_sym, d_c + first, 8 * bursts * sizeof(sora_complex16), nullptr), "copy");
        must(sora_hip_memcpy_d2d(d_sym + 8 * bursts, d_c + n + first, 8 * bursts * sizeof(sora_complex16), nullptr), "copy");
    };
    // ---- the two HT-LTF symbols: the burst THipHt40MimoEst takes is chain 0's two transforms, then chain 1's -- what FFT<128> x 4 leaves behind DataSymbol<2>
    {
        THipHt40MimoEst<CF_Error, TDrop<CF_Error>> est(err, nullptr, d_w, noise_var != 0.0f ? d_nv : nullptr, d_h);
        THipFFT128<4, CF_Error, decltype(est)> fft(err, &est, d_f);
        THipHt40DataSymbol<2, CF_Error, decltype(fft)> sym(err, &fft, d_y, d_tab);
        comp(0, 40);
        DevicePin<sora_complex16, 640> pin(d_sym); pin.append();
        if (!sym.Process(pin) || err.error_code) { fprintf(stderr, "HT-LTF: 0x%x %s\n", err.error_code, sora_hip_last_error()); return 1; }
    }
    // ---- the data symbols
    {
        THipHt40PilotTrack<1, CF_Error, TDrop<CF_Error>> track(err, nullptr, d_state, d_theta, d_tab + 8);
        THipHt40MimoComp<1, CF_Error, decltype(track)> mcomp(err, &track, d_w, d_xs);
        THipFFT128<2, CF_Error, decltype(mcomp)> fft(err, &mcomp, d_f);
        THipHt40DataSymbol<1, CF_Error, decltype(fft)> sym(err, &fft, d_y, d_tab + 16);
        for (uint32_t d = 0; d < nsym; d++) {
            comp(320 + 160 * d, 20);
            DevicePin<sora_complex16, 320> pin(d_sym); pin.append();
            if (!sym.Process(pin) || err.error_code) { fprintf(stderr, "symbol %u: 0x%x %s\n", d, err.error_code, sora_hip_last_error()); return 1; }
            const size_t at = (size_t)d * 108 * nb;
            switch (nb) {
            case 1: demap_symbol<1>(err, d_xs, d_raw, d_soft, at); break;
            case 2: demap_symbol<2>(err, d_xs, d_raw, d_soft, at); break;
            case 4: demap_symbol<4>(err, d_xs, d_raw, d_soft, at); break;
            default: demap_symbol<6>(err, d_xs, d_raw, d_soft, at); break;
            }
        }
    }
    // ---- T11aViterbi<.., 192, 36> per stream, T11aDesc, TBB11aFrameSink
    const size_t ws_bytes = sora_hip_viterbi11n_workspace_bytes(2 * per + 64, 2);
    uint8_t* d_ws = dmalloc<uint8_t>(ws_bytes); uint8_t* d_dec = dmalloc<uint8_t>(2 * 4352); uint8_t* d_psdu = dmalloc<uint8_t>(2 * 4096);
    sora_sink11a_rec* d_rec = dmalloc<sora_sink11a_rec>(2);
    const uint32_t soft_off[2] = { 0u, (uint32_t)per }, nsoft[2] = { (uint32_t)per, (uint32_t)per }, dec_off[2] = { 0u, 4352u }, out_off[2] = { 0u, 4096u };
    const uint16_t flen[2] = { (uint16_t)len[0], (uint16_t)len[1] };
    up(d_tab + 40, soft_off, 2); up(d_tab + 42, nsoft, 2); up(d_tab + 44, dec_off, 2); up(d_tab + 46, out_off, 2); up(d_tab + 48, len, 2);
    uint16_t* d_flen = dmalloc<uint16_t>(2); up(d_flen, flen, 2);
    must(sora_hip_viterbi11n_ws(d_soft_all, 2 * per + 64, d_tab + 40, d_tab + 42, d_flen, cr, d_dec, d_tab + 44, 2, d_ws, ws_bytes, 0, nullptr), "viterbi11n_ws");
    must(sora_hip_desc11a(d_dec, d_tab + 44, d_tab + 48, d_psdu, d_tab + 46, 2, nullptr), "desc11a");
    must(sora_hip_frame_sink11a(d_psdu, d_tab + 46, d_tab + 48, d_rec, 2, nullptr), "frame_sink11a");
    must(sora_hip_stream_synchronize(nullptr), "synchronize");
    sora_sink11a_rec rec[2]; int16_t state[24]; std::vector<uint8_t> soft(2 * per);
    must(sora_hip_memcpy_d2h(rec, d_rec, sizeof(rec)), "rows"); must(sora_hip_memcpy_d2h(state, d_state, sizeof(state)), "state");
    must(sora_hip_memcpy_d2h(soft.data(), d_soft_all, 2 * per), "soft");
    uint32_t sum = 0;
    for (size_t i = 0; i < 2 * per; i++) sum = sum * 31u + soft[i];
    printf("nsym=%u theta=%d error0=0x%x fcs0=0x%08x error1=0x%x fcs1=0x%08x soft_checksum=0x%08x\n", nsym, (int)state[16], rec[0].error_code, rec[0].frame_crc32,
           rec[1].error_code, rec[1].frame_crc32, sum);
    return 0;
}
