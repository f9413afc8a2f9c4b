// k_ht40_stages.hip -- the 40 MHz HT 2x2 receiver (SURVEY.md section 8(f)1 extension, BASELINE configs[3]), stage level: the bricks of k_ht40_frame (k_ht40.hip) and what
// k_scan_ht40 (k_rx11n.hip) adds to the 802.11n front end, as batched per-stage entry points with the bricks' port shapes (sora_hip_*_ht40).  With sora_hip_freq_comp11n,
// sora_hip_fft128, sora_hip_viterbi11n_ws, sora_hip_desc11a and sora_hip_frame_sink11a the whole receiver stands as stages (sora_amd.rx_ht40_by_stages).
// The arithmetic is stated in dev_11n.h and dev_ht40.h; a kernel here is a brick's piece behind its loads and in front of its stores.
//   sora_hip_data_symbol_ht40   2 x 160 -> 2 x 128, the cyclic prefix of both chains dropped
//   sora_hip_mimo_est_ht40      TMimoChannelEst's combination with the 40 MHz HT-LTF signs; weights: its own inverse (noise_var 0) or the handle's unbiased MMSE
//   sora_hip_mimo_comp_ht40     TMimoChannelComp over 128 bins
//   sora_hip_pilot_track_ht40   TPilotTrack_11n over six pilots per stream, sum / 6
//   sora_hip_demap_ht40         T11nDemap* over the 108 data carriers
//   sora_hip_deinterleave_ht40  the HT interleaver for 40 MHz (N_COL 18, N_ROW 6 N_BPSC, N_ROT 29) inverted
//   sora_hip_stream_join_ht40   TStreamJoin + TStreamConcat over 2 x 108 N_BPSC: the joint coding's de-parser (k_stream_join11n, the same interleave of two byte streams)
//   sora_hip_downsample_ht40    the derotating decimator            sora_hip_noise_var_ht40   sum |Y1 - Y2|^2 over the L-LTF's 52 carriers of both chains, / 416
// All but the tracker stream: one symbol of one chain or stream per 32 lanes, four bins (one 16-byte load and store) per lane where the buffers are 16-byte aligned,
// tables in LDS, byte outputs gathered to 32-bit stores where the buffers are 4-byte aligned.
#include "kernels.h"
#include "dev_11n.h"
#include "dev_ht40.h"
#include "host_stage.h"

namespace sora {

template <int S>
__global__ void k_stream_join11n(const uint8_t* __restrict__ s0, const uint8_t* __restrict__ s1, uint8_t* __restrict__ out, uint64_t total, uint64_t vec_chunks);      // k_11n.hip

namespace {
__device__ __forceinline__ uint4 ld4(const uint32_t* p, bool vec) { return vec ? *reinterpret_cast<const uint4*>(p) : uint4{ p[0], p[1], p[2], p[3] }; }
__device__ __forceinline__ void st4(uint32_t* p, uint4 v, bool vec)
{
    if (vec) *reinterpret_cast<uint4*>(p) = v; else { p[0] = v.x; p[1] = v.y; p[2] = v.z; p[3] = v.w; }
}
}  // namespace

// ---- the cyclic prefix dropped: a thread moves four samples of both chains (k_data_symbol11n's shape at 160 -> 128)
__global__ void __launch_bounds__(256) k_ht40s_data_symbol(const uint32_t* __restrict__ in0, const uint32_t* __restrict__ in1, uint32_t* __restrict__ out0, uint32_t* __restrict__ out1,
        const uint32_t* __restrict__ first, const uint32_t* __restrict__ nsym, const uint32_t* __restrict__ out_first)
{
    const uint32_t f = blockIdx.y, n = min(nsym[f], 1u << 26);
    const size_t src = first[f], dst = (size_t)out_first[f] * 128;
    const bool vin = (((uintptr_t)(in0 + src) | (uintptr_t)(in1 + src)) & 15) == 0, vout = (((uintptr_t)out0 | (uintptr_t)out1) & 15) == 0;
    for (uint32_t m = blockIdx.x * 256 + threadIdx.x; m < n * 32u; m += gridDim.x * 256) {
        const uint32_t k = m >> 5, j = m & 31u;
        const size_t a = src + (size_t)k * 160 + 32 + 4 * j, o = dst + (size_t)k * 128 + 4 * j;
        st4(out0 + o, ld4(in0 + a, vin), vout);
        st4(out1 + o, ld4(in1 + a, vin), vout);
    }
}

// ---- channel matrix and detection weights: one frame per wave, bins lane and lane + 64 (k_ht40_frame's layout).  ltf_r[f][256]: HT-LTF 1 | HT-LTF 2 of chain r after FFT<128>
__global__ void __launch_bounds__(256) k_ht40s_mimo_est(const uint32_t* __restrict__ ltf0, const uint32_t* __restrict__ ltf1, const float* __restrict__ noise_var,
        uint32_t* __restrict__ h, uint32_t* __restrict__ w, uint32_t nframes)
{
    const uint32_t f = blockIdx.x * 4 + (threadIdx.x >> 6); const int lane = threadIdx.x & 63;
    if (f >= nframes) return;
    const float s2 = noise_var ? noise_var[f] : 0.0f;
    const uint32_t* l0 = ltf0 + (size_t)f * 256; const uint32_t* l1 = ltf1 + (size_t)f * 256;
#pragma unroll
    for (int hb = 0; hb < 2; hb++) {
        const int i = lane + 64 * hb, ltf = ltf_sign40(i);
        uint32_t ho[4] = { 0u, 0u, 0u, 0u }, wo[4] = { 0u, 0u, 0u, 0u };       // the 14 bins outside the occupied carriers: 0
        if (ltf != 0) {
            cpx hh[2][2]; cf wf[4];
            mimo_h_carrier(unpack(l0[i]), unpack(l0[128 + i]), unpack(l1[i]), unpack(l1[128 + i]), ltf != 1, hh);
            if (s2 == 0.0f) mimo_inverse(hh, wf);                             // zero forcing: TMimoChannelEst's own inverse
            else ht40_mmse_weights(hh, s2, wf);
            ho[0] = pack(hh[0][0]); ho[1] = pack(hh[0][1]); ho[2] = pack(hh[1][0]); ho[3] = pack(hh[1][1]);
#pragma unroll
            for (int m = 0; m < 4; m++) wo[m] = mimo_weight_pack(wf[m]);
        }
#pragma unroll
        for (int m = 0; m < 4; m++) {
            if (h) h[((size_t)f * 4 + m) * 128 + i] = ho[m];
            w[((size_t)f * 4 + m) * 128 + i] = wo[m];
        }
    }
}

// ---- TMimoChannelComp over 128 bins: 32 lanes per symbol, four bins per lane
__global__ void __launch_bounds__(256) k_ht40s_mimo_comp(const uint32_t* __restrict__ w, const uint32_t* __restrict__ frame_index, const uint32_t* __restrict__ y0,
        const uint32_t* __restrict__ y1, uint32_t* __restrict__ x0, uint32_t* __restrict__ x1, uint32_t nsym, int vec)
{
    const uint32_t s = blockIdx.x * 8 + (threadIdx.x >> 5); const int e = threadIdx.x & 31;
    if (s >= nsym) return;
    const uint32_t* wf = w + (size_t)(frame_index ? frame_index[s] : 0u) * 512 + 4 * e;
    const size_t at = (size_t)s * 128 + 4 * e;
    const uint4 a = ld4(y0 + at, vec), b = ld4(y1 + at, vec);
    const uint4 w00 = ld4(wf, vec), w01 = ld4(wf + 128, vec), w10 = ld4(wf + 256, vec), w11 = ld4(wf + 384, vec);
    const uint32_t av[4] = { a.x, a.y, a.z, a.w }, bv[4] = { b.x, b.y, b.z, b.w };
    const uint32_t c00[4] = { w00.x, w00.y, w00.z, w00.w }, c01[4] = { w01.x, w01.y, w01.z, w01.w };
    const uint32_t c10[4] = { w10.x, w10.y, w10.z, w10.w }, c11[4] = { w11.x, w11.y, w11.z, w11.w };
    uint32_t o0[4], o1[4];
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const cpx p = unpack(av[q]), r = unpack(bv[q]);
        o0[q] = pack(mimo_comp_row(unpack(c00[q]), unpack(c01[q]), p, r));
        o1[q] = pack(mimo_comp_row(unpack(c10[q]), unpack(c11[q]), p, r));
    }
    st4(x0 + at, uint4{ o0[0], o0[1], o0[2], o0[3] }, vec);
    st4(x1 + at, uint4{ o1[0], o1[1], o1[2], o1[3] }, vec);
}

// ---- the pilot phase: one wave per frame, four symbols per pass with 16 lanes each; lane 16 q + 8 s + k (k < 6) takes pilot k of stream s of symbol p + q (k_ht40_frame's
// lanes, four times).  The increments do not depend on theta, so a pass is four of them and a wrapping prefix sum
__global__ void __launch_bounds__(256) k_ht40s_pilot_track(const uint32_t* __restrict__ x0, const uint32_t* __restrict__ x1, const uint32_t* __restrict__ first,
        const uint32_t* __restrict__ nsym, short* __restrict__ state, short* __restrict__ theta_out, uint32_t nframes, const short* __restrict__ atan_tab)
{
    const uint32_t f = blockIdx.x * 4 + (threadIdx.x >> 6); const int lane = threadIdx.x & 63;
    if (f >= nframes) return;
    short* st = state + (size_t)f * 24;
    const int base = st[16 + (lane & 7)];                                      // vfo_theta_i[lane & 7]
    const int base0 = __shfl(base, 0);
    const uint32_t n = (uint32_t)uni((int)nsym[f]), s0 = (uint32_t)uni((int)first[f]);
    const int k = lane & 7, sidx = (lane >> 3) & 1, q = lane >> 4;
    int run = 0;                                                               // the sum of the increments so far
    for (uint32_t p = 0; p < n; p += 4) {
        const uint32_t s = p + (uint32_t)q;
        int th = 0;
        if (s < n && k < 6) {
            const cpx v = unpack((sidx ? x1 : x0)[(size_t)(s0 + s) * 128 + pilot_bin40(k)]);
            th = dsp_atan16(atan_tab, v.re, v.im);
        }
        th += __shfl_xor(th, 1); th += __shfl_xor(th, 2); th += __shfl_xor(th, 4);
        int pre = pilot_inc40(__shfl(th, 16 * q), __shfl(th, 16 * q + 8));     // 0 behind the frame's last symbol
        { const int v = __shfl_up(pre, 16); if (lane >= 16) pre += v; }
        { const int v = __shfl_up(pre, 32); if (lane >= 32) pre += v; }
        if (theta_out && s < n && (lane & 15) == 0) theta_out[s0 + s] = (short)(base0 + run + pre);
        run += __shfl(pre, 63);
    }
    if (lane < 8) st[16 + lane] = (short)(base + run);
}

// ---- T11nDemap*: 32 lanes per symbol.  The symbol goes through LDS (one 16-byte load per lane); lane j < 27 demaps data carriers 4 j .. 4 j + 3 into 4 N_BPSC
// bytes, which leave as N_BPSC 32-bit stores
template <int NB>
__global__ void __launch_bounds__(256) k_ht40s_demap(const uint32_t* __restrict__ in, uint8_t* __restrict__ soft, uint32_t n, int vec_in, int vec_out)
{
    __shared__ uint8_t s_lut[6][256];
    __shared__ uint32_t s_x[8][128];
    fill_demap_luts(s_lut);
    const int g = threadIdx.x >> 5, e = threadIdx.x & 31;
    const uint32_t sym = blockIdx.x * 8 + g;
    if (sym < n) {
        const uint4 v = ld4(in + (size_t)sym * 128 + 4 * e, vec_in);
        s_x[g][4 * e] = v.x; s_x[g][4 * e + 1] = v.y; s_x[g][4 * e + 2] = v.z; s_x[g][4 * e + 3] = v.w;
    }
    __syncthreads();
    if (sym >= n || e >= 27) return;
    uint8_t b[4 * NB];
#pragma unroll
    for (int c = 0; c < 4; c++) demap11n_store(b + c * NB, s_lut, unpack(s_x[g][data_bin40(4 * e + c)]), NB);
    uint8_t* o = soft + ((size_t)sym * 108 + 4 * e) * NB;
    if (vec_out) {
#pragma unroll
        for (int wd = 0; wd < NB; wd++)
            reinterpret_cast<uint32_t*>(o)[wd] = (uint32_t)b[4 * wd] | ((uint32_t)b[4 * wd + 1] << 8) | ((uint32_t)b[4 * wd + 2] << 16) | ((uint32_t)b[4 * wd + 3] << 24);
    } else {
#pragma unroll
        for (int i = 0; i < 4 * NB; i++) o[i] = b[i];
    }
}

// ---- the de-interleaver: the index table (at most 648 entries of 16 bits) built once per workgroup; 32 lanes per symbol, the symbol through LDS, four output bytes
// gathered per 32-bit store
__global__ void __launch_bounds__(256) k_ht40s_deint(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, int nb, int iss, uint32_t n, int aligned)
{
    __shared__ uint16_t s_tab[648];
    __shared__ uint32_t s_in[8][162];
    const int per = 108 * nb, pw = 27 * nb;
    for (int k = threadIdx.x; k < per; k += 256) s_tab[k] = (uint16_t)deint40_index(nb, iss, k);
    const int g = threadIdx.x >> 5, e = threadIdx.x & 31;
    const uint32_t sym = blockIdx.x * 8 + g;
    uint8_t* const sb = reinterpret_cast<uint8_t*>(s_in[g]);
    if (sym < n) {
        const uint8_t* src = in + (size_t)sym * per;
        if (aligned) for (int wd = e; wd < pw; wd += 32) s_in[g][wd] = reinterpret_cast<const uint32_t*>(src)[wd];
        else for (int k = e; k < per; k += 32) sb[k] = src[k];
    }
    __syncthreads();
    if (sym >= n) return;
    uint8_t* dst = out + (size_t)sym * per;
    for (int wd = e; wd < pw; wd += 32) {
        const uint32_t b0 = sb[s_tab[4 * wd]], b1 = sb[s_tab[4 * wd + 1]], b2 = sb[s_tab[4 * wd + 2]], b3 = sb[s_tab[4 * wd + 3]];
        if (aligned) reinterpret_cast<uint32_t*>(dst)[wd] = b0 | (b1 << 8) | (b2 << 16) | (b3 << 24);
        else { dst[4 * wd] = (uint8_t)b0; dst[4 * wd + 1] = (uint8_t)b1; dst[4 * wd + 2] = (uint8_t)b2; dst[4 * wd + 3] = (uint8_t)b3; }
    }
}

// ---- the derotating decimator: a thread makes four kept samples of both chains out of eight raw ones (two 16-byte loads, one 16-byte store).  The stream's last
// group goes sample by sample and reads the even raw samples only: nothing behind raw sample 2 (n - 1) is touched
__global__ void __launch_bounds__(256) k_ht40s_downsample(const uint32_t* __restrict__ in0, const uint32_t* __restrict__ in1, uint32_t* __restrict__ out0, uint32_t* __restrict__ out1,
        const uint32_t* __restrict__ first, const uint32_t* __restrict__ n, const uint32_t* __restrict__ m0, const uint32_t* __restrict__ out_first, uint32_t max_n)
{
    const uint32_t f = blockIdx.y, cnt = min(n[f], max_n), par = m0[f] & 1u;
    const size_t src = first[f], dst = out_first[f];
    const bool vin = (((uintptr_t)(in0 + src) | (uintptr_t)(in1 + src)) & 15) == 0, vout = (((uintptr_t)(out0 + dst) | (uintptr_t)(out1 + dst)) & 15) == 0;
    const uint32_t groups = (cnt + 3u) / 4u;
    for (uint32_t t = blockIdx.x * 256 + threadIdx.x; t < groups; t += gridDim.x * 256) {
        const uint32_t m = 4u * t;
#pragma unroll
        for (int c = 0; c < 2; c++) {
            const uint32_t* s = (c ? in1 : in0) + src + 2 * (size_t)m; uint32_t* d = (c ? out1 : out0) + dst + m;
            if (t + 1 < groups) {
                const uint4 a = ld4(s, vin), b = ld4(s + 4, vin);
                st4(d, uint4{ derotate40(a.x, par), derotate40(a.z, par + 1u), derotate40(b.x, par), derotate40(b.z, par + 1u) }, vout);
            } else
                for (uint32_t i = 0; m + i < cnt; i++) d[i] = derotate40(s[2 * i], par + i);
        }
    }
}

// ---- the noise estimate: one wave per frame, lane = L-LTF carrier; lltf_r[f][128] = the two L-LTF symbols of chain r after FFT<64>
__global__ void __launch_bounds__(256) k_ht40s_noise_var(const uint32_t* __restrict__ l0, const uint32_t* __restrict__ l1, unsigned long long* __restrict__ S_out,
        float* __restrict__ nv_out, uint32_t nframes)
{
    const uint32_t f = blockIdx.x * 4 + (threadIdx.x >> 6); const int lane = threadIdx.x & 63;
    if (f >= nframes) return;
    unsigned long long acc = 0;
    if (lane != 0 && (lane < 27 || lane >= 38)) {                            // the 52 occupied carriers: bins 1..26 and 38..63
#pragma unroll
        for (int r = 0; r < 2; r++) {
            const uint32_t* l = (r ? l1 : l0) + (size_t)f * 128;
            const cpx p = unpack(l[lane]), q = unpack(l[64 + lane]);
            const long long dr = p.re - q.re, di = p.im - q.im;
            acc += (unsigned long long)(dr * dr + di * di);
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) acc += (unsigned long long)__shfl_xor((long long)acc, d);
    if (lane == 0) {
        if (S_out) S_out[f] = acc;
        nv_out[f] = (float)((double)acc / 416.0);                            // S < 2^40: exact in a double; one rounding to single
    }
}

}  // namespace sora

using namespace sora;

// ---- the stage entry points (host_stage.h: the prologue and helpers every stage shares).  n_bpsc and spatial_stream are checked before the prologue here
int sora_hip_data_symbol_ht40(const sora_complex16* d_in0, const sora_complex16* d_in1, const uint32_t* d_first, const uint32_t* d_nsym, const uint32_t* d_out_first,
                              sora_complex16* d_out0, sora_complex16* d_out1, size_t nframes, size_t max_nsym, void* stream)
{
    STAGE_ENTRY("sora_hip_data_symbol_ht40", !d_in0 || !d_in1 || !d_first || !d_nsym || !d_out_first || !d_out0 || !d_out1, nframes)
    if (max_nsym == 0) return SORA_OK;
    if (nframes > 65535 || max_nsym > (1u << 26)) return sora_internal_fail(SORA_ERR_CAPACITY, "sora_hip_data_symbol_ht40: at most 65535 frames of 2^26 symbols per call", 0);
    const unsigned gx = (unsigned)((max_nsym * 32 + 255) / 256);
    hipLaunchKernelGGL(k_ht40s_data_symbol, dim3(gx < 64 ? gx : 64, (unsigned)nframes), dim3(256), 0, (hipStream_t)stream, u32(d_in0), u32(d_in1), u32(d_out0), u32(d_out1),
                       d_first, d_nsym, d_out_first);
    return launch_result("k_ht40s_data_symbol");
}

int sora_hip_mimo_est_ht40(const sora_complex16* d_ltf0, const sora_complex16* d_ltf1, const float* d_noise_var, sora_complex16* d_h, sora_complex16* d_w, size_t nframes,
                           void* stream)
{
    STAGE_ENTRY("sora_hip_mimo_est_ht40", !d_ltf0 || !d_ltf1 || !d_w, nframes)
    hipLaunchKernelGGL(k_ht40s_mimo_est, dim3((unsigned)((nframes + 3) / 4)), dim3(256), 0, (hipStream_t)stream, u32(d_ltf0), u32(d_ltf1), d_noise_var, d_h ? u32(d_h) : nullptr,
                       u32(d_w), (uint32_t)nframes);
    return launch_result("k_ht40s_mimo_est");
}

int sora_hip_mimo_comp_ht40(const sora_complex16* d_w, const uint32_t* d_frame_index, const sora_complex16* d_y0, const sora_complex16* d_y1, sora_complex16* d_x0,
                            sora_complex16* d_x1, size_t nsym, void* stream)
{
    STAGE_ENTRY("sora_hip_mimo_comp_ht40", !d_w || !d_y0 || !d_y1 || !d_x0 || !d_x1, nsym)
    hipLaunchKernelGGL(k_ht40s_mimo_comp, dim3((unsigned)((nsym + 7) / 8)), dim3(256), 0, (hipStream_t)stream, u32(d_w), d_frame_index, u32(d_y0), u32(d_y1), u32(d_x0), u32(d_x1),
                       (uint32_t)nsym, aligned16(d_w, d_y0, d_y1, d_x0, d_x1) ? 1 : 0);
    return launch_result("k_ht40s_mimo_comp");
}

int sora_hip_pilot_track_ht40(const sora_complex16* d_x0, const sora_complex16* d_x1, const uint32_t* d_first, const uint32_t* d_nsym, int16_t* d_state, int16_t* d_theta,
                              size_t nframes, void* stream)
{
    STAGE_ENTRY("sora_hip_pilot_track_ht40", !d_x0 || !d_x1 || !d_first || !d_nsym || !d_state, nframes)
    const uint32_t* sincos = nullptr; const short* atan = nullptr;
    if (sora_internal_dsp_tables(&sincos, &atan) != SORA_OK) return sora_internal_fail(SORA_ERR_HARDWARE_FAILED, "dsp_math table upload failed", 0);
    hipLaunchKernelGGL(k_ht40s_pilot_track, dim3((unsigned)((nframes + 3) / 4)), dim3(256), 0, (hipStream_t)stream, u32(d_x0), u32(d_x1), d_first, d_nsym, d_state, d_theta,
                       (uint32_t)nframes, atan);
    return launch_result("k_ht40s_pilot_track");
}

int sora_hip_demap_ht40(const sora_complex16* d_in, uint8_t* d_soft, int n_bpsc, size_t n, void* stream)
{
    STAGE_NBPSC("sora_hip_demap_ht40", n_bpsc)
    STAGE_ENTRY("sora_hip_demap_ht40", !d_in || !d_soft, n)
    const dim3 grid((unsigned)((n + 7) / 8)); hipStream_t st = (hipStream_t)stream;
    const int vi = aligned16(d_in) ? 1 : 0, vo = aligned4(d_soft) ? 1 : 0;
    STAGE_BY_NBPSC(n_bpsc, k_ht40s_demap, grid, st, u32(d_in), d_soft, (uint32_t)n, vi, vo)
    return launch_result("k_ht40s_demap");
}

int sora_hip_deinterleave_ht40(const uint8_t* d_in, uint8_t* d_out, int n_bpsc, int spatial_stream, size_t n, void* stream)
{
    STAGE_NBPSC("sora_hip_deinterleave_ht40", n_bpsc)
    if (spatial_stream < 0 || spatial_stream > 1) return sora_internal_fail(SORA_ERR_INVALID_PARAM, "sora_hip_deinterleave_ht40: spatial_stream must be 0 or 1", 0);
    STAGE_ENTRY("sora_hip_deinterleave_ht40", !d_in || !d_out, n)
    hipLaunchKernelGGL(k_ht40s_deint, dim3((unsigned)((n + 7) / 8)), dim3(256), 0, (hipStream_t)stream, d_in, d_out, n_bpsc, spatial_stream, (uint32_t)n,
                       aligned4(d_in, d_out) ? 1 : 0);
    return launch_result("k_ht40s_deint");
}

int sora_hip_stream_join_ht40(const uint8_t* d_s0, const uint8_t* d_s1, uint8_t* d_out, int n_bpsc, size_t n, void* stream)
{
    STAGE_NBPSC("sora_hip_stream_join_ht40", n_bpsc)
    STAGE_ENTRY("sora_hip_stream_join_ht40", !d_s0 || !d_s1 || !d_out, n)
    // 108 N_BPSC is a multiple of s for every modulation: the whole call is one interleave of two byte streams, the 802.11n stage's kernel over 216 N_BPSC per symbol
    const uint64_t total = (uint64_t)n * 216 * n_bpsc;
    const uint64_t chunks = aligned16(d_s0, d_s1, d_out) ? total / 96 : 0, tail = total - chunks * 96;
    const uint64_t threads = chunks + (tail < 65536 ? tail : 65536);
    const unsigned grid = (unsigned)((threads + 255) / 256);
    hipStream_t st = (hipStream_t)stream;
    switch (n_bpsc) {
    case 4: hipLaunchKernelGGL(k_stream_join11n<2>, dim3(grid), dim3(256), 0, st, d_s0, d_s1, d_out, total, chunks); break;
    case 6: hipLaunchKernelGGL(k_stream_join11n<3>, dim3(grid), dim3(256), 0, st, d_s0, d_s1, d_out, total, chunks); break;
    default: hipLaunchKernelGGL(k_stream_join11n<1>, dim3(grid), dim3(256), 0, st, d_s0, d_s1, d_out, total, chunks); break;
    }
    return launch_result("k_stream_join11n");
}

int sora_hip_downsample_ht40(const sora_complex16* d_in0, const sora_complex16* d_in1, const uint32_t* d_first, const uint32_t* d_n, const uint32_t* d_m0,
                             const uint32_t* d_out_first, sora_complex16* d_out0, sora_complex16* d_out1, size_t nstreams, size_t max_n, void* stream)
{
    STAGE_ENTRY("sora_hip_downsample_ht40", !d_in0 || !d_in1 || !d_first || !d_n || !d_m0 || !d_out_first || !d_out0 || !d_out1, nstreams)
    if (max_n == 0) return SORA_OK;
    if (nstreams > 65535 || max_n >= (1ull << 31)) return sora_internal_fail(SORA_ERR_CAPACITY, "sora_hip_downsample_ht40: at most 65535 streams of 2^31 - 1 kept samples per call", 0);
    const unsigned gx = (unsigned)((max_n / 4 + 256) / 256);
    hipLaunchKernelGGL(k_ht40s_downsample, dim3(gx < 256 ? gx : 256, (unsigned)nstreams), dim3(256), 0, (hipStream_t)stream, u32(d_in0), u32(d_in1), u32(d_out0), u32(d_out1),
                       d_first, d_n, d_m0, d_out_first, (uint32_t)max_n);
    return launch_result("k_ht40s_downsample");
}

int sora_hip_noise_var_ht40(const sora_complex16* d_lltf0, const sora_complex16* d_lltf1, uint64_t* d_S, float* d_noise_var, size_t nframes, void* stream)
{
    STAGE_ENTRY("sora_hip_noise_var_ht40", !d_lltf0 || !d_lltf1 || !d_noise_var, nframes)
    hipLaunchKernelGGL(k_ht40s_noise_var, dim3((unsigned)((nframes + 3) / 4)), dim3(256), 0, (hipStream_t)stream, u32(d_lltf0), u32(d_lltf1),
                       reinterpret_cast<unsigned long long*>(d_S), d_noise_var, (uint32_t)nframes);
    return launch_result("k_ht40s_noise_var");
}
