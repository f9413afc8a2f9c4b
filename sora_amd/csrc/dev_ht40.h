// dev_ht40.h -- what the 40 MHz HT receiver (k_ht40.hip, k_ht40_stages.hip) and transmitter (k_tx_ht40.hip) state about the format, from IEEE 802.11n-2009
// clause 20: the HT-LTF sequence, the data carriers and the HT interleaver for 40 MHz; and what the receiver's stage entry points add to the bricks of dev_11n.h:
// the unbiased MMSE solve, the pilot phase increment and the front end's derotating decimator.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "dev_11n.h"

namespace sora {

static __constant__ int8_t kHtLtf40[117] = {    // carriers -58..58 (IEEE 802.11n-2009 eq. 20-24)
    1, 1, -1, -1, 1, 1, -1, 1, -1, 1, 1, 1, 1, 1, 1, -1, -1, 1, 1, -1, 1, -1, 1, 1, 1, 1, 1, 1, -1, -1, 1, 1, -1, 1, -1, 1, -1, -1, -1, -1, -1, 1, 1, -1, -1, 1, -1, 1, -1, 1, 1, 1, 1,
    -1, -1, -1, 1, 0, 0, 0, -1, 1, 1, -1,
    1, 1, -1, -1, 1, 1, -1, 1, -1, 1, 1, 1, 1, 1, 1, -1, -1, 1, 1, -1, 1, -1, 1, 1, 1, 1, 1, 1, -1, -1, 1, 1, -1, 1, -1, 1, -1, -1, -1, -1, -1, 1, 1, -1, -1, 1, -1, 1, -1, 1, 1, 1, 1 };
__device__ __forceinline__ int data_bin40(int c)          // data carrier c (0..107) -> FFT bin: -58..-2 then 2..58 without +-11, +-25, +-53
{
    int k;
    if (c < 54) { k = -58 + c; if (k >= -53) k++; if (k >= -25) k++; if (k >= -11) k++; }
    else { k = 2 + (c - 54); if (k >= 11) k++; if (k >= 25) k++; if (k >= 53) k++; }
    return k & 127;
}
__device__ __forceinline__ int deint40_index(int nb, int iss, int k)     // HT interleaver for 40 MHz: where coded bit k of stream iss sits in the symbol
{
    const int s = nb / 2 > 1 ? nb / 2 : 1, nrow = 6 * nb, np = 108 * nb;
    const int i = nrow * (k % 18) + k / 18;
    int j = s * (i / s) + (i + np - (18 * i) / np) % s;
    if (iss > 0) j = ((j - ((iss * 2) % 3 + 3 * (iss / 3)) * 29 * nb) % np + np) % np;
    return j;
}
__device__ __forceinline__ int ltf_sign40(int i)           // FFT bin i (0..127) -> the HT-LTF value of its carrier: +-1 on the 114 occupied carriers, else 0
{
    const int k = i < 64 ? i : i - 128;
    return (k >= -58 && k <= 58) ? (int)kHtLtf40[k + 58] : 0;
}
__device__ __forceinline__ int pilot_bin40(int k)          // pilot k (0..5) of a stream -> FFT bin: carriers -53, -25, -11, 11, 25, 53
{
    const int pk = k == 0 ? -53 : k == 1 ? -25 : k == 2 ? -11 : k == 3 ? 11 : k == 4 ? 25 : 53;
    return pk & 127;
}
// what the transmitter (k_tx_ht40.hip) and the modulation stages (k_mod_ht40.hip) put on the carriers, in units of kTxHt40Amp / 128 per LEVEL (tests/tx_ht40_model.py)
__device__ __forceinline__ int level40(int nb) { return nb <= 2 ? 6144 : nb == 4 ? 4000 : 2214; }   // a data carrier's unit d(N_BPSC): rint(A LEVEL / 128), LEVEL = 48, 48, 31.25, 17.3
constexpr int kPilot40 = 12288;                            // a data pilot: 2 d(1)


// ---- what the stage entry points of k_ht40_stages.hip add to the bricks of dev_11n.h
namespace {
// The unbiased MMSE weights of one carrier, x 2^16: W = diag((W' H)_ss)^-1 W', W' = (H^H H + s2 I)^-1 H^H = adj(G) H^H / det(G), G Hermitian.  This is the solve of
// ht40_frame_body (k_ht40.hip) restated operation for operation, in its order, every product, sum and quotient rounded on its own (contraction off): the stage
// sora_hip_mimo_est_ht40 gives the handle's weights bit for bit (tests/test_gpu_ht40_stages.py).  h = mimo_h_carrier's matrix, s2 > 0.
__device__ __forceinline__ void ht40_mmse_weights(const cpx (&h)[2][2], float s2, cf (&w)[4])
{
#pragma clang fp contract(off)
    const cf a00 = { (float)h[0][0].re, (float)h[0][0].im }, a01 = { (float)h[0][1].re, (float)h[0][1].im };
    const cf a10 = { (float)h[1][0].re, (float)h[1][0].im }, a11 = { (float)h[1][1].re, (float)h[1][1].im };
    auto cj = [](cf a) { return cf{ a.re, -a.im }; };
    auto n2 = [](cf a) { return (a.re * a.re) + (a.im * a.im); };
    const float g00 = (n2(a00) + n2(a10)) + s2, g11 = (n2(a01) + n2(a11)) + s2;
    const cf t0 = cf_mul(cj(a00), a01), t1 = cf_mul(cj(a10), a11);
    const cf g01 = { t0.re + t1.re, t0.im + t1.im };
    const float det = ((g00 * g11) - n2(g01)) / 65536.0f;
    // g11 conj(h_r0) - g01 conj(h_r1)
    auto row0 = [&](cf hc0, cf hc1) { const cf u = cf_mul(g01, hc1); return cf{ ((g11 * hc0.re) - u.re) / det, ((g11 * hc0.im) - u.im) / det }; };
    // g00 conj(h_r1) - g10 conj(h_r0)
    auto row1 = [&](cf hc0, cf hc1) { const cf u = cf_mul(cj(g01), hc0); return cf{ ((g00 * hc1.re) - u.re) / det, ((g00 * hc1.im) - u.im) / det }; };
    cf w00 = row0(cj(a00), cj(a01)), w01 = row0(cj(a10), cj(a11));
    cf w10 = row1(cj(a00), cj(a01)), w11 = row1(cj(a10), cj(a11));
    // unbiased: row s is divided by (W H)_ss, the gain the stream's own symbol comes out with
    const cf e0 = cf_mul(w00, a00), e1 = cf_mul(w01, a10), e2 = cf_mul(w10, a01), e3 = cf_mul(w11, a11);
    const float beta0 = (e0.re + e1.re) / 65536.0f, beta1 = (e2.re + e3.re) / 65536.0f;
    w[0] = { w00.re / beta0, w00.im / beta0 }; w[1] = { w01.re / beta0, w01.im / beta0 };
    w[2] = { w10.re / beta1, w10.im / beta1 }; w[3] = { w11.re / beta1, w11.im / beta1 };
}
// The pilot phase of one data symbol as k_ht40_frame forms it: t_s = the sum of stream s's six dsp_atan16, / 6 in C, through int16; the increment of theta
__device__ __forceinline__ int pilot_inc40(int sum0, int sum1)
{
    const int t0 = (int)(short)(sum0 / 6), t1 = (int)(short)(sum1 / 6);
    return (int)(short)((t0 + t1) >> 1);
}
// The derotating decimator of the 40 MHz front end (k_scan_ht40's fetch): kept sample m is x[2m], negated with saturation when m is odd
__device__ __forceinline__ uint32_t derotate40(uint32_t v, uint32_t m)
{
    if (!(m & 1u)) return v;
    const cpx c = unpack(v);
    return pack(mk(sat16(-c.re), sat16(-c.im)));
}
}  // namespace
}  // namespace sora
