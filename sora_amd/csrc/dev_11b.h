// dev_11b.h -- the arithmetic of the 802.11b receive graph's bricks (CreateDemodGraph, kernel/bb/demod11/fb11bdemod_config.hpp:122-172) as device functions, one brick
// step each, for the stage kernels of k_11b.hip.  (k_rx11b.hip, the handle's whole-capture form, keeps its own statement of the same bricks.)  Every sum wraps where the
// brick's SSE operator wraps: int16 through w16, int32 through unsigned arithmetic.  tests/cxx/rx11b_stage_model.c is the same text in C.
#pragma once
#include "dev_arith.h"

namespace sora {

enum { k11bRateSync = 0, k11bRate1M, k11bRate2M, k11bRate5p5M, k11bRate11M };
enum { k11bNoPeak = 0, k11bPeakFound, k11bPeakValid, k11bPeakValided, k11bBarkerSynced };
constexpr uint32_t kE11bFrameOk = 0x00000001u, kE11bSfdFail = 0x80000004u, kE11bPlcpFail = 0x80000005u, kE11bCrc32Fail = 0x80000006u, kE11bCsTimeout = 0x80000007u,
                   kE11bSfdTimeout = 0x80000008u, kE11bSyncTimeout = 0x80000009u;

__device__ __forceinline__ int wadd32(int a, int b) { return (int)((unsigned)a + (unsigned)b); }
__device__ __forceinline__ int wsub32(int a, int b) { return (int)((unsigned)a - (unsigned)b); }
__device__ __forceinline__ int wneg32(int a) { return (int)(0u - (unsigned)a); }
__device__ __forceinline__ int wmul32(int a, int b) { return (int)((unsigned)a * (unsigned)b); }
__device__ __forceinline__ cpx cadd16(cpx a, cpx b) { return mk(w16(a.re + b.re), w16(a.im + b.im)); }
__device__ __forceinline__ cpx csub16(cpx a, cpx b) { return mk(w16(a.re - b.re), w16(a.im - b.im)); }

// ---- TBB11bDespread::QuickBarkerDespread (barkerspread.hpp:277-303): chips 1 and 4 are negated BEFORE the >> 4, chips 8-10 subtracted after it; c = 11 packed chips at
// a stride of `stride` words
__device__ __forceinline__ uint32_t b11_despread(const uint32_t* c, int stride = 1)
{
    cpx a[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        cpx v = unpack(c[k * stride]); if (k == 1) v = mk(neg16(v.re), neg16(v.im));
        a[k] = sra(v, 4);
    }
#pragma unroll
    for (int k = 0; k < 4; k++) {
        cpx v = unpack(c[(4 + k) * stride]); if (k == 0) v = mk(neg16(v.re), neg16(v.im));
        a[k] = cadd16(a[k], sra(v, 4));
    }
#pragma unroll
    for (int k = 0; k < 3; k++) a[k] = csub16(a[k], sra(unpack(c[(8 + k) * stride]), 4));
    return pack(mk(w16(a[0].re + a[1].re + a[2].re + a[3].re), w16(a[0].im + a[1].im + a[2].im + a[3].im)));
}

// (ulong)(ref.re * x.re + ref.im * x.im) >> 31: the DBPSK bit of TDBPSKDemap and TSFDSync
__device__ __forceinline__ uint32_t b11_dot_sign(cpx ref, cpx x) { return (uint32_t)wadd32(ref.re * x.re, ref.im * x.im) >> 31; }

// the two DQPSK bits of x against ref (TDQPSKDemap: SH = 0; demap_dqpsk_bits of the CCK decoders, core/inc/soradsp.h:190-198: SH = 1)
template <int SH>
__device__ __forceinline__ uint32_t b11_dqpsk_bits(cpx ref, cpx x)
{
    const int re = wadd32(ref.re * x.re, ref.im * x.im) >> SH, im = wsub32(ref.re * x.im, ref.im * x.re) >> SH;
    return ((uint32_t)wadd32(re, im) >> 31) | (((uint32_t)wsub32(re, im) >> 31) << 1);
}

// ---- CCK (cck.hpp).  a * j^k; with k a constant the selects fold, with k per lane (the pruned search's third module) they stay selects: no branch
__device__ __forceinline__ cpx b11_rot(cpx a, int k)
{
    const bool sw = k & 1, nre = ((k + 1) & 2) != 0, nim = (k & 2) != 0;       // k = 1: (-im, re), 2: (-re, -im), 3: (im, -re) -- components are sums of int16: no wrap
    const int re = sw ? a.im : a.re, im = sw ? a.re : a.im;
    return mk(nre ? -re : re, nim ? -im : im);
}
__device__ __forceinline__ cpx b11_add32(cpx a, cpx b) { return mk(wadd32(a.re, b.re), wadd32(a.im, b.im)); }
// A1 = P1 + r P0, A2 = r P2 - P3, A3 = P5 + r P4, A4 = P7 - r P6 with r = (-j)^m = j^k (cck.hpp:268-275, 392-399, 514-521, 635-642; 81-88, 103-110)
__device__ __forceinline__ void b11_cck_partial(const cpx P[8], int k, cpx A[4])
{
    A[0] = b11_add32(P[1], b11_rot(P[0], k));
    A[1] = b11_add32(b11_rot(P[2], k), b11_rot(P[3], 2));
    A[2] = b11_add32(P[5], b11_rot(P[4], k));
    A[3] = b11_add32(P[7], b11_rot(P[6], k + 2));
}
// one "Module" of CCK11_DECODER (e.g. cck.hpp:277-390): L = conj((A2 + q A1) >> 2) * ((A4 + q A3) >> 2) for q = 1, j, -1, -j (value bits 0x00, 0x30, 0x10, 0x20); the
// larger of |re|, |im| picks phi4; then the reference's comparison tree with its strict comparisons
__device__ __forceinline__ void b11_cck11_module(const cpx A[4], int& mm, uint32_t& vv)
{
    int M[4]; uint32_t V[4];
#pragma unroll
    for (int s = 0; s < 4; s++) {
        const uint32_t base = s == 0 ? 0x00u : s == 1 ? 0x30u : s == 2 ? 0x10u : 0x20u;
        const cpx bx = sra(b11_add32(A[1], b11_rot(A[0], s)), 2), by = sra(b11_add32(A[3], b11_rot(A[2], s)), 2);
        const int lre = wadd32(wmul32(bx.re, by.re), wmul32(bx.im, by.im)), lim = wsub32(wmul32(bx.re, by.im), wmul32(bx.im, by.re));
        const int a1 = lre < 0 ? wneg32(lre) : lre, a2 = lim < 0 ? wneg32(lim) : lim;
        const bool byre = a1 > a2, pos = (byre ? lre : lim) > 0;
        M[s] = pos ? (byre ? lre : lim) : wneg32(byre ? lre : lim);
        V[s] = base | (byre ? (pos ? 0x00u : 0x40u) : (pos ? 0xC0u : 0x80u));
    }
    const bool a = M[0] > M[1];
    mm = a ? M[0] : M[1]; vv = a ? V[0] : V[1];
    const bool b = M[2] > M[3];
    const int m2 = b ? M[2] : M[3]; const uint32_t v2 = b ? V[2] : V[3];
    if (m2 > mm) { mm = m2; vv = v2; }
}
// TCCK11Decoder::CCK11_DECODER (cck.hpp:255-763) on 8 chips: phi2 = 0 and pi/2, then the one of 3 pi/2 (m1 > m2) and pi; the two DQPSK bits and the odd symbol's
// rotation are the caller's
__device__ __forceinline__ uint32_t b11_cck11_bits(const cpx P[8])
{
    cpx A[4]; int m1, m2, m34; uint32_t v1, v2, v34;
    b11_cck_partial(P, 0, A); b11_cck11_module(A, m1, v1);
    b11_cck_partial(P, 3, A); b11_cck11_module(A, m2, v2); v2 |= 0x08u;        // m = 1: r = j^3
    const bool first = m1 > m2;
    b11_cck_partial(P, first ? 1 : 2, A); b11_cck11_module(A, m34, v34);        // m = 3: r = j, m = 2: r = j^2
    v34 |= first ? 0x0Cu : 0x04u;
    const int mb = first ? m1 : m2; const uint32_t vb = first ? v1 : v2;
    return mb > m34 ? vb : v34;
}
// one half byte of TCCK5P5Decoder (cck.hpp:70-206): phi2 = pi/2 against 3 pi/2; the imaginary part of B0 is negated BEFORE the shift
__device__ __forceinline__ int b11_cck5_metric(const cpx P[8], int k, bool& neg)
{
    cpx A[4]; b11_cck_partial(P, k, A);
    cpx b0 = b11_add32(A[0], A[1]), b1 = b11_add32(A[2], A[3]);
    b0.im = wneg32(b0.im);
    b0 = sra(b0, 2); b1 = sra(b1, 2);
    const int lre = wsub32(wmul32(b0.re, b1.re), wmul32(b0.im, b1.im));
    neg = !(lre > 0);
    return lre > 0 ? lre : wneg32(lre);
}
__device__ __forceinline__ uint32_t b11_cck5_nibble(const cpx P[8])
{
    bool n1, n2;
    const int max1 = b11_cck5_metric(P, 3, n1), max2 = b11_cck5_metric(P, 1, n2);   // m = 1: r = j^3, m = 3: r = j
    return max1 > max2 ? (n1 ? 0x08u : 0x00u) : (n2 ? 0x0Cu : 0x04u);
}

// ---- TDesc741 (scramble.hpp:93-170): out bit k = b[k] ^ b[k-4] ^ b[k-7] over the bit stream; s = the previous byte's (or the register's) 7 bits | b << 7
__device__ __forceinline__ uint32_t b11_desc741(uint32_t reg7, uint32_t b)
{
    const uint32_t s = (reg7 & 0x7Fu) | (b << 7);
    return ((s >> 7) ^ (s >> 3) ^ s) & 0xFFu;
}

// CalcCRC16 (core/inc/CRC16.h): reflected 0x8408, init 0xFFFF, ~
__device__ __forceinline__ uint32_t b11_crc16(const uint32_t h[4])
{
    uint32_t c = 0xFFFFu;
    for (int i = 0; i < 4; i++) {
        c ^= h[i];
        for (int k = 0; k < 8; k++) c = (c & 1u) ? (c >> 1) ^ 0x8408u : c >> 1;
    }
    return ~c & 0xFFFFu;
}

}  // namespace sora
