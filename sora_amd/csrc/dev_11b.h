// dev_11b.h -- the arithmetic of the 802.11b receive graph's bricks (CreateDemodGraph, kernel/bb/demod11/fb11bdemod_config.hpp:122-172) as device functions, one brick
// step each, for both forms of the graph: the stage kernels of k_11b.hip and the handle's whole-capture kernels of k_rx11b.hip (call by call and in bulk_pass).  Every
// sum wraps where the brick's SSE operator wraps: int16 through w16, int32 through unsigned arithmetic.  tests/cxx/rx11b_stage_model.c is the same text in C.
// The handle keeps all of a capture's state in scalar registers, and its form decides the form of a piece with state: no "store to one of two variables" and no
// pointer select (the note on code shape in k_rx11b.hip).  b11_timing_carry is selects throughout; b11_barker_peak is the handle's switch, whose branches are scalar
// and write each variable under a condition of its own.  The stage kernels' lane-0 loops take the same text.
#pragma once
#include "dev_arith.h"
#include "rx_types.h"

namespace sora {

enum { k11bRateSync = 0, k11bRate1M, k11bRate2M, k11bRate5p5M, k11bRate11M };
enum { k11bNoPeak = 0, k11bPeakFound, k11bPeakValid, k11bPeakValided, k11bBarkerSynced };
// the graph's other error codes (E_FRAME_OK, E_PLCP_HEADER_FAIL, E_CRC32_FAIL, E_CS_TIMEOUT: rx_types.h)
constexpr uint32_t E_NOT_SUPPORTED = 0x80000003u, E_SFD_FAIL = 0x80000004u, E_SFD_TIMEOUT = 0x80000008u, E_SYNC_TIMEOUT = 0x80000009u;

__device__ __forceinline__ int wadd32(int a, int b) { return (int)((unsigned)a + (unsigned)b); }
__device__ __forceinline__ int wsub32(int a, int b) { return (int)((unsigned)a - (unsigned)b); }
__device__ __forceinline__ int wneg32(int a) { return (int)(0u - (unsigned)a); }
__device__ __forceinline__ int wmul32(int a, int b) { return (int)((unsigned)a * (unsigned)b); }
__device__ __forceinline__ cpx cadd16(cpx a, cpx b) { return mk(w16(a.re + b.re), w16(a.im + b.im)); }
__device__ __forceinline__ cpx csub16(cpx a, cpx b) { return mk(w16(a.re - b.re), w16(a.im - b.im)); }

// ---- TSymTiming::AdjustTiming (symtiming.hpp:118-170): the early-late detector on the energies at the sampling phase (sm), the one before it (se) and the one behind
// it (sl).  di = the step of m_index, df = the step of m_frag; at most one of them is not 0.
struct B11Timing { int di, df; };
__device__ __forceinline__ B11Timing b11_adjust_timing(int sm, int se, int sl)
{
    const bool late_better = se < sl, a = sm < se, b = sm < sl;
    B11Timing t;
    t.di = late_better ? (a ? 1 : 0) : (b ? -1 : 0);
    t.df = late_better ? (!a && b ? 1 : 0) : (!b && a ? -1 : 0);
    return t;
}
// a decision as four bits (di + 1, df + 1: two bits each), for the kernels that work the decisions out ahead of the walk
__device__ __forceinline__ uint32_t b11_timing_code(B11Timing t) { return (uint32_t)((t.di + 1) | ((t.df + 1) << 2)); }
__device__ __forceinline__ B11Timing b11_timing_of(uint32_t code) { B11Timing t; t.di = (int)(code & 3u) - 1; t.df = (int)((code >> 2) & 3u) - 1; return t; }
// ... and what it does to (m_index, m_frag): an index step clears the fraction; a fraction that reaches +-4 carries into the index and comes out at -+3
__device__ __forceinline__ void b11_timing_carry(B11Timing t, int& m_index, int& m_frag)
{
    const int mf = t.di != 0 ? 0 : m_frag + t.df;
    const int carry = mf >= 4 ? 1 : (mf <= -4 ? -1 : 0);
    m_index += t.di + carry; m_frag = carry > 0 ? -3 : (carry < 0 ? 3 : mf);
}

// ---- TBarkerSync (symtiming.hpp:229-313).  UpdateBarkerCorrelation (:296-313): partial sum k becomes partial sum k + 1 plus or minus the chip >> 4 (bit k of
// kB11BarkerAdd: plus), the sum that falls out is the correlation.  ld(k) reads partial sum k, st(k, v) writes it: the caller's storage
constexpr uint32_t kB11BarkerAdd = 0x0DCu;
template <typename LD, typename ST>
__device__ __forceinline__ cpx b11_barker_shift(cpx ss, LD ld, ST st)
{
    const cpx o = csub16(ld(0), ss);
#pragma unroll
    for (int k = 0; k < 9; k++) st(k, (kB11BarkerAdd >> k) & 1u ? cadd16(ld(k + 1), ss) : csub16(ld(k + 1), ss));
    st(9, ss);
    return o;
}
// the peak search (:229-294) on one correlation value
__device__ __forceinline__ void b11_barker_peak(int corr, int& flag, int& peak, int& m_max)
{
    switch (flag) {
    case k11bNoPeak:
        if (corr > m_max) { m_max = corr; peak = 1; } else if (++peak == 11) flag = k11bPeakFound;
        break;
    case k11bPeakFound:
        m_max = corr / 2; peak = 1; flag = k11bPeakValid;
        break;
    case k11bPeakValid:
        if (corr > m_max) { m_max = corr; peak = 0; flag = k11bNoPeak; } else if (++peak == 11) flag = k11bPeakValided;
        break;
    default:
        flag = k11bBarkerSynced;                                                // "just skip one more symbol"
    }
}

// ---- TBB11bDespread::QuickBarkerDespread (barkerspread.hpp:277-303): what the chip at `place` (0..10) of the code adds to the symbol -- chips 1 and 4 are negated BEFORE
// the >> 4, chips 8-10 subtracted after it.  The symbol is the wrapping int16 sum of the eleven terms, in any order
__device__ __forceinline__ cpx b11_barker_term(cpx v, int place)
{
    const bool pre = place == 1 || place == 4;
    const cpx t = sra(mk(pre ? neg16(v.re) : v.re, pre ? neg16(v.im) : v.im), 4);
    return place >= 8 ? mk(-t.re, -t.im) : t;
}
// c = 11 packed chips at a stride of `stride` words
__device__ __forceinline__ uint32_t b11_despread(const uint32_t* c, int stride = 1)
{
    int re = 0, im = 0;
#pragma unroll
    for (int k = 0; k < 11; k++) { const cpx t = b11_barker_term(unpack(c[k * stride]), k); re += t.re; im += t.im; }
    return pack(mk(w16(re), w16(im)));
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

// ---- CCK (cck.hpp).  a * j^k; with k a constant the selects fold, with k per lane (the pruned search's third module, the handle's hypothesis per lane) they stay
// selects: no branch
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
// one correlation: the hypothesis phi2 = j^k, phi3 = j^s on 8 chips.  Bx = (A2 + q A1) >> 2, By = (A4 + q A3) >> 2 with q = j^s; L = conj(Bx) By (cck.hpp:268-303 and its
// three repetitions); l5 = the 5.5 Mbps decoder's real part, where the imaginary part of Bx is negated BEFORE the shift (cck.hpp:94-98)
struct B11Corr { int lre, lim, l5; };
__device__ __forceinline__ B11Corr b11_cck_corr(const cpx P[8], int k, int s)
{
    cpx A[4]; b11_cck_partial(P, k, A);
    const cpx bx0 = b11_add32(A[1], b11_rot(A[0], s)), bx = sra(bx0, 2), by = sra(b11_add32(A[3], b11_rot(A[2], s)), 2);
    B11Corr c;
    c.lre = wadd32(wmul32(bx.re, by.re), wmul32(bx.im, by.im));
    c.lim = wsub32(wmul32(bx.re, by.im), wmul32(bx.im, by.re));
    c.l5  = wsub32(wmul32(bx.re, by.re), wmul32(wneg32(bx0.im) >> 2, by.im));
    return c;
}
// what CCK11_DECODER makes of one correlation: the larger of |re|, |im| picks phi4 (strictly: a tie takes the imaginary part), its size is the metric; value bits
// 0x00, 0x30, 0x10, 0x20 for phi3 = 1, j, -1, -j
__device__ __forceinline__ void b11_cck11_leaf(B11Corr c, int s, int& M, uint32_t& V)
{
    const uint32_t base = s == 0 ? 0x00u : s == 1 ? 0x30u : s == 2 ? 0x10u : 0x20u;
    const int a1 = c.lre < 0 ? wneg32(c.lre) : c.lre, a2 = c.lim < 0 ? wneg32(c.lim) : c.lim;
    const bool byre = a1 > a2, pos = (byre ? c.lre : c.lim) > 0;
    M = pos ? (byre ? c.lre : c.lim) : wneg32(byre ? c.lre : c.lim);
    V = base | (byre ? (pos ? 0x00u : 0x40u) : (pos ? 0xC0u : 0x80u));
}
// one "Module" of CCK11_DECODER (e.g. cck.hpp:277-390): the four phi3 hypotheses of one phi2, then the reference's comparison tree with its strict comparisons
__device__ __forceinline__ void b11_cck11_module(const cpx P[8], int k, int& mm, uint32_t& vv)
{
    int M[4]; uint32_t V[4];
#pragma unroll
    for (int s = 0; s < 4; s++) b11_cck11_leaf(b11_cck_corr(P, k, s), s, M[s], V[s]);
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
    int m1, m2, m34; uint32_t v1, v2, v34;
    b11_cck11_module(P, 0, m1, v1);
    b11_cck11_module(P, 3, m2, v2); v2 |= 0x08u;                                // m = 1: r = j^3
    const bool first = m1 > m2;
    b11_cck11_module(P, first ? 1 : 2, m34, v34);                               // m = 3: r = j, m = 2: r = j^2
    v34 |= first ? 0x0Cu : 0x04u;
    const int mb = first ? m1 : m2; const uint32_t vb = first ? v1 : v2;
    return mb > m34 ? vb : v34;
}
// one half byte of TCCK5P5Decoder (cck.hpp:70-206) from its two correlations l1 (phi2 = pi/2) and l2 (3 pi/2), both with phi3 = 0
__device__ __forceinline__ uint32_t b11_cck5_pick(int l1, int l2)
{
    const int max1 = l1 > 0 ? l1 : wneg32(l1), max2 = l2 > 0 ? l2 : wneg32(l2);
    return max1 > max2 ? (l1 > 0 ? 0x00u : 0x08u) : (l2 > 0 ? 0x04u : 0x0Cu);
}
__device__ __forceinline__ uint32_t b11_cck5_nibble(const cpx P[8]) { return b11_cck5_pick(b11_cck_corr(P, 3, 0).l5, b11_cck_corr(P, 1, 0).l5); }   // m = 1: r = j^3, m = 3: r = j

// ---- TDesc741 (scramble.hpp:93-170): out bit k = b[k] ^ b[k-4] ^ b[k-7] over the bit stream.  bits = the stream from here on (bit 0 first) in a 32- or 64-bit
// word, reg7 = the seven bits in front of it; all but the top seven bits of the result stand
template <typename T>
__device__ __forceinline__ T b11_desc741_bits(uint32_t reg7, T bits)
{
    const T s = (T)(bits << 7) | (T)(reg7 & 0x7Fu);
    return (s >> 7) ^ (s >> 3) ^ s;
}
// one byte
__device__ __forceinline__ uint32_t b11_desc741(uint32_t reg7, uint32_t b) { return b11_desc741_bits(reg7, b) & 0xFFu; }

// CalcCRC16 (core/inc/CRC16.h): reflected 0x8408, init 0xFFFF, ~
__device__ __forceinline__ uint32_t b11_crc16(const uint32_t h[4])
{
    uint32_t c = 0xFFFFu;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        c ^= h[i];
#pragma unroll
        for (int k = 0; k < 8; k++) c = (c & 1u) ? (c >> 1) ^ 0x8408u : c >> 1;
    }
    return ~c & 0xFFFFu;
}
// ---- TBB11bPlcpParser (PHY_11b.hpp:560-640) behind a good CRC-16: SIGNAL, SERVICE (its length-extension bits) and LENGTH (microseconds) -> rate and bytes.  An
// unknown SIGNAL gives 0 kbps, 0 bytes and leaves the rate state at `rate`, the caller's
struct B11Plcp { uint32_t kbps, len; int rate; };
__device__ __forceinline__ B11Plcp b11_plcp_fields(uint32_t signal, uint32_t service, uint32_t length, int rate)
{
    const uint32_t ext = (service >> 7) + ((service >> 3) & 1u);
    B11Plcp p; p.kbps = 0; p.len = 0; p.rate = rate;
    switch (signal) {
    case 0x0A: p.kbps = 1000;  p.len = length >> 3; p.rate = k11bRate1M; break;
    case 0x14: p.kbps = 2000;  p.len = length >> 2; p.rate = k11bRate2M; break;
    case 0x37: p.kbps = 5500;  p.len = (((length * 11u) >> 4) - ext) & 0xFFFFu; p.rate = k11bRate5p5M; break;
    case 0x6E: p.kbps = 11000; p.len = (((length * 11u) >> 3) - ext) & 0xFFFFu; p.rate = k11bRate11M; break;
    default: break;
    }
    return p;
}

// ---- TBB11bFrameSink (PHY_11b.hpp:700-740), "speculating ACK": the verdict falls with three FCS bytes in hand.  crc = the register over the bytes in front of the FCS
__device__ __forceinline__ uint32_t b11_fcs_verdict(uint32_t crc, uint32_t fcs) { return (~crc & 0x00FFFFFFu) == (fcs & 0x00FFFFFFu) ? E_FRAME_OK : E_CRC32_FAIL; }

}  // namespace sora
