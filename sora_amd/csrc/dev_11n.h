// dev_11n.h -- the reference's 802.11n receive bricks, each stated once, for the three forms that run them:
//   the stage entry points sora_hip_*11n (k_11n.hip), the whole-path chain k_scan11n / k_scan11n_stream / k_scan_ht40 -> k_frame11n -> k_finish11n
//   (k_rx11n.hip), and the 40 MHz data field k_ht40_frame / k_ht40_finish (k_ht40.hip).
// A piece works on values: one carrier's, sample's or frame's worth of registers in and out.  A form keeps its schedule, its lane layout, its LDS
// structs, its prefetching and its hand-offs (DESIGN.md section 7, f1a has the piece x form table).  Reference locations are cited at each piece.
//   tables            kRuns / fill_demap_luts (dsp_demap.h), kHtLtf, kLLtfPlus, data_bin
//   MCS geometry      nbpsc11n, code_rate11n, data_bits11n, ht40_ndbps
//   TFreqEstimator    cfo_est11n (over dsp_atan32)            TFreqComp_11n       freq_comp11n
//   TSisoChannelEst   siso_est_carrier (over siso_one)        TSisoChannelComp + TMrcCombine   siso_comp_mrc
//   T11nSigDemap      sig_demap_soft, sig_deint_index         T11nViterbiSig      viterbi_sig_wave
//   T11nSigParser     sig_parse_front (what stands in front of each form's own gate)
//   TMimoChannelEst   mimo_h_carrier, mimo_inverse, mimo_weight_pack, mimo_est_carrier          TMimoChannelComp   mimo_comp_row
//   TPilotTrack_11n   dsp_atan16                              T11nDemap*          demap11n_store
//   T11nDeinterleave  deint11n_index                          T11aDesc + TBB11aFrameSink   finish_frame = desc11a_phase / desc11a_byte + fcs_verdict
#pragma once
#include "dev_arith.h"
#include "rx_types.h"

namespace sora {
// ---- MCS 8..14 (two streams) -> N_BPSC (rate_selector, fb11ndemod_config.hpp:136-147), code rate (0 / 1 / 2 = 1/2, 2/3, 3/4) and the data bits that
// `coded` coded bits carry (every count this is applied to divides: 104 and 108 N_BPSC per symbol, the decoder's 312-value bursts)
__host__ __device__ inline uint32_t nbpsc11n(uint32_t mcs) { return mcs == 8 ? 1u : mcs <= 10 ? 2u : mcs <= 12 ? 4u : 6u; }
__host__ __device__ inline uint32_t code_rate11n(uint32_t mcs) { return (mcs == 10 || mcs == 12 || mcs == 14) ? 2u : mcs == 13 ? 1u : 0u; }
__host__ __device__ inline uint32_t data_bits11n(uint32_t coded, uint32_t cr) { return cr == 0 ? coded / 2 : cr == 1 ? coded / 3 * 2 : coded / 4 * 3; }
// per stream, 108 data carriers; rate 5/6 (SORA_CR_56 = 3, the 40 MHz pair only): 90 N_BPSC
__host__ __device__ inline uint32_t ht40_ndbps(uint32_t nb, uint32_t cr) { return cr == 3 ? 90u * nb : data_bits11n(108u * nb, cr); }
// the 40 MHz pair's rate table: MCS 15 is 64-QAM, rate 5/6 (a front end whose gate is 14 never asks)
__host__ __device__ inline uint32_t code_rate_ht40(uint32_t mcs) { return mcs == 15 ? 3u : code_rate11n(mcs); }
namespace {
struct Run { uint8_t v, n; };
static __constant__ Run kRuns[83] = {
    {0,97},{1,10},{2,10},{3,11},{4,11},{5,10},{6,10},{7,97},                                                              // [0,8)   BPSK / QPSK
    {0,113},{1,7},{2,4},{3,4},{4,5},{5,4},{6,7},{7,112},                                                                   // [8,16)  16-QAM bit 0
    {0,58},{1,3},{2,2},{3,2},{4,2},{5,3},{6,3},{7,111},{6,3},{5,3},{4,2},{3,2},{2,2},{1,3},{0,57},                         // [16,31) 16-QAM bit 1
    {0,122},{1,3},{2,2},{3,1},{4,2},{5,2},{6,3},{7,121},                                                                   // [31,39) 64-QAM bit 0
    {0,52},{1,3},{2,2},{3,2},{4,1},{5,2},{6,3},{7,127},{6,3},{5,2},{4,1},{3,2},{2,2},{1,3},{0,51},                         // [39,54) 64-QAM bit 1
    {0,18},{1,2},{2,2},{3,2},{4,2},{5,1},{6,3},{7,57},{6,3},{5,2},{4,2},{3,1},{2,2},{1,3},{0,57},
    {1,3},{2,2},{3,1},{4,2},{5,2},{6,3},{7,57},{6,3},{5,1},{4,2},{3,2},{2,2},{1,2},{0,17} };                               // [54,83) 64-QAM bit 2
static __constant__ int kRunFirst[7] = { 0, 8, 16, 31, 39, 54, 83 };

__device__ __forceinline__ int data_bin(int l)               // carrier walk of the 11n demappers: -28..-1 then 1..28, pilots at +-7, +-21 skipped
{
    if (l < 26) return l < 7 ? 36 + l : (l < 20 ? 37 + l : 38 + l);
    const int m = l - 26;
    return m < 6 ? 1 + m : (m < 19 ? 2 + m : 3 + m);
}

__device__ __forceinline__ void fill_demap_luts(uint8_t (*lut)[256])      // the six step tables of dsp_demap.h, index v + 128; blockDim.x == 256
{
    const int t = threadIdx.x;
    for (int w = 0; w < 6; w++) {
        int acc = 0; uint8_t val = 0;
        for (int r = kRunFirst[w]; r < kRunFirst[w + 1]; r++) { if (t >= acc && t < acc + kRuns[r].n) val = kRuns[r].v; acc += kRuns[r].n; }
        lut[w][t] = val;
    }
}

// T11nDemap{BPSK,QPSK,QAM16,QAM64} (demapper11n.hpp:89-309): the equalised carrier limited to +-128 (demap_limit), the I bits then the Q bits out of the
// step tables of the modulation
__device__ __forceinline__ void demap11n_store(uint8_t* o, const uint8_t (*lut)[256], cpx x, int nb)
{
    const int re = min(max(x.re, -128), 127) + 128, im = min(max(x.im, -128), 127) + 128;
    switch (nb) {
    case 1: o[0] = lut[0][re]; break;
    case 2: o[0] = lut[0][re]; o[1] = lut[0][im]; break;
    case 4: o[0] = lut[1][re]; o[1] = lut[2][re]; o[2] = lut[1][im]; o[3] = lut[2][im]; break;
    default: o[0] = lut[3][re]; o[1] = lut[4][re]; o[2] = lut[5][re]; o[3] = lut[3][im]; o[4] = lut[4][im]; o[5] = lut[5][im];
    }
}
// T11nSigDemap (demapper11n.hpp:6-87): L-SIG (symbol 0) on I, HT-SIG 1 / 2 on Q, table 0; its carrier k of 48 sits at bin carrier_bin48(k).  The BPSK
// de-interleaver behind it (T11aDeinterleaveBPSK): de-interleaved position k of a symbol comes from position sig_deint_index(k)
__device__ __forceinline__ uint8_t sig_demap_soft(cpx v, int s3, const uint8_t (*lut)[256]) { return lut[0][min(max(s3 == 0 ? v.re : v.im, -128), 127) + 128]; }
__device__ __forceinline__ int sig_deint_index(int k) { return 3 * (k & 15) + (k >> 4); }

static __constant__ int8_t kHtLtf[57] = {   // HT-LTF, carriers -28..28 (IEEE 802.11n, 20 MHz)
    1, 1, 1, 1, -1, -1, 1, 1, -1, 1, -1, 1, 1, 1, 1, 1, 1, -1, -1, 1, 1, -1, 1, -1, 1, 1, 1, 1, 0,
    1, -1, -1, 1, 1, -1, 1, -1, 1, -1, -1, -1, -1, -1, 1, 1, -1, -1, 1, -1, 1, -1, 1, 1, 1, 1, -1, -1 };
struct cf { float re, im; };
// vcf mul (vector128.h:1107-1116): every product and every sum rounded on its own -- no fused multiply-add
// (the default -ffp-contract=fast-honor-pragmas would fuse a*b - c*d into an fma: one rounding less than the reference's
//  mulps / addsubps.  The pragma keeps every operation on its own; plain operators are IEEE single precision on gfx950.)
__device__ __forceinline__ cf cf_mul(cf a, cf b)
{
#pragma clang fp contract(off)
    cf r; r.re = (a.re * b.re) - (a.im * b.im); r.im = (a.im * b.re) + (a.re * b.im); return r;
}
__device__ __forceinline__ int cvtps_sat16(float x)    // cvtps2dq (nearest even; 0x80000000 when out of range or NaN), then packssdw
{
    const int v = (x >= -2147483648.0f && x < 2147483648.0f) ? (int)rintf(x) : (int)0x80000000;
    return sat16(v);
}
// TMimoChannelEst (channel_11n.hpp:329-443).  p_r / q_r: the carrier of HT-LTF 1 / 2 on RX chain r; negate: the carrier's HT-LTF value is not +1
// (_80211n_HTLTFMask; the caller's table: 20 and 40 MHz differ).  h[r][0] / h[r][1]: the P-matrix combination (p - q) / 2, (p + q) / 2
__device__ __forceinline__ void mimo_h_carrier(cpx p0, cpx q0, cpx p1, cpx q1, bool negate, cpx (&h)[2][2])
{
#pragma unroll
    for (int r = 0; r < 2; r++) {
        const cpx p = r ? p1 : p0, q = r ? q1 : q0;
        cpx d = sra(csubs(p, q), 1), s = sra(cadds(p, q), 1);
        if (negate) { d = mk(neg16(d.re), neg16(d.im)); s = mk(neg16(s.re), neg16(s.im)); }
        h[r][0] = d; h[r][1] = s;
    }
}
// ... its 2x2 inverse x 2^16 in single precision, operation for operation as brick/inc/sora_matrix.h:134-148,305-313: w[2 i + j] = entry (i, j); and a weight's
// way into COMPLEX16 (cvtps2dq, packssdw)
__device__ __forceinline__ uint32_t mimo_weight_pack(cf w) { return pack(mk(cvtps_sat16(w.re), cvtps_sat16(w.im))); }
__device__ __forceinline__ void mimo_inverse(const cpx (&h)[2][2], cf (&w)[4])
{
#pragma clang fp contract(off)
    const cf a00 = { (float)h[0][0].re, (float)h[0][0].im }, a01 = { (float)h[0][1].re, (float)h[0][1].im };
    const cf a10 = { (float)h[1][0].re, (float)h[1][0].im }, a11 = { (float)h[1][1].re, (float)h[1][1].im };
    const cf ad = cf_mul(a00, a11), bc = cf_mul(a01, a10);
    const cf det = { ad.re - bc.re, ad.im - bc.im };
    const float n = ((det.re * det.re) + (det.im * det.im)) / 65536.0f;
    const cf ds = { det.re, -det.im }, m01 = { -a01.re, -a01.im }, m10 = { -a10.re, -a10.im };
    const cf r00 = cf_mul(a11, ds), r01 = cf_mul(m01, ds), r10 = cf_mul(m10, ds), r11 = cf_mul(a00, ds);
    w[0] = { r00.re / n, r00.im / n }; w[1] = { r01.re / n, r01.im / n }; w[2] = { r10.re / n, r10.im / n }; w[3] = { r11.re / n, r11.im / n };
}
__device__ __forceinline__ void mimo_est_carrier(cpx p0, cpx q0, cpx p1, cpx q1, bool negate, cpx (&h)[2][2], uint32_t (&hinv)[4])
{
    mimo_h_carrier(p0, q0, p1, q1, negate, h);
    cf w[4]; mimo_inverse(h, w);
#pragma unroll
    for (int m = 0; m < 4; m++) hinv[m] = mimo_weight_pack(w[m]);
}
// TMimoChannelComp (channel_11n.hpp:445-521): one row of x = sat((W y) >> 9), the two products summed wrapping; a, b = the carrier on RX chain 0 / 1
__device__ __forceinline__ cpx mimo_comp_row(cpx w0, cpx w1, cpx a, cpx b)
{
    int ar, ai, br, bi;
    mul32(w0, a, ar, ai); mul32(w1, b, br, bi);
    return mk(sat16((int)((unsigned)ar + (unsigned)br) >> 9), sat16((int)((unsigned)ai + (unsigned)bi) >> 9));
}
// TFreqComp_11n (freqoffset_11n.hpp:162-280): the sample times the dsp_math sincos entry of its running phase, sat(>> 15)
__device__ __forceinline__ cpx freq_comp11n(cpx x, cpx cof)
{
    int re, im; mul32(x, cof, re, im);
    return mk(sat16(re >> 15), sat16(im >> 15));
}
// TSisoChannelComp (channel_11n.hpp:233-297) + TMrcCombine (PHY_11n.hpp:362-398): x_r = sat((y_r c_r) >> 9), mrc = (x_0 + x_1) >> 1 in wrapping int16
__device__ __forceinline__ cpx siso_comp_mrc(cpx y0, cpx c0, cpx y1, cpx c1, cpx& x0, cpx& x1)
{
    int re, im;
    mul32(y0, c0, re, im); x0 = mk(sat16(re >> 9), sat16(im >> 9));
    mul32(y1, c1, re, im); x1 = mk(sat16(re >> 9), sat16(im >> 9));
    return mk((short)((short)(x0.re + x1.re) >> 1), (short)((short)(x0.im + x1.im) >> 1));
}

static __constant__ unsigned long long kLLtfPlus = 0xF59FACC007A982B2ull;     // bit i: the L-LTF is +1 on FFT bin i (_80211_LLTFMask 0xFFFF0000 lanes)
__device__ __forceinline__ int sqn_wrap(cpx v) { return (int)((unsigned)(v.re * v.re) + (unsigned)(v.im * v.im)); }
__device__ __forceinline__ cpx siso_one(const uint32_t* x4, int j, int bin)
{
    const cpx x = unpack(x4[j]), xr = unpack(x4[(2 * j) & 3]), xi = unpack(x4[(2 * j + 1) & 3]);
    int sq = sqn_wrap(x);                                                  // pmaddwd: (-32768, -32768) wraps to INT_MIN
    if (sq == 0) sq = 1;
    const int hr = sqn_wrap(xr) >> 1, hi = sqn_wrap(xi) >> 1;
    const int re = (int)(((unsigned)x.re << 16) + (unsigned)hr) / sq, im = (int)(((unsigned)x.im << 16) + (unsigned)hi) / sq;
    cpx c = mk(sat16(re), sat16(im));
    if ((kLLtfPlus >> bin) & 1) c.im = (short)-c.im; else c.re = (short)-c.re;
    return c;
}
// TSisoChannelEst (channel_11n.hpp:33-231), bin i of one RX chain; y = the chain's two L-LTF symbols in the frequency domain, 64 bins each: zero in the
// guard band, else the wrapping average of the two symbols' estimates.  The rounding term is added lane for lane as the reference's vectors line up:
// component c of carrier j of a group of four gets |x[(2j + c) mod 4]|^2 >> 1 (siso_one)
__device__ __forceinline__ uint32_t siso_est_carrier(const uint32_t* y, int i)
{
    if (!(i < 28 || i >= 36)) return 0u;
    const uint32_t* l = y + (i & ~3);
    const cpx a = siso_one(l, i & 3, i), b = siso_one(l + 64, i & 3, i);
    return pack(mk((short)((short)(a.re + b.re) >> 1), (short)((short)(a.im + b.im) >> 1)));
}

// T11nSigParser (PHY_11n.hpp:432-513), the part in front of the gate: the L-SIG's reserved bits, parity, rate code (ieee80211a_cmn.h:97-107) and length, the
// HT-SIG's CRC-8 and its fields.  A check that fails leaves what was extracted before it and ok = false; which MCS, bandwidth and HT length a form takes is
// the caller's gate.  lsig: the 24 decoded L-SIG bits, ht: the 48 of HT-SIG 1 / 2
struct SigFront { bool ok; uint32_t rate_kbps, lsig_len, mcs, cbw40, ht_len; };
__device__ __forceinline__ SigFront sig_parse_front(uint32_t lsig, uint64_t ht)
{
    SigFront P = { false, 0u, 0u, 0u, 0u, 0u };
    const uint32_t sig = lsig & 0xFFFFFF;
    if ((sig & 0xFC0010) || (__popc(sig) & 1)) return P;
    const uint32_t code = sig & 0xF;
    if (code < 8) return P;
    P.rate_kbps = code == 0x8 ? 48000u : code == 0x9 ? 24000u : code == 0xA ? 12000u : code == 0xB ? 6000u : code == 0xC ? 54000u
                : code == 0xD ? 36000u : code == 0xE ? 18000u : 9000u;
    P.lsig_len = ((sig >> 5) & 0xFFF) * 2;
    if (P.lsig_len > 1500) return P;
    uint32_t crc = 0xFF;                                                     // CalcCRC8(ip, 4, 2): reflected, polynomial 0xE0, over HT-SIG bits 0..33
    for (int b = 0; b < 34; b++) { crc ^= (uint32_t)(ht >> b) & 1; crc = (crc & 1) ? (crc >> 1) ^ 0xE0 : crc >> 1; }
    if (((~crc) & 0xFF) != (uint32_t)((ht >> 34) & 0x3FFF)) return P;       // compared in int: bits 42.. (always 0 after the >> 6) included
    P.mcs = (uint32_t)ht & 0x7F; P.cbw40 = (uint32_t)(ht >> 7) & 1; P.ht_len = (uint32_t)(ht >> 8) & 0xFFFF;
    P.ok = true;
    return P;
}

template <int NB>
__device__ __forceinline__ uint64_t viterbi_sig_wave(const uint8_t* soft, uint64_t* dec, int lane)     // soft[2 * NB] de-interleaved, dec[NB + 1] in LDS
{
    const int n = lane, r0 = n, r1 = 64 | n;
    const int cA0 = __popc(r0 & 0155) & 1, cB0 = __popc(r0 & 0117) & 1, cA1 = __popc(r1 & 0155) & 1, cB1 = __popc(r1 & 0117) & 1;
    unsigned m = (n == 0) ? 0u : 0x30u;
    if (lane == 0) dec[0] = 0;
#pragma unroll 8
    for (int t = 1; t <= NB; t++) {
        const int va = soft[2 * (t - 1)], vb = soft[2 * (t - 1) + 1];
        const unsigned m0 = (unsigned)__shfl((int)m, n >> 1), m1 = (unsigned)__shfl((int)m, 32 + (n >> 1));
        const unsigned b0 = (cA0 ? 2 * (7 - va) : 2 * va) + (cB0 ? 2 * (7 - vb) : 2 * vb);
        const unsigned b1 = (cA1 ? 2 * (7 - va) : 2 * va) + (cB1 ? 2 * (7 - vb) : 2 * vb);
        const unsigned c0 = (m0 + b0) & 0xFE, c1 = ((m1 + b1) & 0xFF) | 1;
        m = min(c0, c1);
        { const uint64_t d = __ballot(m & 1); if (lane == 0) dec[t] = d; }
        if ((t & 7) == 0) {
            unsigned mn = m;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) mn = min(mn, (unsigned)__shfl_xor((int)mn, o));
            m = (m - (mn & 0xFE)) & 0xFF;
        }
    }
    unsigned kmin = (m << 8) | ((unsigned)n << 2);                           // smallest metric, then smallest state (INDEXES, hmin)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) kmin = min(kmin, (unsigned)__shfl_xor((int)kmin, o));
    int pos = (int)((kmin >> 2) & 0x3F) | (int)(((kmin >> 8) & 1) << 6);
    __builtin_amdgcn_s_waitcnt(0); __builtin_amdgcn_wave_barrier();
    uint64_t out = 0;
    for (int b = 0; b < NB; b++) {                                           // bit b of the walk is output bit NB - 1 - b
        out |= (uint64_t)((pos >> 6) & 1) << (NB - 1 - b);
        pos = (pos >> 1) & 0x3F;
        pos |= (int)((dec[NB - 1 - b] >> pos) & 1) << 6;
    }
    return out;
}

__device__ __forceinline__ int atan_tail(const short* tab, int idx, int tsign, int sign)
{
    if (idx < 0 || idx >= 4097) return 0;
    int srad = tab[idx];
    srad = (int)(short)((16384 & tsign) + ((srad ^ tsign) - tsign));
    srad ^= sign; return (int)(short)(srad - sign);
}
__device__ __forceinline__ int dsp_atan16(const short* tab, int x, int y)      // dsp_math::atan(short, short); x, y already int16 values
{
    const int sign = (x ^ y) >> 15;                                            // -1 / 0
    const int absx = (int)(short)((x ^ (x >> 15)) - (x >> 15)), absy = (int)(short)((y ^ (y >> 15)) - (y >> 15));
    const int tsign = (int)(short)((absx - absy) >> 15);
    const int tsum = absx + absy, d = absx - absy;
    const int tmax = (tsum + ((d ^ (d >> 31)) - (d >> 31))) >> 1, tmin = tsum - tmax;
    if (tmax == 0) return 0;
    int idx;
    if (tmin >= 0 && tmin <= tmax && tmax < 32768) {
        // The usual case (everything but an input of -32768): numerator < 2^31 + 2^14, divisor < 2^15, quotient <= 65536.  One reciprocal and a
        // correction in each direction instead of the 30-instruction integer division: the float estimate is off by less than 0.02.
        const unsigned num = ((unsigned)tmin << 16) + ((unsigned)tmax >> 1);
        unsigned q = (unsigned)((float)num * __builtin_amdgcn_rcpf((float)tmax));
        int r = (int)(num - __umul24(q, (unsigned)tmax));
        if (r < 0) { q--; r += tmax; }
        if (r >= tmax) q++;
        idx = (int)q;
    } else idx = (int)(((unsigned)tmin << 16) + (unsigned)(tmax >> 1)) / tmax;
    return atan_tail(tab, idx >> 4, tsign, sign);
}
// dsp_math::atan(int, int).  The reference's imax() forms 2 max(|x|, |y|) in int, which overflows from 2^30 on; its compiled code forms that sum 64 bits
// wide (it only feeds the __int64 division), so tmax / tmin are the exact larger / smaller magnitude.  An L-LTF near the int16 rails gets there: the 128
// products >> 7 of TFreqEstimator_11n add up to 2 |x|^2.  x = INT_MIN: 0 at y = 0 and y = INT_MIN as measured on the compiled reference (oracle/so_11n.c).
__device__ __forceinline__ int dsp_atan32(const short* tab, int x, int y)
{
    if (x == (int)0x80000000 && (y == 0 || y == (int)0x80000000)) return 0;
    const int sign = (int)(short)(((x ^ y) >> 31) & 0xFFFF);
    const int absx = (int)(((unsigned)x ^ (unsigned)(x >> 31)) - (unsigned)(x >> 31)), absy = (int)(((unsigned)y ^ (unsigned)(y >> 31)) - (unsigned)(y >> 31));
    const int tsign = (int)(short)(((int)((unsigned)absx - (unsigned)absy) >> 31) & 0xFFFF);
    const long long tsum = (long long)absx + absy, d = (long long)absx - absy;
    const long long tmax = (tsum + (d < 0 ? -d : d)) >> 1, tmin = tsum - tmax;
    const long long i64y = tmax == 0 ? 1 : tmax;
    const int idx = (int)((tmin * 65536 + (i64y >> 1)) / i64y);
    return atan_tail(tab, idx >> 4, tsign, sign);
}
// TFreqEstimator_11n (freqoffset_11n.hpp:42-160): lane = sample n of the first L-LTF half; a_r / b_r = samples n / n + 64 on RX chain r.  Per lane the two
// conjugate products >> 7, summed over the wave (wrapping 32-bit sums: order does not matter), then the phase step per sample, in every lane
__device__ __forceinline__ int cfo_est11n(const short* atan_tab, cpx a0, cpx b0, cpx a1, cpx b1)
{
    int re, im, sre, sim;
    conj_mul32(a0, b0, re, im); sre = re >> 7; sim = im >> 7;
    conj_mul32(a1, b1, re, im); sre += re >> 7; sim += im >> 7;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { sre += __shfl_xor(sre, d); sim += __shfl_xor(sim, d); }
    return dsp_atan32(atan_tab, sre, sim) >> 6;
}

// T11aDesc + TBB11aFrameSink (scramble.hpp:319-349, PHY_11a.hpp:660-692) on a decoded frame, one wave: dec = the decoder's bytes (SERVICE field first), L = the
// PSDU length.  Descrambles by the phase table into `bytes` (the wave's LDS buffer, >= L bytes) and the MPDU slot `mp`, runs the parallel CRC-32 and
// returns the verdict; fcs = the frame's last four bytes.  Both are lane 0's to store (crc32_wave leaves the register there).  One pass of crc32_wave covers the
// last 64 x 40 = 2560 bytes: enough for the 802.11n handle (LENGTH <= 1500).  LONG (the 40 MHz handle, LENGTH <= 4000): a longer PSDU takes a second pass over the
// 2560 bytes in front of those, joined through Z_2560 as dev_tx.h joins the transmitter's two FCS waves.
// The two halves, which are also the stages sora_hip_desc11a and sora_hip_frame_sink11a (k_11n.hip):
//   desc11a_phase / desc11a_byte   T11aDesc: byte 0 of the decoder's output is dropped, byte 1 >> 1 seeds the register; descrambled byte i is decoded byte 2 + i
//                                  xor the scrambler's byte 8 i cycle positions behind the seed's (seed 0: the register stays 0)
//   fcs_verdict                    TBB11aFrameSink on L descrambled bytes (in LDS, L >= 4 for the brick to decide): the CRC-32 over the first L - 4 against the last four
__device__ __forceinline__ unsigned desc11a_phase(const Tables& T, const uint8_t* dec) { return T.scr_phase[(dec[1] >> 1) & 0x7F]; }
__device__ __forceinline__ unsigned desc11a_byte(const Tables& T, unsigned phase, const uint8_t* dec, uint32_t i)
{
    const unsigned sb = phase == 255 ? 0u : T.scr_seq[(phase + 8u * i) % 127u];
    return dec[2 + i] ^ sb;
}
template <bool LONG>
__device__ __forceinline__ uint32_t fcs_verdict(const uint8_t* bytes, uint32_t L, const uint32_t* s_crc, const uint32_t* s_z, int lane, uint32_t& fcs);

template <bool LONG = false>
__device__ __forceinline__ uint32_t finish_frame(const Tables& T, const uint8_t* dec, uint32_t L, uint8_t* bytes, uint8_t* mp, const uint32_t* s_crc,
                                                 const uint32_t* s_z, int lane, uint32_t& fcs)
{
    const unsigned phase = desc11a_phase(T, dec);
    for (uint32_t i = lane; i < L; i += 64) {
        const unsigned o = desc11a_byte(T, phase, dec, i);
        bytes[i] = (uint8_t)o; mp[i] = (uint8_t)o;
    }
    wave_lds_sync();
    return fcs_verdict<LONG>(bytes, L, s_crc, s_z, lane, fcs);
}
template <bool LONG>
__device__ __forceinline__ uint32_t fcs_verdict(const uint8_t* bytes, uint32_t L, const uint32_t* s_crc, const uint32_t* s_z, int lane, uint32_t& fcs)
{
    const int n = L >= 4 ? (int)L - 4 : 0;
    uint32_t crc;
    if (n >= 4) {
        crc = crc32_wave(bytes, n, s_crc, s_z, lane);
        if constexpr (LONG) {
            if (n > 64 * 40) crc ^= crc_zeros(s_z, 5, crc_zeros(s_z, 5, crc32_wave(bytes, n, s_crc, s_z, lane + 64)));
        }
    }
    else { crc = 0xFFFFFFFFu; for (int i = 0; i < n; i++) crc = (crc >> 8) ^ s_crc[(bytes[i] ^ crc) & 0xFF]; }
    fcs = 0;
    if (L >= 4) fcs = (uint32_t)bytes[L - 4] | ((uint32_t)bytes[L - 3] << 8) | ((uint32_t)bytes[L - 2] << 16) | ((uint32_t)bytes[L - 1] << 24);
    return ((~crc) == fcs) ? E_FRAME_OK : E_CRC32_FAIL;
}

// T11nDeinterleave*_S{0,1} (deinterleaver_11n.hpp): source position of de-interleaved position k -- the HT interleaver (N_COL 13,
// N_ROW 4 N_BPSC, N_ROT 11) inverted
__device__ __forceinline__ int deint11n_index(int nb, int iss, int k)
{
    const int s = nb / 2 > 1 ? nb / 2 : 1, nrow = 4 * nb, np = 52 * nb;
    const int i = nrow * (k % 13) + k / 13;
    int j = s * (i / s) + (i + np - (13 * i) / np) % s;
    if (iss > 0) j = ((j - ((iss * 2) % 3 + 3 * (iss / 3)) * 11 * nb) % np + np) % np;
    return j;
}
}  // namespace
}  // namespace sora
