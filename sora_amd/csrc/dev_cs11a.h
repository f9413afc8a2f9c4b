// dev_cs11a.h -- the arithmetic of the 802.11a receive graph's front-end bricks as stages (k_11a.hip; fb11ademod_config.hpp:169-232): TDCRemoveEx<4>, TCCA11a and
// TDCEstimator -- one burst at a time over a state every lane holds alike (the events), a span of plain bursts position-parallel (the idle search) -- and T11aPLCPParser.
// k_scan.hip states the same constants for its fused passes and does not include this file.
#pragma once
#include "kernels.h"

namespace sora {

// sora_cca11a_state / sora_dcest11a_state / sora_cs11a_state as words (include/sora_hip.h)
constexpr int kCca11aWords = 44, kDcEst11aWords = 4, kCs11aWords = kCca11aWords + kDcEst11aWords;
constexpr uint32_t kCs11aMaxSense = 84;                     // TCCA11a::max_sense_count (cca.hpp:114)
constexpr uint32_t kCs11aDcInterval = 8;                    // TDCEstimator::dc_update_interval (dc.hpp:102)
constexpr uint32_t kCs11aTimeout = 0x80000007u;             // E_ERROR_CS_TIMEOUT
constexpr uint32_t kPlcpHeaderFail = 0x80000005u;           // E_ERROR_PLCP_HEADER_FAIL

// rep_sub / add on packed COMPLEX16 words: both halves wrap at 16 bits (_mm_sub_epi16 / _mm_add_epi16)
__device__ __forceinline__ uint32_t cs11a_sub16(uint32_t a, uint32_t b) { return ((a - b) & 0xFFFFu) | (((a >> 16) - (b >> 16)) << 16); }
__device__ __forceinline__ uint32_t cs11a_add16(uint32_t a, uint32_t b) { return ((a + b) & 0xFFFFu) | (((a >> 16) + (b >> 16)) << 16); }
// shift_right(vcs, n): arithmetic, half by half
__device__ __forceinline__ uint32_t cs11a_sra16(uint32_t a, int n) { return ((uint32_t)((int)(short)a >> n) & 0xFFFFu) | ((uint32_t)((int)a >> (16 + n)) << 16); }
__device__ __forceinline__ int cs11a_abs(int v) { return v < 0 ? (int)(0u - (unsigned)v) : v; }

// TDCEstimator's term of one burst (dc.hpp:137): hadd(shift_right(pi, 5)), wrapping at 16 bits, the same in all four elements
__device__ __forceinline__ uint32_t cs11a_dc_term(const uint32_t p[4])
{
    uint32_t h = 0;
#pragma unroll
    for (int e = 0; e < 4; e++) h = cs11a_add16(h, cs11a_sra16(p[e], 5));
    return h;
}

// CMovingWindow<int, 4> + CAccumulator (dspalg.hpp:5-98), oldest element first
struct Cs11aAcc { int w[4]; int reg; };
__device__ __forceinline__ void cs11a_push(Cs11aAcc& a, int d)
{
    a.reg = (int)((unsigned)a.reg + (unsigned)d - (unsigned)a.w[0]);
    a.w[0] = a.w[1]; a.w[1] = a.w[2]; a.w[2] = a.w[3]; a.w[3] = d;
}

// What TCCA11a keeps, the context fields it touches, and TDCEstimator's three words.  Every member is wave-uniform.
struct Cs11a {
    uint32_t cca_state, error_code, thr, reading, ctx_peak_index;
    uint32_t sync, auto_count, sense_count, high_count;
    int peak_corr; uint32_t peak_index;
    uint32_t his[16];                                       // sample_his: four bursts, oldest first, already >> 2
    Cs11aAcc ac_re, ac_im, energy;
    uint32_t update_cnt, sum_dc, dc;                        // TDCEstimator + CF_VecDC (one element: the four are equal)
};

__device__ __forceinline__ void cs11a_load(Cs11a& S, const uint32_t* st, bool with_dc)
{
    S.cca_state = st[0]; S.error_code = st[1]; S.thr = st[2]; S.reading = st[3]; S.ctx_peak_index = st[4];
    S.sync = st[5] & 1u; S.auto_count = st[6]; S.sense_count = st[7]; S.high_count = st[8]; S.peak_corr = (int)st[9]; S.peak_index = st[10] & 15u;
#pragma unroll
    for (int i = 0; i < 16; i++) S.his[i] = st[12 + i];
#pragma unroll
    for (int g = 0; g < 4; g++) { S.ac_re.w[g] = (int)st[28 + g]; S.ac_im.w[g] = (int)st[32 + g]; S.energy.w[g] = (int)st[36 + g]; }
    S.ac_re.reg = (int)st[40]; S.ac_im.reg = (int)st[41]; S.energy.reg = (int)st[42];
    S.update_cnt = with_dc ? st[kCca11aWords] : 0u; S.sum_dc = with_dc ? st[kCca11aWords + 1] : 0u; S.dc = with_dc ? st[kCca11aWords + 2] : 0u;
}
__device__ __forceinline__ void cs11a_store(const Cs11a& S, uint32_t* st, bool with_dc)      // cca_pwr_threshold (word 2) and the reserved words stand
{
    st[0] = S.cca_state; st[1] = S.error_code; st[3] = S.reading; st[4] = S.ctx_peak_index;
    st[5] = S.sync; st[6] = S.auto_count; st[7] = S.sense_count; st[8] = S.high_count; st[9] = (uint32_t)S.peak_corr; st[10] = S.peak_index;
#pragma unroll
    for (int i = 0; i < 16; i++) st[12 + i] = S.his[i];
#pragma unroll
    for (int g = 0; g < 4; g++) { st[28 + g] = (uint32_t)S.ac_re.w[g]; st[32 + g] = (uint32_t)S.ac_im.w[g]; st[36 + g] = (uint32_t)S.energy.w[g]; }
    st[40] = (uint32_t)S.ac_re.reg; st[41] = (uint32_t)S.ac_im.reg; st[42] = (uint32_t)S.energy.reg;
    if (with_dc) { st[kCca11aWords] = S.update_cnt; st[kCca11aWords + 1] = S.sum_dc; st[kCca11aWords + 2] = S.dc; }
}

// GetCrossCorrelation (cca.hpp:202-218) of the four bursts in sample_his with the pattern this lane holds (pat[16]: pattern lane & 15, packed).  Every sum wraps
// at 32 bits, so their order is free.
__device__ __forceinline__ int cs11a_cross(const uint32_t his[16], const uint32_t pat[16])
{
    unsigned r = 0, i = 0;
#pragma unroll
    for (int k = 0; k < 16; k++) {
        int re, im; conj_mul32(unpack(pat[k]), unpack(his[k]), re, im);
        r += (unsigned)re; i += (unsigned)im;
    }
    return (int)((unsigned)cs11a_abs((int)r) + (unsigned)cs11a_abs((int)i));
}
__device__ __forceinline__ int cs11a_lane(int v, uint32_t l) { return __builtin_amdgcn_readlane(v, uni((int)l)); }      // l wave-uniform

// One burst through TCCA11a::Process (cca.hpp:318-437) and, FUSED, the TDCRemoveEx in front of it and the TDCEstimator behind its gate: in[4] = the burst as it
// arrives (raw when FUSED, DC-removed otherwise), every word wave-uniform; pat = this lane's pattern.  -> true where the burst passes the gate (sync_state is
// no_energy behind it); raised = this burst changed error_code.
template <bool FUSED>
__device__ __forceinline__ bool cs11a_burst(Cs11a& S, const uint32_t in[4], const uint32_t pat[16], bool& raised)
{
    uint32_t pi[4], pii[4];
#pragma unroll
    for (int e = 0; e < 4; e++) { pi[e] = FUSED ? cs11a_sub16(in[e], S.dc) : in[e]; pii[e] = cs11a_sra16(pi[e], 2); }
    if (!S.sync) {
        unsigned sr = 0, si = 0, se = 0;
#pragma unroll
        for (int e = 0; e < 4; e++) {                         // GetAutoCorrelation (cca.hpp:165-186), GetEnergy (:188-193)
            int re, im; const cpx x = unpack(pii[e]);
            conj_mul32(x, unpack(S.his[e]), re, im);
            sr += (unsigned)(re >> 4); si += (unsigned)(im >> 4); se += (unsigned)(sqnorm(x) >> 4);
        }
        cs11a_push(S.ac_re, (int)sr); cs11a_push(S.ac_im, (int)si); cs11a_push(S.energy, (int)se);
        const int a = (int)((unsigned)cs11a_abs(S.ac_re.reg) + (unsigned)cs11a_abs(S.ac_im.reg)), en = S.energy.reg;
#pragma unroll
        for (int k = 0; k < 12; k++) S.his[k] = S.his[k + 4];
#pragma unroll
        for (int e = 0; e < 4; e++) S.his[12 + e] = pii[e];
        S.sense_count += 4;
        if (en > (int)S.thr && a >= en - (en >> 3)) {
            S.auto_count++; S.sense_count = 0;
            if (S.auto_count >= 4) {                          // establish_sync (cca.hpp:220-243): pattern i in lane i of every row
                const int corr = cs11a_cross(S.his, pat);
                int best = corr, at = (int)(threadIdx.x & 15u); unsigned sum = (unsigned)corr;
#pragma unroll
                for (int o = 8; o > 0; o >>= 1) {
                    const int c2 = __shfl_xor(best, o), a2 = __shfl_xor(at, o);
                    sum += (unsigned)__shfl_xor((int)sum, o);
                    if (c2 > best || (c2 == best && a2 < at)) { best = c2; at = a2; }
                }
                best = uni(best); at = uni(at); const int sum_corr = uni((int)sum);
                S.peak_corr = 0;
                if (best > 0) { S.peak_corr = best; S.peak_index = (uint32_t)at; }
                if (S.peak_corr > (sum_corr >> 3)) {
                    S.sync = 1; S.high_count = 0; S.reading = (uint32_t)en;
                    if (S.peak_index > 3) { S.high_count = S.peak_index / 4; S.peak_index &= 3u; }
                    S.ctx_peak_index = S.peak_index;
                }
            }
        } else S.auto_count = 0;
    } else {
#pragma unroll
        for (int k = 0; k < 12; k++) S.his[k] = S.his[k + 4];
#pragma unroll
        for (int e = 0; e < 4; e++) S.his[12 + e] = pii[e];
        S.high_count++;
        if (S.high_count % 4 == 0) {                          // check_sync (cca.hpp:245-265)
            const int corr = uni(cs11a_lane(cs11a_cross(S.his, pat), S.peak_index));
            if (corr < (S.peak_corr >> 1)) {
                if (S.high_count > 8) S.cca_state = 1;       // power_detected
                else { S.sync = 0; S.sense_count = 0; }
            } else if (corr > S.peak_corr) S.peak_corr = corr;
        }
    }
    const bool pass = !S.sync;
    if (FUSED && pass) {                                      // TDCEstimator (dc.hpp:132-163)
        S.sum_dc = cs11a_add16(S.sum_dc, cs11a_dc_term(pi));
        if (S.update_cnt == 0) { S.dc = cs11a_add16(S.dc, cs11a_sra16(S.sum_dc, 2)); S.update_cnt = kCs11aDcInterval; S.sum_dc = 0; }
        S.update_cnt--;
    }
    raised = false;
    if (S.sense_count >= kCs11aMaxSense && !S.sync) { raised = S.error_code != kCs11aTimeout; S.error_code = kCs11aTimeout; }      // cca.hpp:433-437
    return pass;
}

// inclusive prefix sums over the wave: 32-bit wrapping, and packed COMPLEX16 wrapping half by half
// (reach: how many lanes back a sum has to look -- the span's length; wave-uniform)
__device__ __forceinline__ unsigned cs11a_scan32(unsigned t, int lane, uint32_t reach = 64)
{
    for (int o = 1; o < (int)reach; o <<= 1) { const unsigned u = (unsigned)__shfl_up((int)t, o); if (lane >= o) t += u; }
    return t;
}
__device__ __forceinline__ uint32_t cs11a_scan16(uint32_t t, int lane, uint32_t reach = 64)
{
    for (int o = 1; o < (int)reach; o <<= 1) { const uint32_t u = (uint32_t)__shfl_up((int)t, o); if (lane >= o) t = cs11a_add16(t, u); }
    return t;
}
__device__ __forceinline__ void cs11a_win_shift(Cs11aAcc& a, int d) { a.w[0] = a.w[1]; a.w[1] = a.w[2]; a.w[2] = a.w[3]; a.w[3] = d; }

// a window's sum behind every burst of a span: the sum carried in plus the wave prefix sum of (term - term four bursts back: the lane four below, or the window's own)
__device__ __forceinline__ int cs11a_span_sum(const Cs11aAcc& A, unsigned d, int k, bool live, int lane, uint32_t reach)
{
    const unsigned up = (unsigned)__shfl_up((int)d, 4);
    const int w0 = A.w[0], w1 = A.w[1], w2 = A.w[2], w3 = A.w[3];
    const unsigned wk = (unsigned)(k == 0 ? w0 : k == 1 ? w1 : k == 2 ? w2 : w3);
    return (int)((unsigned)A.reg + cs11a_scan32(live ? d - (k >= 4 ? up : wk) : 0u, lane, reach));
}

// The position-parallel pass over a tile while sync_state is no_energy: lane l holds burst l of the tile (v: as it arrives).  From burst b on, with the DC estimate as
// it stands, every lane forms its burst's auto-correlation, energy and estimator terms (the partner four bursts back from the lane four below, or from sample_his), the
// three windowed sums as wave prefix sums of (term - term four bursts back) on top of the sums carried in, and the carrier test; the ballot of the tests gives the first
// true one.  The bursts in front of it are "plain": auto_count 0, sense_count + 4 each, every one through the gate.  They are consumed in closed form up to and including
// the first burst that is an event of its own: the estimator's update (FUSED: the estimate changes every later lane's terms, so the pass ends behind it and is formed
// again), or the burst that raises the time-out.  -> e: bursts b .. e - 1 consumed; hit: burst e is a true carrier test (for the serial step); raised as cs11a_burst.
template <bool FUSED>
__device__ __forceinline__ uint32_t cs11a_plain_span(Cs11a& S, const uint4 v, uint32_t b, uint32_t nv, int lane, bool& hit, bool& raised)
{
    const uint32_t in[4] = { v.x, v.y, v.z, v.w };
    const int k = lane - (int)b;                                // the lane's place in the span
    // the span cannot reach past the estimator's next update (FUSED) or the tile's end: no lane behind that is formed, and the prefix sums look no further back
    const uint32_t reach = FUSED ? min(nv - b, min(S.update_cnt, 64u) + 1u) : nv - b;
    const bool live = k >= 0 && (uint32_t)k < reach;
    uint32_t pi[4], pii[4];
    unsigned sr = 0, si = 0, se = 0;
#pragma unroll
    for (int e = 0; e < 4; e++) {
        pi[e] = FUSED ? cs11a_sub16(in[e], S.dc) : in[e]; pii[e] = cs11a_sra16(pi[e], 2);
        const uint32_t up = (uint32_t)__shfl_up((int)pii[e], 4);
        const uint32_t h0 = S.his[e], h1 = S.his[4 + e], h2 = S.his[8 + e], h3 = S.his[12 + e];      // (read first: a choice between VALUES, not between addresses)
        const uint32_t hk = k == 0 ? h0 : k == 1 ? h1 : k == 2 ? h2 : h3;
        int re, im; const cpx x = unpack(pii[e]);
        conj_mul32(x, unpack(k >= 4 ? up : hk), re, im);
        sr += (unsigned)(re >> 4); si += (unsigned)(im >> 4); se += (unsigned)(sqnorm(x) >> 4);
    }
    const int reg_re = cs11a_span_sum(S.ac_re, sr, k, live, lane, reach), reg_im = cs11a_span_sum(S.ac_im, si, k, live, lane, reach),
              reg_en = cs11a_span_sum(S.energy, se, k, live, lane, reach);
    const int a = (int)((unsigned)cs11a_abs(reg_re) + (unsigned)cs11a_abs(reg_im)), en = reg_en;
    const unsigned long long T = __ballot(live && en > (int)S.thr && a >= en - (en >> 3));
    const uint32_t f1 = T ? (uint32_t)__ffsll((long long)T) - 1u : nv;
    uint32_t e = min(f1, b + reach);
    bool to = false;
    if (S.error_code != kCs11aTimeout) {
        const uint32_t need = S.sense_count >= kCs11aMaxSense ? 1u : (kCs11aMaxSense - S.sense_count + 3u) / 4u;
        if (b + need <= e) { e = b + need; to = true; }
    }
    hit = e == f1 && f1 < nv; raised = false;
    const uint32_t m = e - b;
    if (m == 0) return e;
    const uint32_t last = e - 1u;
    S.auto_count = 0; S.sense_count += 4u * m;
    S.ac_re.reg = cs11a_lane(reg_re, last); S.ac_im.reg = cs11a_lane(reg_im, last); S.energy.reg = cs11a_lane(reg_en, last);
#pragma unroll
    for (uint32_t j = 4; j > 0; j--) {                          // the last four bursts' terms and samples are what the windows and sample_his hold
        if (m < j) continue;
        const uint32_t l = e - j;
        cs11a_win_shift(S.ac_re, cs11a_lane((int)sr, l)); cs11a_win_shift(S.ac_im, cs11a_lane((int)si, l)); cs11a_win_shift(S.energy, cs11a_lane((int)se, l));
#pragma unroll
        for (int i = 0; i < 12; i++) S.his[i] = S.his[i + 4];
#pragma unroll
        for (int i = 0; i < 4; i++) S.his[12 + i] = (uint32_t)cs11a_lane((int)pii[i], l);
    }
    if (FUSED) {                                                // TDCEstimator over the span (dc.hpp:132-163): every plain burst passes the gate
        const uint32_t h = cs11a_scan16(live ? cs11a_dc_term(pi) : 0u, lane, reach);
        S.sum_dc = cs11a_add16(S.sum_dc, (uint32_t)cs11a_lane((int)h, last));
        if (m == S.update_cnt + 1u) { S.dc = cs11a_add16(S.dc, cs11a_sra16(S.sum_dc, 2)); S.sum_dc = 0; S.update_cnt = kCs11aDcInterval - 1u; }
        else S.update_cnt -= m;
    }
    if (to) { S.error_code = kCs11aTimeout; raised = true; }     // cca.hpp:433-437: this burst changes error_code
    return e;
}

// T11aPLCPParser::_parse_plcp (PHY_11a.hpp:548-580) into a record that starts at 0: error_code, data_rate_kbps, frame_length, code_rate, total_symbols.  The
// rejects in the brick's order; behind one the fields hold what it had written by then
__device__ __forceinline__ void plcp_parse11a(uint32_t sig, uint32_t rec[5])
{
    rec[0] = kPlcpHeaderFail; rec[1] = rec[2] = rec[3] = rec[4] = 0;
    sig &= 0xFFFFFFu;
    if (sig & 0xFC0010u) return;                              // the reserved bits
    if (__popc(sig) & 1) return;                              // parity
    const uint32_t code = sig & 0xFu;                         // BB11aParseDataRate (ieee80211a_cmn.h:97-107)
    if (code < 8) return;                                     // data_rate_kbps = 0
    const uint32_t kbps = code == 0x8 ? 48000u : code == 0x9 ? 24000u : code == 0xA ? 12000u : code == 0xB ? 6000u : code == 0xC ? 54000u
                        : code == 0xD ? 36000u : code == 0xE ? 18000u : 9000u;
    rec[1] = kbps;
    rec[3] = code == 0x8 ? (uint32_t)SORA_CR_23 : code >= 0xC ? (uint32_t)SORA_CR_34 : (uint32_t)SORA_CR_12;      // BB11aGetCodingRateFromDataRate: 9, 18, 36, 54 Mbps are 3/4
    const uint32_t len = (sig >> 5) & 0xFFFu;
    rec[2] = len;
    if (len > 2500) return;
    const uint32_t nd = kbps / 250u;                          // N_DBPS: 24 .. 216 = four bits per 1000 kbps
    rec[4] = (len * 8 + 16 + 6 + nd - 1) / nd + 1;           // B11aGetSymbolCount, and this SIGNAL symbol
    rec[0] = 0;
}

}  // namespace sora
