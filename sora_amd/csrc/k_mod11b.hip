// k_mod11b.hip -- the bricks of the 802.11b modulation graph (kernel/bb/demod11/fb11bmod_config.hpp:28-50, CreateModGraph) as stand-alone, batched stages, one C entry
// point each (include/sora_hip.h), with the reference bricks' ports:
//   k_mod11b_ppdu    TBB11bSrc           (PHY_11b.hpp:19-206)        MPDU -> SYNC, SFD, SIGNAL, SERVICE, LENGTH, CRC-16, MPDU, FCS
//   k_mod11b_sc741   TSc741              (scramble.hpp:7-88)         uchar -> uchar
//   k_mod11b_dbpsk   TBB11bDBPSKSpread   (barkerspread.hpp:9-111)    uchar -> COMPLEX8 x 88
//   k_mod11b_dqpsk   TBB11bDQPSKSpread   (barkerspread.hpp:113-225)  uchar -> COMPLEX8 x 44
//   k_mod11b_cck5    TCCK5Encode         (cck.hpp:880-953)           uchar -> COMPLEX8 x 16
//   k_mod11b_cck11   TCCK11Encode        (cck.hpp:782-870)           uchar -> COMPLEX8 x 8
//   k_mod11b_shape   TQuickPulseShaper   (pulse.hpp:254-384)         COMPLEX8 -> COMPLEX16 x 4
// The bricks are stateful streams.  A workgroup owns one stream of the batch and walks it in passes of kMod11bT input units; within a pass the stream lies across the
// lanes, and what a brick carries from unit to unit is restated so that a pass is data-parallel:
//   * the scrambler is linear over GF(2) with a 7-bit state: a lane scrambles a run of four bytes from state 0 (lane 0: from the register), a scan composes the runs
//     (the state after e zero-input steps is M^e s, e mod 127), and a second walk starts every run from its true state;
//   * the differential phase is a sum mod 4 of per-byte quarter turns: a scan; last_phase's encoding enters only where the record is read and written;
//   * a shaper output is the brick's stored partial sum (for the first four steps of a call) plus at most five products of the call's own inputs.
// The pass carries its end state to the next one in registers; the last pass writes the record.  Output goes out by absolute 16-byte words: the elements in front of
// the first boundary of a pass one by one, one word per lane, then the elements behind the last whole word.  The constants are dev_mod11b.h's.
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "dev_tx.h"
#include "dev_mod11b.h"
#include "host_stage.h"

namespace sora {

// ---- TBB11bSrc: the header's geometry is tx11b_plan's, the FCS tx_fcs_waves' (what k_tx11b runs); one workgroup per frame assembles the PPDU in LDS
__global__ void __launch_bounds__(kMod11bThreads) k_mod11b_ppdu(const uint8_t* __restrict__ mpdu, const uint32_t* __restrict__ off, const uint32_t* __restrict__ len,
                                                                const uint32_t* __restrict__ rate, const uint8_t* __restrict__ kind, uint8_t* __restrict__ out,
                                                                const uint32_t* __restrict__ out_first, const uint32_t* __restrict__ crc, const uint32_t* __restrict__ crcz)
{
    __shared__ alignas(16) uint8_t s_byte[24 + 4092 + 4 + 8];                    // PPDU byte b at s_byte[24 - hb + b]: the MPDU starts at s_byte + 24 for either kind
    __shared__ uint32_t s_crc[256];
    __shared__ uint32_t s_z[6 * 8 * 16];
    __shared__ uint32_t s_crcw[2];
    const uint32_t f = blockIdx.x;
    const int tid = threadIdx.x;
    const uint32_t L = len[f];
    Tx11bPlan P;
    if (!tx11b_plan(L, rate[f], P, kind[f])) return;                             // a frame that is not accepted: nothing is written
    const uint32_t HB = P.hb;
    uint8_t* const ppdu = s_byte + (24 - HB);
    if (tid == 0) {
        const uint32_t size = L + 4;                                             // GetPPDULength (PHY_11b.hpp:82-104): microseconds, and the length extension at 11 Mbps
        uint32_t us, ext = 0;
        if (P.cpb == 88) us = size * 8;
        else if (P.cpb == 44) us = size * 4;
        else if (P.cpb == 16) us = (size * 16 + 10) / 11;
        else { us = (size * 8 + 10) / 11; ext = us * 11 - size * 8 >= 8 ? 1u : 0u; }
        uint8_t h[8] = { (uint8_t)P.sfd, (uint8_t)(P.sfd >> 8), (uint8_t)P.code, (uint8_t)(ext << 7), (uint8_t)us, (uint8_t)(us >> 8), 0, 0 };
        uint32_t c = 0xFFFFu;                                                    // CalcCRC16 of SIGNAL..LENGTH: reflected 0x8408, init 0xFFFF, inverted
        for (int i = 2; i < 6; i++) {
            c ^= h[i];
            for (int k = 0; k < 8; k++) c = (c & 1u) ? (c >> 1) ^ 0x8408u : c >> 1;
        }
        c = ~c & 0xFFFFu;
        h[6] = (uint8_t)c; h[7] = (uint8_t)(c >> 8);
        for (uint32_t i = 0; i + 8 < HB; i++) ppdu[i] = (uint8_t)P.sync;
        for (uint32_t i = 0; i < 8; i++) s_byte[16 + i] = h[i];
    }
    mod11b_load_bytes(s_byte + 24, mpdu + off[f], L, tid);
    s_crc[tid] = crc[tid];
    for (int i = tid; i < 6 * 8 * 16; i += kMod11bThreads) s_z[i] = crcz[i];
    __syncthreads();
    if (tid < 128) tx_fcs_waves<2>(s_byte + 24, L, s_crc, s_z, tid, s_crcw);     // FCS = CalcCRC32 of the MPDU, little-endian
    __syncthreads();
    if (tid == 0) {
        const uint32_t fcs = tx_fcs_join<2>(s_z, s_crcw);
        for (uint32_t k = 0; k < 4; k++) s_byte[24 + L + k] = (uint8_t)(fcs >> (8 * k));
    }
    __syncthreads();
    mod11b_store_bytes(out + out_first[f], ppdu, HB + L + 4, tid);
}

// ---- TSc741.  Only the low seven bits of the record are read (the brick indexes a [256][128] table)
__global__ void __launch_bounds__(kMod11bThreads) k_mod11b_sc741(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, const uint32_t* __restrict__ first,
                                                                 const uint32_t* __restrict__ nn, const uint32_t* __restrict__ out_first, uint32_t* __restrict__ reg,
                                                                 uint32_t max_n)
{
    __shared__ alignas(16) uint8_t s_b[kMod11bT + 16];
    __shared__ uint32_t s_scan[kMod11bThreads / 64];
    __shared__ uint32_t s_carry;
    const uint32_t f = blockIdx.x;
    const int tid = threadIdx.x;
    const uint32_t n = min(nn[f], max_n);
    if (n == 0) return;                                                          // (the record stays as it is)
    const uint8_t* const src = in + first[f];
    uint8_t* const dst = out + out_first[f];
    uint32_t carry = reg[f] & 0x7Fu;
    constexpr uint32_t K = kMod11bT / kMod11bThreads;                            // bytes per lane and pass
    for (uint32_t b0 = 0; b0 < n; b0 += kMod11bT) {
        const uint32_t nb = min((uint32_t)kMod11bT, n - b0);
        __syncthreads();                                                         // the pass before has stored s_b
        mod11b_load_bytes(s_b, src + b0, nb, tid);
        __syncthreads();
        const uint32_t blo = min((uint32_t)tid * K, nb), bhi = min(blo + K, nb);
        uint32_t r = tid == 0 ? carry : 0u;
        for (uint32_t b = blo; b < bhi; b++) (void)mod11b_scramble8(s_b[b], r);
        r = mod11b_scan_scr(r, 8 * K, carry, s_scan, tid);                       // the state the lane's run truly starts from
        for (uint32_t b = blo; b < bhi; b++) s_b[b] = (uint8_t)mod11b_scramble8(s_b[b], r);
        if (bhi == nb && blo < nb) s_carry = r;                                  // the lane that holds the pass's last byte
        __syncthreads();
        carry = s_carry;
        mod11b_store_bytes(dst + b0, s_b, nb, tid);
    }
    if (tid == 0) reg[f] = carry;
}

// ---- the four spreaders over CF_DifferentialMap::last_phase.  KIND 0: DBPSK, 1: DQPSK (Barker, 11 chips a symbol), 2: CCK 5.5, 3: CCK 11 (8 chips a symbol)
template <int KIND> struct Mod11bSpread {
    static constexpr uint32_t SPB = KIND == 0 ? 8 : KIND == 1 ? 4 : KIND == 2 ? 2 : 1;   // symbols a byte
    static constexpr uint32_t LS = KIND < 2 ? 11 : 8;                                     // chips a symbol
    static constexpr uint32_t CPB = SPB * LS;                                             // 88, 44, 16, 8
};
// the quarter turns byte v adds to the differential phase (odd: TCCK11Encode's bEven at this byte)
template <int KIND> __device__ __forceinline__ uint32_t mod11b_inc(uint32_t v, uint32_t odd)
{
    if (KIND == 0) return 2 * (__popc(v) & 1);                                   // pi per one bit
    if (KIND == 1) return mod11b_dq(v & 3) + mod11b_dq((v >> 2) & 3) + mod11b_dq((v >> 4) & 3) + mod11b_dq(v >> 6);
    if (KIND == 2) return mod11b_dq(v & 3) + mod11b_dq((v >> 4) & 3) + 2;        // two symbols, the second one turned by pi
    return mod11b_dq(v & 3) + 2 * odd;                                           // odd symbols: pi more
}
// the chip angles of symbol i of byte v, chip 0 in the lowest two bits; p: the phase in front of the byte
template <int KIND> __device__ __forceinline__ uint32_t mod11b_sym_word(uint32_t v, uint32_t p, uint32_t i, uint32_t odd)
{
    if (KIND == 0) return kMod11bBarker22 ^ (((p + 2 * (__popc(v & ((2u << i) - 1u)) & 1)) & 3u) * kMod11bRep11);   // the bits up to this one flip the phase
    if (KIND == 1) {                                                             // dibits 0..i
        uint32_t a = p;
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) a += k <= i ? mod11b_dq((v >> (2 * k)) & 3u) : 0u;
        return kMod11bBarker22 ^ ((a & 3u) * kMod11bRep11);
    }
    uint32_t a, p2, p3, p4;
    if (KIND == 2) {                                                             // d0 d1 -> phi1, d2 -> phi2 = pi/2 + d2 pi, phi3 = 0, d3 -> phi4 = d3 pi
        const uint32_t nib = (v >> (4 * i)) & 15u;
        a = p + mod11b_dq(v & 3u) + (i ? mod11b_dq((v >> 4) & 3u) + 2 : 0u);
        p2 = 1 + 2 * ((nib >> 2) & 1u); p3 = 0; p4 = 2 * (nib >> 3);
    } else {                                                                     // d0 d1 -> phi1, d2..d7 -> phi2..phi4
        a = p + mod11b_dq(v & 3u) + 2 * odd;
        p2 = mod11b_cq((v >> 2) & 3u); p3 = mod11b_cq((v >> 4) & 3u); p4 = mod11b_cq(v >> 6);
    }
    const uint32_t o[8] = { p2 + p3 + p4, p3 + p4, p2 + p4, p4 + 2, p2 + p3, p3, p2 + 2, 0 };
    uint32_t w = 0;
#pragma unroll
    for (int c = 0; c < 8; c++) w |= ((a + o[c]) & 3u) << (2 * c);
    return w;
}

template <int KIND>
__device__ __forceinline__ void mod11b_spread(const uint8_t* __restrict__ in, uint16_t* __restrict__ out, const uint32_t* __restrict__ first,
                                              const uint32_t* __restrict__ nn, const uint32_t* __restrict__ out_first, uint32_t* __restrict__ state, uint32_t max_n)
{
    using G = Mod11bSpread<KIND>;
    __shared__ alignas(16) uint8_t s_in[kMod11bT + 16];
    __shared__ uint8_t s_ph[kMod11bT + 16];                                      // quarter turns in front of each byte
    __shared__ uint32_t s_scan[kMod11bThreads / 64];
    const uint32_t f = blockIdx.x;
    const int tid = threadIdx.x;
    const uint32_t n = min(nn[f], max_n);
    if (n == 0) return;                                                          // (the record stays as it is)
    const uint8_t* const src = in + first[f];
    uint16_t* const dst = out + out_first[f];
    const uint32_t code = state[4 * f];
    const uint32_t even0 = KIND == 3 ? state[4 * f + 1] & 1u : 0u;
    uint32_t ph = KIND == 0 ? 2 * (code & 1u) : mod11b_turns_of_code(code);      // m_Coding_LUT[b][m_reg & 1]: the DBPSK brick starts at 0 or pi
    constexpr uint32_t K = kMod11bT / kMod11bThreads;
    for (uint32_t b0 = 0; b0 < n; b0 += kMod11bT) {
        const uint32_t nb = min((uint32_t)kMod11bT, n - b0);
        __syncthreads();                                                         // the pass before has read s_in and s_ph
        mod11b_load_bytes(s_in, src + b0, nb, tid);
        __syncthreads();
        uint32_t inc[K], sum = 0;
#pragma unroll
        for (uint32_t k = 0; k < K; k++) {
            const uint32_t b = K * tid + k;
            inc[k] = b < nb ? mod11b_inc<KIND>(s_in[b], (even0 + b0 + b) & 1u) : 0u;
            sum += inc[k];
        }
        uint32_t total;
        uint32_t p = ph + mod11b_scan_add(sum, s_scan, tid, total);
#pragma unroll
        for (uint32_t k = 0; k < K; k++) {
            const uint32_t b = K * tid + k;
            if (b < nb) s_ph[b] = (uint8_t)(p & 3u);
            p += inc[k];
        }
        ph = (ph + total) & 3u;
        __syncthreads();
        uint16_t* const o = dst + (size_t)b0 * G::CPB;
        const uint32_t nchips = nb * G::CPB, head = mod11b_head(o, nchips, 2), nw = (nchips - head) / 8;
        auto word = [&](uint32_t b, uint32_t i) { return b < nb ? mod11b_sym_word<KIND>(s_in[b], s_ph[b], i, (even0 + b0 + b) & 1u) : 0u; };
        auto chip = [&](uint32_t c) {
            const uint32_t b = c / G::CPB, j = c - b * G::CPB, i = j / G::LS, k = j - i * G::LS;
            return (uint16_t)mod11b_chip(word(b, i) >> (2 * k));
        };
        for (uint32_t c = tid; c < head; c += kMod11bThreads) o[c] = chip(c);
        for (uint32_t w = tid; w < nw; w += kMod11bThreads) {                    // eight chips, one store: they lie in one symbol or in two
            const uint32_t c0 = head + 8 * w;
            const uint32_t b = c0 / G::CPB, j = c0 - b * G::CPB, i = j / G::LS, k = j - i * G::LS;
            const uint32_t i1 = i + 1 == G::SPB ? 0u : i + 1, b1 = i + 1 == G::SPB ? b + 1 : b;
            const uint32_t ws = (word(b, i) >> (2 * k)) | (G::LS - k >= 8 ? 0u : word(b1, i1) << (2 * (G::LS - k)));
            uint32_t h[4];
#pragma unroll
            for (int q = 0; q < 4; q++) h[q] = mod11b_chip(ws >> (4 * q)) | (mod11b_chip(ws >> (4 * q + 2)) << 16);
            *reinterpret_cast<uint4*>(o + c0) = make_uint4(h[0], h[1], h[2], h[3]);
        }
        for (uint32_t c = head + 8 * nw + tid; c < nchips; c += kMod11bThreads) o[c] = chip(c);
    }
    if (tid == 0) {
        state[4 * f] = mod11b_code_of_turns(ph);                                 // (the DBPSK brick leaves 0 or 3: its phase is 0 or pi)
        if (KIND == 3) state[4 * f + 1] = (even0 + n) & 1u;
    }
}
#define MOD11B_SPREAD(name, KIND) \
    __global__ void __launch_bounds__(kMod11bThreads) name(const uint8_t* in, uint16_t* out, const uint32_t* first, const uint32_t* nn, const uint32_t* out_first, \
                                                           uint32_t* state, uint32_t max_n) { mod11b_spread<KIND>(in, out, first, nn, out_first, state, max_n); }
MOD11B_SPREAD(k_mod11b_dbpsk, 0)
MOD11B_SPREAD(k_mod11b_dqpsk, 1)
MOD11B_SPREAD(k_mod11b_cck5, 2)
MOD11B_SPREAD(k_mod11b_cck11, 3)
#undef MOD11B_SPREAD

// ---- TQuickPulseShaper.  QuickShape (pulse.hpp:370-383): out = x tap[0] + m_temps[0]; m_temps[i] = m_temps[i + 1] + x tap[i + 1], mul_low and wrapping 16-bit adds,
// m_temps[4] never written.  Unrolled from the record S the call starts with: sample s of step m is
//     wrap16(S[m][s] (m < 4) + sum_{j = 0 .. min(m, 4)} x[m - j] tap[4 j + s])
// and the record after N steps is row i = what step N + i has collected from the inputs x[.. N - 1].  x[k] is 0 behind the stream's chips (Flush feeds zeros).
// The four samples of step m, the inputs read through X (x[k] as a packed COMPLEX8, 0 where there is none); M: the step's number in the call
template <class XF>
__device__ __forceinline__ void mod11b_step4(XF X, uint32_t M, const uint32_t* s_st, uint32_t w[4])
{
    int re[4] = { 0, 0, 0, 0 }, im[4] = { 0, 0, 0, 0 };
#pragma unroll
    for (int j = 0; j < 5; j++) {
        const uint32_t x = X(j);                                                 // x[M - j]
        const int xr = (int)(int8_t)(x & 0xFFu), xi = (int)(int8_t)(x >> 8);
#pragma unroll
        for (int s = 0; s < 4; s++) { re[s] += xr * kMod11bTaps[4 * j + s]; im[s] += xi * kMod11bTaps[4 * j + s]; }
    }
#pragma unroll
    for (int s = 0; s < 4; s++) {
        const uint32_t st = M < 4 ? s_st[4 * M + s] : 0u;
        w[s] = (((uint32_t)re[s] + (st & 0xFFFFu)) & 0xFFFFu) | (((uint32_t)im[s] + (st >> 16)) << 16);
    }
}
__device__ __forceinline__ uint32_t mod11b_pick(const uint32_t a[4], const uint32_t b[4], uint32_t t)   // element t of a | b without a register index
{
    uint32_t r = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4; k++) { r = t == k ? a[k] : r; r = t == k + 4 ? b[k] : r; }
    return r;
}

__global__ void __launch_bounds__(kMod11bThreads) k_mod11b_shape(const uint16_t* __restrict__ in, uint32_t* __restrict__ out, const uint32_t* __restrict__ first,
                                                                 const uint32_t* __restrict__ nn, const uint32_t* __restrict__ out_first, const uint8_t* __restrict__ flush,
                                                                 uint32_t* __restrict__ state, uint32_t max_n)
{
    __shared__ uint32_t s_x[kMod11bT + 8];                                       // x[m0 - 4 ..] of the pass
    __shared__ uint32_t s_st[16];
    const uint32_t f = blockIdx.x;
    const int tid = threadIdx.x;
    const uint32_t n = min(nn[f], max_n);
    const uint32_t N = n + ((flush && flush[f]) ? 5u : 0u);                      // Flush: five more bursts from zero input
    if (N == 0) return;                                                          // (the record stays as it is)
    const uint16_t* const src = in + first[f];
    uint32_t* const dst = out + out_first[f];
    if (tid < 16) s_st[tid] = state[16 * f + tid];
    for (uint32_t m0 = 0; m0 < N; m0 += kMod11bT) {
        const uint32_t nm = min((uint32_t)kMod11bT, N - m0);
        __syncthreads();                                                         // the pass before has read s_x
        for (uint32_t i = tid; i < nm + 4; i += kMod11bThreads) {
            const uint32_t m = m0 + i;                                           // x[m - 4]
            s_x[i] = (m >= 4 && m - 4 < n) ? (uint32_t)src[m - 4] : 0u;
        }
        __syncthreads();
        uint32_t* const o = dst + (size_t)4 * m0;
        const uint32_t nsamp = 4 * nm, head = mod11b_head(o, nsamp, 4), nw = (nsamp - head) / 4;
        auto step = [&](uint32_t m, uint32_t w[4]) { mod11b_step4([&](int j) { return s_x[m + 4 - j]; }, m0 + m, s_st, w); };
        if ((uint32_t)tid < head) {                                              // samples 0 .. head - 1 of the pass's first step
            uint32_t a[4]; step(0, a);
            o[tid] = mod11b_pick(a, a, (uint32_t)tid);
        }
        for (uint32_t w = tid; w < nw; w += kMod11bThreads) {                    // four samples, one store: of one step, or of two where the stream starts off a boundary
            uint32_t a[4], b[4] = { 0, 0, 0, 0 };
            step(w, a);
            if (head) step(w + 1, b);
            uint4 v;
            v.x = mod11b_pick(a, b, head); v.y = mod11b_pick(a, b, head + 1); v.z = mod11b_pick(a, b, head + 2); v.w = mod11b_pick(a, b, head + 3);
            *reinterpret_cast<uint4*>(o + head + 4 * w) = v;
        }
        const uint32_t q0 = head + 4 * nw;                                       // the samples behind the last whole word: of the pass's last step
        if (q0 + tid < nsamp) {
            uint32_t a[4]; step(nm - 1, a);
            o[q0 + tid] = mod11b_pick(a, a, (q0 + tid) & 3u);
        }
    }
    __syncthreads();
    if (tid < 4) {                                                               // row tid of the record: step N + tid over the inputs x[.. N - 1]
        uint32_t w[4];
        const uint32_t M = N + (uint32_t)tid;
        mod11b_step4([&](int j) { const uint32_t k = M - (uint32_t)j; return (k < N && k < n) ? (uint32_t)src[k] : 0u; }, M, s_st, w);
#pragma unroll
        for (int s = 0; s < 4; s++) state[16 * f + 4 * tid + s] = w[s];
    }
}

}  // namespace sora

using namespace sora;

// ---- the stage entry points (host_stage.h: the prologue and helpers every stage shares): a workgroup per stream
static_assert(sizeof(sora_mod11b_state) == 16 && sizeof(sora_shaper11b_state) == 64, "the 802.11b modulation stage records are 32-bit words");
constexpr size_t kMod11bMaxN = (size_t)1 << 24;             // 88 chips a byte: a stream's output offsets stay 32-bit

int sora_hip_ppdu11b(const uint8_t* d_mpdu, const uint32_t* d_off, const uint32_t* d_len, const uint32_t* d_rate_kbps, const uint8_t* d_preamble, uint8_t* d_out,
                     const uint32_t* d_out_first, size_t nframes, void* stream)
{
    STAGE_ENTRY("sora_hip_ppdu11b", !d_mpdu || !d_off || !d_len || !d_rate_kbps || !d_preamble || !d_out || !d_out_first, nframes)
    Tables T; if (const int rc = stage_tables(&T)) return rc;
    hipLaunchKernelGGL(k_mod11b_ppdu, dim3((unsigned)nframes), dim3(256), 0, (hipStream_t)stream, d_mpdu, d_off, d_len, d_rate_kbps, d_preamble, d_out, d_out_first, T.crc, T.crcz);
    return launch_result("k_mod11b_ppdu");
}

int sora_hip_sc741_11b(const uint8_t* d_in, const uint32_t* d_first, const uint32_t* d_n, const uint32_t* d_out_first, uint32_t* d_reg, uint8_t* d_out,
                       size_t nstreams, size_t max_n, void* stream)
{
    STAGE_ENTRY("sora_hip_sc741_11b", !d_in || !d_first || !d_n || !d_out_first || !d_reg || !d_out, nstreams)
    if (max_n == 0) return SORA_OK;
    if (max_n > kMod11bMaxN) return sora_internal_fail(SORA_ERR_CAPACITY, "sora_hip_sc741_11b: max_n is too large for one call", 0);
    hipLaunchKernelGGL(k_mod11b_sc741, dim3((unsigned)nstreams), dim3(256), 0, (hipStream_t)stream, d_in, d_out, d_first, d_n, d_out_first, d_reg, (uint32_t)max_n);
    return launch_result("k_mod11b_sc741");
}

#define MOD11B_SPREAD(name, kernel) \
    int name(const uint8_t* d_in, const uint32_t* d_first, const uint32_t* d_n, const uint32_t* d_out_first, sora_mod11b_state* d_state, int8_t* d_out, size_t nstreams, \
             size_t max_n, void* stream) \
    { \
        STAGE_ENTRY(#name, !d_in || !d_first || !d_n || !d_out_first || !d_state || !d_out, nstreams) \
        if (max_n == 0) return SORA_OK; \
        if (max_n > kMod11bMaxN) return sora_internal_fail(SORA_ERR_CAPACITY, #name ": max_n is too large for one call", 0); \
        if ((uintptr_t)d_out & 1) return sora_internal_fail(SORA_ERR_INVALID_PARAM, #name ": d_out must be aligned to a COMPLEX8", 0); \
        hipLaunchKernelGGL(kernel, dim3((unsigned)nstreams), dim3(256), 0, (hipStream_t)stream, d_in, reinterpret_cast<uint16_t*>(d_out), d_first, d_n, d_out_first, \
                           u32(d_state), (uint32_t)max_n); \
        return launch_result(#kernel); \
    }
MOD11B_SPREAD(sora_hip_dbpsk_spread11b, k_mod11b_dbpsk)
MOD11B_SPREAD(sora_hip_dqpsk_spread11b, k_mod11b_dqpsk)
MOD11B_SPREAD(sora_hip_cck5_encode11b, k_mod11b_cck5)
MOD11B_SPREAD(sora_hip_cck11_encode11b, k_mod11b_cck11)
#undef MOD11B_SPREAD

int sora_hip_pulse_shape11b(const int8_t* d_in, const uint32_t* d_first, const uint32_t* d_n, const uint32_t* d_out_first, const uint8_t* d_flush,
                            sora_shaper11b_state* d_state, sora_complex16* d_out, size_t nstreams, size_t max_n, void* stream)
{
    STAGE_ENTRY("sora_hip_pulse_shape11b", !d_in || !d_first || !d_n || !d_out_first || !d_state || !d_out, nstreams)
    if (max_n == 0 && !d_flush) return SORA_OK;
    if (max_n > kMod11bMaxN) return sora_internal_fail(SORA_ERR_CAPACITY, "sora_hip_pulse_shape11b: max_n is too large for one call", 0);
    if (((uintptr_t)d_in & 1) || !aligned4(d_out)) return sora_internal_fail(SORA_ERR_INVALID_PARAM, "sora_hip_pulse_shape11b: d_in and d_out must be aligned to their elements", 0);
    hipLaunchKernelGGL(k_mod11b_shape, dim3((unsigned)nstreams), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const uint16_t*>(d_in), u32(d_out), d_first, d_n, d_out_first,
                       d_flush, u32(d_state), (uint32_t)max_n);
    return launch_result("k_mod11b_shape");
}
