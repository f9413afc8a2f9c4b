// k_11b.hip -- the bricks of the 802.11b receive graph (CreateDemodGraph, kernel/bb/demod11/fb11bdemod_config.hpp:122-172) as stand-alone, batched stages, one C entry
// point each (include/sora_hip.h: sora_hip_*11b).  The bricks are stateful streams: a call works on `nstreams` independent streams described by device tables (stream f:
// n[f] units from unit first[f] of the input, written from unit out_first[f] of the output) and a state record per stream, all 32-bit words; first and out_first count
// elements (samples, chips, symbols, bytes) and need no alignment, n counts units.
//   k_11b_dc_remove      TDCRemove                 (Brick11/src/dc.hpp:6-38)               COMPLEX16 x 4  -> COMPLEX16 x 4
//   k_11b_energy_detect  TEnergyDetect + TDCEstimator (cca.hpp:11-98, dc.hpp:92-166)       COMPLEX16 x 4  -> (state)
//   k_11b_symtiming      TSymTiming                (symtiming.hpp:10-170)                  COMPLEX16 x 28 -> COMPLEX16 x 6 / 7 / 8
//   k_11b_barker_sync    TBarkerSync               (symtiming.hpp:176-315)                 COMPLEX16 x 1  -> (the chips behind it)
//   k_11b_despread       TBB11bDespread            (barkerspread.hpp:277-303)              COMPLEX16 x 11 -> COMPLEX16 x 1
//   k_11b_sfd_sync       TSFDSync                  (sfd_sync.hpp:10-134)                   COMPLEX16 x 1  -> (state)
//   k_11b_demap<BITS>    TDBPSKDemap / TDQPSKDemap (barkerspread.hpp:312-454)              COMPLEX16 x 8 / 4 -> uchar
//   k_11b_cck<R>         TCCK5P5Decoder / TCCK11Decoder (cck.hpp:70-206, 255-763)          COMPLEX16 x 16 / 8 -> uchar
//   k_11b_desc741        TDesc741                  (scramble.hpp:93-170)                   uchar -> uchar
//   k_11b_plcp_parse     TBB11bPlcpParser          (PHY_11b.hpp:524-640)                   uchar x 6 -> record
//   k_11b_frame_sink     TBB11bFrameSink           (PHY_11b.hpp:643-749)                   uchar x frame_length -> record
// The position-parallel stages (dc_remove, despread, demap, cck, desc741) are one output unit per lane, workgroup (f, c) taking units 256 c .. of stream f; what a unit needs
// of the stream before it is its neighbour's input (the symbol before, the byte before), the stream's first unit takes it from the state.  Their states are written by
// k_11b_stream_state, launched BEHIND them on the same stream: the first lanes of a stream read the record while its last lanes would write it.  The three searches and the
// sink are one wave per stream: the lanes bring the per-position quantity (the burst energies, the scaled chips, the differential bits, the CRC table) into LDS, lane 0 walks
// the brick's short state machine over it, the lanes write the record's words back.  The arithmetic is dev_11b.h's.
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "dev_11b.h"
#include "host_stage.h"

namespace sora {

// a workgroup's `cnt` units of NC words (contiguous in global memory, any alignment) into LDS by coalesced word loads, unit u at s + u * (NC | 1): an odd stride, so the
// lanes' reads of their own unit meet no bank twice
template <int NC>
__device__ __forceinline__ void b11_stage(uint32_t* s, const uint32_t* __restrict__ src, uint32_t cnt)
{
    for (uint32_t q = threadIdx.x; q < cnt * NC; q += 256u) { const uint32_t u = q / NC; s[u * (NC | 1) + (q - u * NC)] = src[q]; }
    __syncthreads();
}

// ---- TDCRemove: out = wrap16(in - dc[f]), a lane per sample
__global__ void __launch_bounds__(256) k_11b_dc_remove(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, const uint32_t* __restrict__ first, const uint32_t* __restrict__ n,
        const uint32_t* __restrict__ out_first, const uint32_t* __restrict__ dc, uint32_t nstreams, uint32_t chunks)
{
    const uint32_t f = blockIdx.x / chunks, i = (blockIdx.x - f * chunks) * 256u + threadIdx.x;
    if (f >= nstreams || i >= 4u * n[f]) return;
    out[(size_t)out_first[f] + i] = pack(csub16(unpack(in[(size_t)first[f] + i]), unpack(dc[f])));
}

// ---- TBB11bDespread: lane l despreads the 11 chips of symbol l of its workgroup's tile
__global__ void __launch_bounds__(256) k_11b_despread(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, const uint32_t* __restrict__ first, const uint32_t* __restrict__ n,
        const uint32_t* __restrict__ out_first, uint32_t nstreams, uint32_t chunks)
{
    __shared__ uint32_t s_c[256 * 11];
    const uint32_t f = blockIdx.x / chunks, i0 = (blockIdx.x - f * chunks) * 256u;
    if (f >= nstreams || i0 >= n[f]) return;                                     // (uniform per workgroup)
    const uint32_t cnt = min(256u, n[f] - i0);
    b11_stage<11>(s_c, in + (size_t)first[f] + (size_t)i0 * 11, cnt);
    if (threadIdx.x < cnt) out[(size_t)out_first[f] + i0 + threadIdx.x] = b11_despread(s_c + threadIdx.x * 11);
}

// ---- TDBPSKDemap (BITS = 1: 8 symbols per byte) / TDQPSKDemap (BITS = 2: 4 symbols per byte): a lane takes its byte's symbols and the symbol before them
template <int BITS>
__global__ void __launch_bounds__(256) k_11b_demap(const uint32_t* __restrict__ in, uint8_t* __restrict__ out, const uint32_t* __restrict__ first, const uint32_t* __restrict__ n,
        const uint32_t* __restrict__ out_first, const uint32_t* __restrict__ state, uint32_t nstreams, uint32_t chunks)
{
    constexpr int NS = 8 / BITS;
    __shared__ uint32_t s_x[256 * (NS | 1)];
    const uint32_t f = blockIdx.x / chunks, i0 = (blockIdx.x - f * chunks) * 256u;
    if (f >= nstreams || i0 >= n[f]) return;
    const uint32_t cnt = min(256u, n[f] - i0), i = i0 + threadIdx.x;
    const uint32_t* src = in + (size_t)first[f] + (size_t)i0 * NS;
    b11_stage<NS>(s_x, src, cnt);
    if (threadIdx.x >= cnt) return;
    const uint32_t* w = s_x + threadIdx.x * (NS | 1);
    cpx ref = unpack(i == 0 ? state[4 * f] : threadIdx.x == 0 ? src[-1] : w[-2]);   // (the unit before ends one pad word in front of this one)
    uint32_t r = 0;
#pragma unroll
    for (int k = 0; k < NS; k++) {
        const cpx x = unpack(w[k]);
        r |= (BITS == 1 ? b11_dot_sign(ref, x) : b11_dqpsk_bits<0>(ref, x)) << (BITS * k);
        ref = x;
    }
    out[(size_t)out_first[f] + i] = (uint8_t)r;
}
template __global__ void k_11b_demap<1>(const uint32_t*, uint8_t*, const uint32_t*, const uint32_t*, const uint32_t*, const uint32_t*, uint32_t, uint32_t);
template __global__ void k_11b_demap<2>(const uint32_t*, uint8_t*, const uint32_t*, const uint32_t*, const uint32_t*, const uint32_t*, uint32_t, uint32_t);

// ---- TCCK5P5Decoder (R = 5: 16 chips per byte, two half bytes) / TCCK11Decoder (R = 11: 8 chips per byte; byte i of a stream is an odd symbol where is_even ^ (i & 1))
template <int R>
__global__ void __launch_bounds__(256) k_11b_cck(const uint32_t* __restrict__ in, uint8_t* __restrict__ out, const uint32_t* __restrict__ first, const uint32_t* __restrict__ n,
        const uint32_t* __restrict__ out_first, const uint32_t* __restrict__ state, uint32_t nstreams, uint32_t chunks)
{
    constexpr int NC = R == 5 ? 16 : 8;
    __shared__ uint32_t s_x[256 * (NC | 1)];
    const uint32_t f = blockIdx.x / chunks, i0 = (blockIdx.x - f * chunks) * 256u;
    if (f >= nstreams || i0 >= n[f]) return;
    const uint32_t cnt = min(256u, n[f] - i0), i = i0 + threadIdx.x;
    const uint32_t* src = in + (size_t)first[f] + (size_t)i0 * NC;
    b11_stage<NC>(s_x, src, cnt);
    if (threadIdx.x >= cnt) return;
    const uint32_t* w = s_x + threadIdx.x * (NC | 1);
    cpx ref = unpack(i == 0 ? state[4 * f] : threadIdx.x == 0 ? src[-1] : w[-2]);
    uint32_t o = 0;
#pragma unroll
    for (int half = 0; half < NC / 8; half++) {
        cpx P[8];
#pragma unroll
        for (int k = 0; k < 8; k++) P[k] = unpack(w[8 * half + k]);
        if (R == 5) {
            o |= (b11_cck5_nibble(P) | b11_dqpsk_bits<1>(ref, P[7])) << (4 * half);
            if (half == 1) o ^= 0x30u;
        } else {
            o = b11_cck11_bits(P) | b11_dqpsk_bits<1>(ref, P[7]);
            if ((state[4 * f + 2] ^ i) & 1u) o ^= 3u;
        }
        ref = P[7];
    }
    out[(size_t)out_first[f] + i] = (uint8_t)o;
}
template __global__ void k_11b_cck<5>(const uint32_t*, uint8_t*, const uint32_t*, const uint32_t*, const uint32_t*, const uint32_t*, uint32_t, uint32_t);
template __global__ void k_11b_cck<11>(const uint32_t*, uint8_t*, const uint32_t*, const uint32_t*, const uint32_t*, const uint32_t*, uint32_t, uint32_t);

// ---- TDesc741: self-synchronising, so byte i needs byte i - 1 alone (the stream's first byte: the register)
__global__ void __launch_bounds__(256) k_11b_desc741(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, const uint32_t* __restrict__ first, const uint32_t* __restrict__ n,
        const uint32_t* __restrict__ out_first, const uint32_t* __restrict__ state, uint32_t nstreams, uint32_t chunks)
{
    const uint32_t f = blockIdx.x / chunks, i = (blockIdx.x - f * chunks) * 256u + threadIdx.x;
    if (f >= nstreams || i >= n[f]) return;
    const uint8_t* src = in + (size_t)first[f] + i;
    const uint32_t reg7 = i == 0 ? state[4 * f + 1] : (uint32_t)src[-1] >> 1;
    out[(size_t)out_first[f] + i] = (uint8_t)b11_desc741(reg7, src[0]);
}

// ---- the state behind a call of the five stream stages above (launched after them): kind 0 / 1 = DBPSK / DQPSK demap, 2 / 3 = CCK 5.5 / 11 (last_symbol = the stream's
// last input symbol; CCK 11: is_even ^= n & 1), 4 = TDesc741 (byte_reg = the last input byte >> 1).  A stream of 0 units keeps its record.
__global__ void __launch_bounds__(256) k_11b_stream_state(const void* __restrict__ in, const uint32_t* __restrict__ first, const uint32_t* __restrict__ n, uint32_t* __restrict__ state,
        uint32_t nstreams, int kind)
{
    const uint32_t f = blockIdx.x * 256u + threadIdx.x;
    if (f >= nstreams || n[f] == 0) return;
    if (kind == 4) { state[4 * f + 1] = (uint32_t)static_cast<const uint8_t*>(in)[(size_t)first[f] + n[f] - 1] >> 1; return; }
    const uint32_t per = kind == 0 ? 8u : kind == 1 ? 4u : kind == 2 ? 16u : 8u;
    state[4 * f] = static_cast<const uint32_t*>(in)[(size_t)first[f] + (size_t)n[f] * per - 1];
    if (kind == 3) state[4 * f + 2] = (state[4 * f + 2] ^ n[f]) & 1u;
}

// ---- TSymTiming: one wave per stream, tiles of 64 blocks of 28 samples (under 8 KB of LDS: some twenty streams' walks share a CU and hide each other's latency).
// Per tile: (1) the tile is staged in LDS (29 words per block: an odd stride); lane b sums the
// four phase energies of block b and boils them down to what AdjustTiming would do for each of the four values m_index can have there: 4 bits each (b11_timing_code), one word per block; (2) the
// wave walks the recurrence of m_index / m_frag over those words ALONE -- the words come 64 at a time into one register, block j's by v_readlane, so the walk is a chain of scalar
// instructions with no memory access on it -- and leaves each block's first index and output position; (3) lane b gathers its block's 6, 7 or 8 chips from LDS to that position.
// state = { m_index, m_frag }.  A block gives at most 8 chips: an m_index below -4, which no brick holds, is decimated as -4.
constexpr int kSymtTile = 64;                                                   // = the workgroup: one wave
__global__ void __launch_bounds__(kSymtTile) k_11b_symtiming(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, const uint32_t* __restrict__ first, const uint32_t* __restrict__ n,
        const uint32_t* __restrict__ out_first, int* __restrict__ state, uint32_t* __restrict__ nchips, uint32_t nstreams)
{
    __shared__ uint32_t s_x[kSymtTile * 29];
    __shared__ uint32_t s_code[kSymtTile];
    __shared__ uint32_t s_rec[kSymtTile];                                        // (first index + 4) << 16 | the block's first chip, counted from the tile's
    __shared__ int s_st[2];
    __shared__ uint32_t s_total;
    const uint32_t f = blockIdx.x;
    if (f >= nstreams) return;
    const int tid = threadIdx.x;
    const uint32_t nb = n[f];
    const uint32_t* src = in + first[f];
    uint32_t* dst = out + out_first[f];
    if (tid == 0) { s_st[0] = state[2 * f]; s_st[1] = state[2 * f + 1]; s_total = 0; }
    for (uint32_t b0 = 0; b0 < nb; b0 += kSymtTile) {                            // (uniform per workgroup)
        const int cnt = (int)min((uint32_t)kSymtTile, nb - b0);
        __syncthreads();
        for (int q = tid; q < cnt * 28; q += kSymtTile) { const int b = q / 28; s_x[b * 29 + (q - 28 * b)] = src[(size_t)b0 * 28 + q]; }
        __syncthreads();
        if (tid < cnt) {
            int sum[4] = { 0, 0, 0, 0 };
#pragma unroll
            for (int i = 0; i < 28; i++) sum[i & 3] = wadd32(sum[i & 3], sqnorm(sra(unpack(s_x[tid * 29 + i]), 3)));
            uint32_t code = 0;
#pragma unroll
            for (int mi = 0; mi < 4; mi++)                                       // AdjustTiming at each of the four sampling phases
                code |= b11_timing_code(b11_adjust_timing(sum[mi], sum[(mi + 3) & 3], sum[(mi + 1) & 3])) << (4 * mi);
            s_code[tid] = code;
        }
        __syncthreads();
        const uint32_t base = s_total;
#ifdef SORA_DBG_SYMT_NO_SCAN                                                     // tools/bench_11b_stages.py: the kernel without the recurrence (7 chips from index 2 per block): what the scan costs
        if (tid < cnt) s_rec[tid] = (6u << 16) | (7u * tid);
        __syncthreads();
        if (tid == 0) s_total = base + 7u * cnt;
#else
        {                                                                        // every lane alike: the compiler keeps the walk in scalar registers
            int mi = uni(s_st[0]), fr = uni(s_st[1]); uint32_t pos = 0;
            for (int j0 = 0; j0 < cnt; j0 += 64) {
                const uint32_t codes = s_code[min(j0 + tid, kSymtTile - 1)];
                uint32_t mine = 0;
                const int m = min(64, cnt - j0);
                for (int j = 0; j < m; j++) {
                    const uint32_t code = (uint32_t)__builtin_amdgcn_readlane((int)codes, j);
                    mi = max(mi, -4);
                    const int idx0 = mi;                                         // Decimation (:66-83): indices idx0, idx0 + 4, .. < 28; a negative one reads sample 0 and moves m_index by 4
                    const int c = idx0 < 28 ? (28 - idx0 + 3) / 4 : 0;
                    if (mi < 0) mi += 4 * min(c, (3 - mi) / 4);
                    if (mi >= 4) mi = 0;
                    const uint32_t rec = ((uint32_t)(idx0 + 4) << 16) | pos;
                    mine = tid == j ? rec : mine;
                    pos += (uint32_t)c;
                    b11_timing_carry(b11_timing_of(code >> (4 * mi)), mi, fr);                  // (selects, not branches: the chain stays a dozen scalar instructions)
                }
                if (tid < m) s_rec[j0 + tid] = mine;
            }
            if (tid == 0) { s_st[0] = mi; s_st[1] = fr; s_total = base + pos; }
        }
#endif
        __syncthreads();
        if (tid < cnt) {
            const uint32_t rec = s_rec[tid];
            const int idx0 = (int)(rec >> 16) - 4;
            uint32_t* o = dst + base + (rec & 0xFFFFu);
            int j = 0;
            for (int idx = idx0; idx < 28; idx += 4) o[j++] = s_x[tid * 29 + max(idx, 0)];
        }
    }
    __syncthreads();
    if (tid < 2) state[2 * f + tid] = s_st[tid];
    if (tid == 2) nchips[f] = s_total;
}

// ---- TEnergyDetect with the TDCEstimator it feeds: one wave per stream.  The lanes put each burst's energy (sum of sqnorm >> 5) and DC share (sum of x >> 5) into LDS, 64
// bursts at a time; lane 0 walks the brick over them until power is detected or an error stands.  state: sora_energy11b_state, 17 words.
constexpr int kEnergyWords = 17;
__global__ void __launch_bounds__(64) k_11b_energy_detect(const uint32_t* __restrict__ in, const uint32_t* __restrict__ first, const uint32_t* __restrict__ n, uint32_t* __restrict__ state,
        uint32_t* __restrict__ used_out, uint32_t nstreams)
{
    __shared__ uint32_t s_ave[64], s_h[64], s_st[kEnergyWords + 2];
    const uint32_t f = blockIdx.x;
    if (f >= nstreams) return;
    const int lane = threadIdx.x;
    const uint32_t nb = n[f];
    if (lane < kEnergyWords) s_st[lane] = lane == 9 ? state[kEnergyWords * f + lane] & 7u : state[kEnergyWords * f + lane];
    if (lane == 0) { s_st[kEnergyWords] = 0; s_st[kEnergyWords + 1] = 0; }       // bursts used, done
    wave_lds_sync();
    for (uint32_t b0 = 0; b0 < nb && !s_st[kEnergyWords + 1]; b0 += 64) {
        if (b0 + lane < nb) {
            const uint32_t* v = in + (size_t)first[f] + 4 * (size_t)(b0 + lane);
            const cpx x[4] = { unpack(v[0]), unpack(v[1]), unpack(v[2]), unpack(v[3]) };
            int ave = 0; cpx h = mk(0, 0);
#pragma unroll
            for (int k = 0; k < 4; k++) { ave = wadd32(ave, sqnorm(x[k]) >> 5); h = cadd16(h, sra(x[k], 5)); }
            s_ave[lane] = (uint32_t)ave; s_h[lane] = pack(h);
        }
        wave_lds_sync();
        if (lane == 0) {
            // words: 0 average_energy, 1..8 window, 9 idx, 10 count, 11 power_detected, 12 error_code, 13 cca_pwr_threshold, 14 update_cnt, 15 sum_dc, 16 dc
            uint32_t used = s_st[kEnergyWords];
            const uint32_t end = min(nb, b0 + 64u);
            while (used < end && !s_st[11] && s_st[12] == 0) {
                const uint32_t ave = s_ave[used - b0]; const cpx h = unpack(s_h[used - b0]);
                used++;
                s_st[0] = s_st[0] - s_st[1 + s_st[9]] + ave;
                s_st[1 + s_st[9]] = ave;
                if (++s_st[9] >= 8) s_st[9] = 0;
                s_st[10]++;
                if (s_st[10] >= 32) {
                    if (s_st[10] >= 100) { s_st[12] = E_CS_TIMEOUT; continue; }
                    if (s_st[0] >= s_st[13]) s_st[11] = 1;
                }
                if (!s_st[11]) {                                                 // energy gating: only low-power bursts reach the DC estimator
                    cpx sum = cadd16(unpack(s_st[15]), h);
                    if (s_st[14] == 0) { s_st[16] = pack(cadd16(unpack(s_st[16]), sra(sum, 2))); s_st[14] = 8; sum = mk(0, 0); }
                    s_st[15] = pack(sum);
                    s_st[14]--;
                }
            }
            s_st[kEnergyWords] = used;
            s_st[kEnergyWords + 1] = (s_st[11] || s_st[12] != 0) ? 1u : 0u;
        }
        wave_lds_sync();
    }
    if (lane < kEnergyWords) state[kEnergyWords * f + lane] = s_st[lane];
    if (lane == kEnergyWords) used_out[f] = s_st[kEnergyWords];
}

// ---- TBarkerSync: one wave per stream; the lanes bring the chips >> 4, lane 0 runs the correlator's shift register and the peak search.  state: sora_barker11b_state, 15
// words = sync_flag, last_peak_cnt, m_max, search_count, partial[10], error_code.
constexpr int kBarkerWords = 15;
__global__ void __launch_bounds__(64) k_11b_barker_sync(const uint32_t* __restrict__ in, const uint32_t* __restrict__ first, const uint32_t* __restrict__ n, uint32_t* __restrict__ state,
        uint32_t* __restrict__ used_out, uint32_t nstreams)
{
    __shared__ uint32_t s_ss[64], s_st[kBarkerWords + 2];
    const uint32_t f = blockIdx.x;
    if (f >= nstreams) return;
    const int lane = threadIdx.x;
    const uint32_t nc = n[f];
    if (lane < kBarkerWords) s_st[lane] = state[kBarkerWords * f + lane];
    if (lane == 0) { s_st[kBarkerWords] = 0; s_st[kBarkerWords + 1] = 0; }
    wave_lds_sync();
    for (uint32_t c0 = 0; c0 < nc && !s_st[kBarkerWords + 1]; c0 += 64) {
        if (c0 + lane < nc) s_ss[lane] = pack(sra(unpack(in[(size_t)first[f] + c0 + lane]), 4));
        wave_lds_sync();
        if (lane == 0) {
            int flag = (int)s_st[0], peak = (int)s_st[1], mmax = (int)s_st[2], search = (int)s_st[3];
            uint32_t err = s_st[14], used = s_st[kBarkerWords];
            cpx p[10];
#pragma unroll
            for (int k = 0; k < 10; k++) p[k] = unpack(s_st[4 + k]);
            const uint32_t end = min(nc, c0 + 64u);
            while (used < end && flag != k11bBarkerSynced && err == 0) {
                const cpx ss = unpack(s_ss[used - c0]);
                used++;
                search++;
                if (search >= 11 * 4) { err = E_SYNC_TIMEOUT; break; }
                const cpx o = b11_barker_shift(ss, [&](int k) { return p[k]; }, [&](int k, cpx v) { p[k] = v; });
                b11_barker_peak(sqnorm(o), flag, peak, mmax);
            }
            s_st[0] = (uint32_t)flag; s_st[1] = (uint32_t)peak; s_st[2] = (uint32_t)mmax; s_st[3] = (uint32_t)search; s_st[14] = err;
#pragma unroll
            for (int k = 0; k < 10; k++) s_st[4 + k] = pack(p[k]);
            s_st[kBarkerWords] = used;
            s_st[kBarkerWords + 1] = (flag == k11bBarkerSynced || err != 0) ? 1u : 0u;
        }
        wave_lds_sync();
    }
    if (lane < kBarkerWords) state[kBarkerWords * f + lane] = s_st[lane];
    if (lane == kBarkerWords) used_out[f] = s_st[kBarkerWords];
}

// ---- TSFDSync (mode 1: with the short preamble's rule, sora_rx11b_set_preamble): one wave per stream; lane l brings the differential bit of symbol l against the symbol
// before it, lane 0 descrambles, shifts the 16-bit window and decides.  state: sora_sfd11b_state, 9 words = last_symbol, byte_reg, bit_one_found, bit_zero_found, word,
// bit_err_cnt, sync_cnt, rxrate_state, error_code.
constexpr int kSfdWords = 9;
__global__ void __launch_bounds__(64) k_11b_sfd_sync(const uint32_t* __restrict__ in, const uint32_t* __restrict__ first, const uint32_t* __restrict__ n, uint32_t* __restrict__ state,
        uint32_t* __restrict__ used_out, uint32_t nstreams, int mode)
{
    __shared__ uint32_t s_bit[64], s_st[kSfdWords + 2];
    const uint32_t f = blockIdx.x;
    if (f >= nstreams) return;
    const int lane = threadIdx.x;
    const uint32_t ns = n[f];
    const uint32_t* src = in + first[f];
    if (lane < kSfdWords) s_st[lane] = state[kSfdWords * f + lane];
    if (lane == 0) { s_st[kSfdWords] = 0; s_st[kSfdWords + 1] = 0; }
    wave_lds_sync();
    const uint32_t last0 = s_st[0];
    for (uint32_t i0 = 0; i0 < ns && !s_st[kSfdWords + 1]; i0 += 64) {
        const uint32_t i = i0 + lane;
        if (i < ns) s_bit[lane] = b11_dot_sign(unpack(i == 0 ? last0 : src[i - 1]), unpack(src[i]));
        wave_lds_sync();
        if (lane == 0) {
            uint32_t reg = s_st[1], one = s_st[2], zero = s_st[3], word = s_st[4], errs = s_st[5], cnt = s_st[6], rate = s_st[7], err = s_st[8], used = s_st[kSfdWords];
            const uint32_t end = min(ns, i0 + 64u);
            while (used < end && rate == k11bRateSync && err == 0) {
                const uint32_t bit = s_bit[used - i0];
                used++;
                reg &= 0x7Fu;
                const uint32_t sbit = (bit ^ reg ^ (reg >> 3)) & 1u;
                reg = (reg >> 1) | (bit << 6);
                word = ((word >> 1) | (sbit << 15)) & 0xFFFFu;
                cnt++;
                if (!one && !zero) {
                    if (word == 0xFFFFu) one = 1;
                    else if (mode >= 1 && word == 0 && cnt >= 16) zero = 1;
                } else if (one) {
                    if (word == 0xF3A0u) rate = k11bRate1M;
                    else if (word != 0xFFFFu) { if (errs++ > 32) { err = E_SFD_FAIL; continue; } }
                } else {
                    if (word == 0x05CFu) rate = k11bRate2M;
                    else if (word != 0) { if (errs++ > 32) { err = E_SFD_FAIL; continue; } }
                }
                if (cnt > 128 + 16) err = E_SFD_TIMEOUT;
            }
            if (used > 0) s_st[0] = src[used - 1];
            s_st[1] = reg; s_st[2] = one; s_st[3] = zero; s_st[4] = word; s_st[5] = errs; s_st[6] = cnt; s_st[7] = rate; s_st[8] = err;
            s_st[kSfdWords] = used;
            s_st[kSfdWords + 1] = (rate != k11bRateSync || err != 0) ? 1u : 0u;
        }
        wave_lds_sync();
    }
    if (lane < kSfdWords) state[kSfdWords * f + lane] = s_st[lane];
    if (lane == kSfdWords) used_out[f] = s_st[kSfdWords];
}

// ---- TBB11bPlcpParser: a thread per header.  rec = error_code, data_rate_kbps, frame_length, rxrate_state; a failed CRC-16 leaves the other three 0.
__global__ void __launch_bounds__(256) k_11b_plcp_parse(const uint8_t* __restrict__ hdr, uint32_t* __restrict__ rec, uint32_t nstreams)
{
    const uint32_t f = blockIdx.x * 256u + threadIdx.x;
    if (f >= nstreams) return;
    uint32_t h[6];
#pragma unroll
    for (int k = 0; k < 6; k++) h[k] = hdr[(size_t)6 * f + k];
    uint4 r = uint4{ E_PLCP_HEADER_FAIL, 0u, 0u, 0u };
    if (b11_crc16(h) == (h[4] | (h[5] << 8))) {
        const B11Plcp p = b11_plcp_fields(h[0], h[1], h[2] | (h[3] << 8), k11bRateSync);
        r = uint4{ 0u, p.kbps, p.len, (uint32_t)p.rate };
    }
    reinterpret_cast<uint4*>(rec)[f] = r;
}

// ---- TBB11bFrameSink: one wave per frame; the CRC-32 table in LDS, lane 0 runs the register over bytes 0 .. len - 5 and compares with bytes len - 4 .. len - 2 (the sink
// decides with three FCS bytes in hand: byte len - 1 is never read).  Bytes from index 4096 on are behind the sink's buffer: they count for the CRC but read back as 0.
__global__ void __launch_bounds__(64) k_11b_frame_sink(const uint8_t* __restrict__ bytes, const uint32_t* __restrict__ first, const uint32_t* __restrict__ len_tab, uint32_t* __restrict__ rec,
        uint32_t nstreams, const uint32_t* __restrict__ crc_tab)
{
    __shared__ uint32_t s_crc[256];
    const uint32_t f = blockIdx.x;
    if (f >= nstreams) return;
    const int lane = threadIdx.x;
    for (int k = lane; k < 256; k += 64) s_crc[k] = crc_tab[k];
    wave_lds_sync();
    if (lane != 0) return;
    const uint32_t len = len_tab[f] & 0xFFFFu;
    uint32_t err = 0, p = 0;
    if (len >= 4) {
        const uint8_t* src = bytes + first[f];
        uint32_t c = 0xFFFFFFFFu;
        for (uint32_t i = 0; i + 4 < len; i++) c = s_crc[(c ^ src[i]) & 0xFFu] ^ (c >> 8);
        for (uint32_t k = 0; k < 3; k++) { const uint32_t i = len - 4 + k; if (i < 4096u) p |= (uint32_t)src[i] << (8 * k); }
        err = b11_fcs_verdict(c, p);
    }
    reinterpret_cast<uint2*>(rec)[f] = uint2{ err, p };
}

}  // namespace sora

using namespace sora;

// ---- the stage entry points (host_stage.h: the prologue and helpers every stage shares)
static_assert(sizeof(sora_stream11b_state) == 16 && sizeof(sora_energy11b_state) == 68 && sizeof(sora_symtiming11b_state) == 8 && sizeof(sora_barker11b_state) == 60 &&
              sizeof(sora_sfd11b_state) == 36 && sizeof(sora_plcp11b_rec) == 16 && sizeof(sora_sink11b_rec) == 8, "the 802.11b stage records are 32-bit words");

int sora_hip_dc_remove11b(const sora_complex16* d_in, const uint32_t* d_first, const uint32_t* d_n, const uint32_t* d_out_first, const sora_complex16* d_dc,
                          sora_complex16* d_out, size_t nstreams, size_t max_n, void* stream)
{
    STAGE_ENTRY("sora_hip_dc_remove11b", !d_in || !d_first || !d_n || !d_out_first || !d_dc || !d_out, nstreams)
    if (max_n == 0) return SORA_OK;
    uint32_t chunks; unsigned grid;
    if (max_n >= (1u << 29) || !stage_grid(nstreams, 4 * max_n, &chunks, &grid))
        return sora_internal_fail(SORA_ERR_CAPACITY, "sora_hip_dc_remove11b: nstreams x max_n is too large for one call", 0);
    hipLaunchKernelGGL(k_11b_dc_remove, dim3(grid), dim3(256), 0, (hipStream_t)stream, u32(d_in), u32(d_out), d_first, d_n, d_out_first, u32(d_dc), (uint32_t)nstreams, chunks);
    return launch_result("k_11b_dc_remove");
}

int sora_hip_energy_detect11b(const sora_complex16* d_in, const uint32_t* d_first, const uint32_t* d_n, sora_energy11b_state* d_state, uint32_t* d_used,
                              size_t nstreams, size_t max_n, void* stream)
{
    (void)max_n;                                                                 // (a wave per stream walks its own d_n[f])
    STAGE_ENTRY("sora_hip_energy_detect11b", !d_in || !d_first || !d_n || !d_state || !d_used, nstreams)
    hipLaunchKernelGGL(k_11b_energy_detect, dim3((unsigned)nstreams), dim3(64), 0, (hipStream_t)stream, u32(d_in), d_first, d_n, u32(d_state), d_used, (uint32_t)nstreams);
    return launch_result("k_11b_energy_detect");
}

int sora_hip_symtiming11b(const sora_complex16* d_in, const uint32_t* d_first, const uint32_t* d_n, const uint32_t* d_out_first, sora_symtiming11b_state* d_state,
                          sora_complex16* d_out, uint32_t* d_nchips, size_t nstreams, size_t max_n, void* stream)
{
    (void)max_n;
    STAGE_ENTRY("sora_hip_symtiming11b", !d_in || !d_first || !d_n || !d_out_first || !d_state || !d_out || !d_nchips, nstreams)
    hipLaunchKernelGGL(k_11b_symtiming, dim3((unsigned)nstreams), dim3(64), 0, (hipStream_t)stream, u32(d_in), u32(d_out), d_first, d_n, d_out_first,
                       reinterpret_cast<int*>(d_state), d_nchips, (uint32_t)nstreams);
    return launch_result("k_11b_symtiming");
}

int sora_hip_barker_sync11b(const sora_complex16* d_in, const uint32_t* d_first, const uint32_t* d_n, sora_barker11b_state* d_state, uint32_t* d_used,
                            size_t nstreams, size_t max_n, void* stream)
{
    (void)max_n;
    STAGE_ENTRY("sora_hip_barker_sync11b", !d_in || !d_first || !d_n || !d_state || !d_used, nstreams)
    hipLaunchKernelGGL(k_11b_barker_sync, dim3((unsigned)nstreams), dim3(64), 0, (hipStream_t)stream, u32(d_in), d_first, d_n, u32(d_state), d_used, (uint32_t)nstreams);
    return launch_result("k_11b_barker_sync");
}

int sora_hip_despread11b(const sora_complex16* d_in, const uint32_t* d_first, const uint32_t* d_n, const uint32_t* d_out_first, sora_complex16* d_out,
                         size_t nstreams, size_t max_n, void* stream)
{
    STAGE_ENTRY("sora_hip_despread11b", !d_in || !d_first || !d_n || !d_out_first || !d_out, nstreams)
    if (max_n == 0) return SORA_OK;
    uint32_t chunks; unsigned grid;
    if (!stage_grid(nstreams, max_n, &chunks, &grid)) return sora_internal_fail(SORA_ERR_CAPACITY, "sora_hip_despread11b: nstreams x max_n is too large for one call", 0);
    hipLaunchKernelGGL(k_11b_despread, dim3(grid), dim3(256), 0, (hipStream_t)stream, u32(d_in), u32(d_out), d_first, d_n, d_out_first, (uint32_t)nstreams, chunks);
    return launch_result("k_11b_despread");
}

int sora_hip_sfd_sync11b(const sora_complex16* d_in, const uint32_t* d_first, const uint32_t* d_n, sora_sfd11b_state* d_state, uint32_t* d_used,
                         size_t nstreams, size_t max_n, int mode, void* stream)
{
    (void)max_n;
    STAGE_ENTRY("sora_hip_sfd_sync11b", !d_in || !d_first || !d_n || !d_state || !d_used, nstreams)
    if (mode != 0 && mode != 1) return sora_internal_fail(SORA_ERR_INVALID_PARAM, "sora_hip_sfd_sync11b: mode must be 0 or 1", 0);
    hipLaunchKernelGGL(k_11b_sfd_sync, dim3((unsigned)nstreams), dim3(64), 0, (hipStream_t)stream, u32(d_in), d_first, d_n, u32(d_state), d_used, (uint32_t)nstreams, mode);
    return launch_result("k_11b_sfd_sync");
}

// the five position-parallel stream stages with a sora_stream11b_state, behind their entry's prologue: the stage's kernel, then the state behind it (kind: k_11b_stream_state)
static int stream11b_stage(int kind, const char* too_large, const void* d_in, const uint32_t* d_first, const uint32_t* d_n, const uint32_t* d_out_first, sora_stream11b_state* d_state,
                           uint8_t* d_out, size_t nstreams, size_t max_n, void* stream)
{
    if (max_n == 0) return SORA_OK;
    uint32_t chunks; unsigned grid;
    if (!stage_grid(nstreams, max_n, &chunks, &grid)) return sora_internal_fail(SORA_ERR_CAPACITY, too_large, 0);
    hipStream_t st = (hipStream_t)stream; const uint32_t ns = (uint32_t)nstreams; uint32_t* state = u32(d_state);
    switch (kind) {
    case 0: hipLaunchKernelGGL(k_11b_demap<1>, dim3(grid), dim3(256), 0, st, u32(d_in), d_out, d_first, d_n, d_out_first, state, ns, chunks); break;
    case 1: hipLaunchKernelGGL(k_11b_demap<2>, dim3(grid), dim3(256), 0, st, u32(d_in), d_out, d_first, d_n, d_out_first, state, ns, chunks); break;
    case 2: hipLaunchKernelGGL(k_11b_cck<5>, dim3(grid), dim3(256), 0, st, u32(d_in), d_out, d_first, d_n, d_out_first, state, ns, chunks); break;
    case 3: hipLaunchKernelGGL(k_11b_cck<11>, dim3(grid), dim3(256), 0, st, u32(d_in), d_out, d_first, d_n, d_out_first, state, ns, chunks); break;
    default: hipLaunchKernelGGL(k_11b_desc741, dim3(grid), dim3(256), 0, st, static_cast<const uint8_t*>(d_in), d_out, d_first, d_n, d_out_first, state, ns, chunks); break;
    }
    static const char* const kernel[5] = { "k_11b_demap<1>", "k_11b_demap<2>", "k_11b_cck<5>", "k_11b_cck<11>", "k_11b_desc741" };
    if (const int rc = launch_result(kernel[kind])) return rc;
    hipLaunchKernelGGL(k_11b_stream_state, dim3((ns + 255) / 256), dim3(256), 0, st, d_in, d_first, d_n, state, ns, kind);
    return launch_result("k_11b_stream_state");
}
#define STREAM11B(name, kind, in_t) \
    int name(const in_t* d_in, const uint32_t* d_first, const uint32_t* d_n, const uint32_t* d_out_first, sora_stream11b_state* d_state, uint8_t* d_out, size_t nstreams, \
             size_t max_n, void* stream) \
    { \
        STAGE_ENTRY(#name, !d_in || !d_first || !d_n || !d_out_first || !d_state || !d_out, nstreams) \
        return stream11b_stage(kind, #name ": nstreams x max_n is too large for one call", d_in, d_first, d_n, d_out_first, d_state, d_out, nstreams, max_n, stream); \
    }
STREAM11B(sora_hip_dbpsk_demap11b, 0, sora_complex16)
STREAM11B(sora_hip_dqpsk_demap11b, 1, sora_complex16)
STREAM11B(sora_hip_cck5p5_decode11b, 2, sora_complex16)
STREAM11B(sora_hip_cck11_decode11b, 3, sora_complex16)
STREAM11B(sora_hip_desc741_11b, 4, uint8_t)
#undef STREAM11B

int sora_hip_plcp_parse11b(const uint8_t* d_hdr, sora_plcp11b_rec* d_rec, size_t nstreams, void* stream)
{
    STAGE_ENTRY("sora_hip_plcp_parse11b", !d_hdr || !d_rec, nstreams)
    if (!aligned16(d_rec)) return sora_internal_fail(SORA_ERR_INVALID_PARAM, "sora_hip_plcp_parse11b: the records must be 16-byte aligned", 0);
    hipLaunchKernelGGL(k_11b_plcp_parse, dim3((unsigned)((nstreams + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d_hdr, u32(d_rec), (uint32_t)nstreams);
    return launch_result("k_11b_plcp_parse");
}

int sora_hip_frame_sink11b(const uint8_t* d_bytes, const uint32_t* d_first, const uint32_t* d_len, sora_sink11b_rec* d_rec, size_t nstreams, void* stream)
{
    STAGE_ENTRY("sora_hip_frame_sink11b", !d_bytes || !d_first || !d_len || !d_rec, nstreams)
    if ((uintptr_t)d_rec & 7) return sora_internal_fail(SORA_ERR_INVALID_PARAM, "sora_hip_frame_sink11b: the records must be 8-byte aligned", 0);
    Tables T; if (const int rc = stage_tables(&T)) return rc;
    hipLaunchKernelGGL(k_11b_frame_sink, dim3((unsigned)nstreams), dim3(64), 0, (hipStream_t)stream, d_bytes, d_first, d_len, u32(d_rec), (uint32_t)nstreams, T.crc);
    return launch_result("k_11b_frame_sink");
}
