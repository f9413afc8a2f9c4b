// dev_mod11b.h -- the tables and pieces of the 802.11b modulation graph's bricks as stages (k_mod11b.hip; fb11bmod_config.hpp:28-50): TQuickPulseShaper's taps, the
// Barker word, the DQPSK / CCK quarter turns, TSc741 and its zero-input powers M^e, and the stores that move a span of a stream 16 bytes per lane.  k_tx11b.hip
// states the same constants for its fused kernel and does not include this file.
#pragma once
#include "kernels.h"

namespace sora {

constexpr int kMod11bThreads = 256;
// TQuickPulseShaper's taps (pulse.hpp:254-293): tap(i) = (short)(x * 80 + .5), x = 4 cos(PI i / 2) / PI / (1 - i^2) (1 at i = +-1), for i = 8, 7, .., -11: row j,
// column s of the brick's table is kMod11bTaps[4 j + s]
constexpr int kMod11bTaps[20] = { -1, 0, 3, 0, -6, 0, 34, 80, 102, 80, 34, 0, -6, 0, 3, 0, -1, 0, 1, 0 };
constexpr uint32_t kMod11bBarker22 = 0x2A0208u;             // Barker 1,-1,1,1,-1,1,1,1,-1,-1,-1: chip k's two-bit field is 2 (half a turn) where the sign is -1
constexpr uint32_t kMod11bRep11 = 0x155555u;                // 1 in each of 11 two-bit fields
// a chip at a quarter turns (1, j, -1, -j) as COMPLEX8: re in the low byte
__device__ __forceinline__ uint32_t mod11b_chip(uint32_t a) { return (uint32_t)(0xFF0000FF01000001ull >> (16 * (a & 3u))) & 0xFFFFu; }
// quarter turns of a DQPSK dibit d0 + 2 d1 (DQPSKEncode: 1, -j, j, -1; also CCK's phi1) and of a CCK 11 Mbps dibit (CCK11D3D2: 1, -1, j, -j)
__device__ __forceinline__ uint32_t mod11b_dq(uint32_t d) { return (0x9Cu >> (2 * d)) & 3u; }
__device__ __forceinline__ uint32_t mod11b_cq(uint32_t d) { return (0xD8u >> (2 * d)) & 3u; }
// CF_DifferentialMap::last_phase (0: 0, 1: -pi/2, 2: pi/2, 3: pi) <-> quarter turns
__device__ __forceinline__ uint32_t mod11b_code_of_turns(uint32_t a) { return (0x78u >> (2 * (a & 3u))) & 3u; }
__device__ __forceinline__ uint32_t mod11b_turns_of_code(uint32_t c) { return (0x9Cu >> (2 * (c & 3u))) & 3u; }

// ---- TSc741 (scramble.hpp:7-88): s[n] = b[n] ^ s[n-4] ^ s[n-7]; r holds the last seven output bits, oldest in bit 0.  One byte, four bits at a time (the shortest
// feedback is four bits back)
__device__ __forceinline__ uint32_t mod11b_scramble8(uint32_t x, uint32_t& r)
{
    const uint32_t lo = (x ^ r ^ (r >> 3)) & 15u;
    r = (r >> 4) | (lo << 3);
    const uint32_t hi = ((x >> 4) ^ r ^ (r >> 3)) & 15u;
    r = (r >> 4) | (hi << 3);
    return lo | (hi << 4);
}
// the zero-input step s -> M s, and M^e for e = 0..126 on the seven basis vectors (the register cycles with period 127)
struct Mod11bScrPow { uint8_t c[127][7]; };
constexpr Mod11bScrPow make_mod11b_scr_pow()
{
    Mod11bScrPow P{};
    for (int i = 0; i < 7; i++) {
        uint32_t s = 1u << i;
        for (int e = 0; e < 127; e++) { P.c[e][i] = (uint8_t)s; s = (s >> 1) | (((s ^ (s >> 3)) & 1u) << 6); }
    }
    return P;
}
static __device__ __constant__ Mod11bScrPow kMod11bScrPow = make_mod11b_scr_pow();
__device__ __forceinline__ uint32_t mod11b_scr_adv(uint32_t s, uint32_t e)
{
    uint32_t r = 0;
#pragma unroll
    for (int i = 0; i < 7; i++) r ^= ((s >> i) & 1u) ? (uint32_t)kMod11bScrPow.c[e][i] : 0u;
    return r;
}

// ---- a span of n bytes between global memory at any offset and LDS: the bytes up to the first 16-byte boundary one by one (head), then one 16-byte word per lane, then
// the bytes behind the last whole word (tail)
__device__ __forceinline__ uint32_t mod11b_head(const void* g, uint32_t n, uint32_t elem) { return min(n, (uint32_t)((16u - ((uint32_t)reinterpret_cast<uintptr_t>(g) & 15u)) & 15u) / elem); }
__device__ __forceinline__ void mod11b_load_bytes(uint8_t* s, const uint8_t* g, uint32_t n, int tid)
{
    const uint32_t head = mod11b_head(g, n, 1), nw = (n - head) / 16;
    for (uint32_t i = tid; i < head; i += kMod11bThreads) s[i] = g[i];
    for (uint32_t w = tid; w < nw; w += kMod11bThreads) {
        const uint4 v = *reinterpret_cast<const uint4*>(g + head + 16 * w);
        const uint32_t h[4] = { v.x, v.y, v.z, v.w };
#pragma unroll
        for (int k = 0; k < 16; k++) s[head + 16 * w + k] = (uint8_t)(h[k >> 2] >> (8 * (k & 3)));
    }
    for (uint32_t i = head + 16 * nw + tid; i < n; i += kMod11bThreads) s[i] = g[i];
}
__device__ __forceinline__ void mod11b_store_bytes(uint8_t* g, const uint8_t* s, uint32_t n, int tid)
{
    const uint32_t head = mod11b_head(g, n, 1), nw = (n - head) / 16;
    for (uint32_t i = tid; i < head; i += kMod11bThreads) g[i] = s[i];
    for (uint32_t w = tid; w < nw; w += kMod11bThreads) {
        const uint8_t* p = s + head + 16 * w;
        uint32_t h[4];
#pragma unroll
        for (int k = 0; k < 4; k++) h[k] = (uint32_t)p[4 * k] | ((uint32_t)p[4 * k + 1] << 8) | ((uint32_t)p[4 * k + 2] << 16) | ((uint32_t)p[4 * k + 3] << 24);
        *reinterpret_cast<uint4*>(g + head + 16 * w) = make_uint4(h[0], h[1], h[2], h[3]);
    }
    for (uint32_t i = head + 16 * nw + tid; i < n; i += kMod11bThreads) g[i] = s[i];
}

// ---- an exclusive scan of one value per lane over the workgroup's four waves (s_scan: 4 words): shuffles inside a wave, the waves' totals through LDS; every
// lane also gets the total
__device__ __forceinline__ uint32_t mod11b_scan_add(uint32_t v, uint32_t* s_scan, int tid, uint32_t& total)
{
    const int lane = tid & 63, wave = tid >> 6;
    uint32_t sum = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = (uint32_t)__shfl_up((int)sum, d);
        if (lane >= d) sum += o;
    }
    __syncthreads();                                                             // (s_scan's readers of the pass before are done)
    if (lane == 63) s_scan[wave] = sum;
    __syncthreads();
    uint32_t base = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < kMod11bThreads / 64; w++) {
        const uint32_t t = s_scan[w];
        base += w < wave ? t : 0u;
        total += t;
    }
    return base + sum - v;
}

// ---- the scrambler's scan: lane t has walked its run of `bits` bits from state 0 (the stream's first lane: from the register) and holds the state r it ended in;
// -> the state lane t's run truly starts from, y_t = M^bits y_(t-1) ^ r_t composed by shuffles inside a wave and through the waves' last states in LDS
__device__ __forceinline__ uint32_t mod11b_scan_scr(uint32_t r, uint32_t bits, uint32_t carry, uint32_t* s_scan, int tid)
{
    const int lane = tid & 63, wave = tid >> 6;
    uint32_t y = r;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = (uint32_t)__shfl_up((int)y, d);
        if (lane >= d) y ^= mod11b_scr_adv(o, (bits * d) % 127);
    }
    __syncthreads();                                                             // (s_scan's readers of the pass before are done)
    if (lane == 63) s_scan[wave] = y;
    __syncthreads();
    uint32_t e = 0;                                                              // the state the wave starts from (wave 0: lane 0 carries the register in)
    for (int w = 0; w < wave; w++) e = mod11b_scr_adv(e, (bits * 64) % 127) ^ s_scan[w];
    y ^= mod11b_scr_adv(e, (bits * (uint32_t)(lane + 1)) % 127);
    const uint32_t before = (uint32_t)__shfl_up((int)y, 1);
    return lane ? before : wave ? e : carry;
}

}  // namespace sora
