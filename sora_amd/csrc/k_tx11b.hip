// k_tx11b.hip -- 802.11b transmitter on the GPU (1, 2, 5.5 and 11 Mbps; long or short preamble): the reference's modulation graph
//   TBB11bSrc -> TSc741 -> TBB11bMRSelect -> TBB11bDBPSKSpread / TBB11bDQPSKSpread / TCCK5Encode / TCCK11Encode
//   -> TQuickPulseShaper -> TPackSample16to8 -> TModSink                (kernel/bb/demod11/fb11bmod_config.hpp:28-50)
// Output: COMPLEX8 at 44 MHz (11 Mchip/s, four samples a chip).  Every stage restated so that it is data-parallel:
//   * PPDU (PHY_11b.hpp:80-200): 16 x 0xFF, SFD 0xF3A0, SIGNAL, SERVICE, LENGTH (us), CRC-16, MPDU, FCS.  The short preamble, which
//     TBB11bSrc::PreparePLCPHeader refuses (PHY_11b.hpp:115-119) and TBB11bMRSelect already counts (:224-229): 7 x 0x00, SFD 0x05CF, the
//     six PLCP bytes at 2 Mbps DQPSK, scrambler register 0x1B; the differential phase runs on from SFD to header to payload.  The
//     header's geometry comes from tx11b_plan (kernels.h), for both kinds
//   * scrambler (scramble.hpp:7-88): s[n] = b[n] ^ s[n-4] ^ s[n-7] from the register 0x6C.  Linear over GF(2) with a 7-bit state:
//     each lane scrambles a run of bytes, and a scan composes the runs (the state after e zero-input steps is M^e s, e mod 127)
//   * every chip is 1, j, -1 or -j: an angle a in quarter turns.  The differential phase is a sum mod 4 of per-byte increments
//     (a second scan); the reference's encoding of last_phase (0: 0, 1: -pi/2, 2: pi/2, 3: pi) only enters at the two ends
//   * spreading: a Barker symbol at phase p has chips p ^ (2 x Barker sign), 11 two-bit fields of one word; a CCK symbol has
//     the chips p + (phi2 + phi3 + phi4, phi3 + phi4, phi2 + phi4, phi4 + 2, phi2 + phi3, phi3, phi2 + 2, 0) (IEEE 802.11-2016 16.3.6.6)
//   * shaper: output sample s of chip step m is sum_j x[m - j] tap(8 - 4 j - s), j = 0..4 (pulse.hpp:254-340), so the four samples
//     of a chip step are a function of five chip angles: a 1024-entry table in LDS, built per workgroup from the 20 taps
// Decomposition: a grid of nframes x G workgroups; workgroup (f, g) writes the g-th of G runs of frame f's chips, cut at byte
// boundaries.  It scans the frame's bytes up to the end of its run (at most 4120, 17 per lane), then writes its run tile by
// tile: the symbol words of a tile into LDS, then one 16-byte store (two chip steps, eight samples) per lane and pass.
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "dev_tx.h"

namespace sora {

namespace {
constexpr int kThreads = 256;
constexpr uint32_t kMaxBytes = 24 + 4092 + 4;               // header + MPDU + FCS
constexpr uint32_t kTileChunks = 4096;                      // chip-step pairs per tile: 8196 chips with the window, <= 1026 symbols of 8 chips
constexpr uint32_t kTileSyms = 1032;
// TQuickPulseShaper's taps (pulse.hpp:254-293): tap(i) = (short)(x * 80 + .5), x = 4 cos(PI i / 2) / PI / (1 - i^2) (1 at i = +-1),
// PI = 3.141593, for i = 8, 7, .., -11.  Output sample s of chip step m takes x[m - j] times kTx11bTaps[4 j + s], j = 0..4.
constexpr int kTx11bTaps[20] = { -1, 0, 3, 0, -6, 0, 34, 80, 102, 80, 34, 0, -6, 0, 3, 0, -1, 0, 1, 0 };
constexpr uint32_t kBarker22 = 0x2A0208u;                   // Barker 1,-1,1,1,-1,1,1,1,-1,-1,-1: chip k's field is 2 where the sign is -1
constexpr uint32_t kRep11 = 0x155555u;                      // 1 in each of 11 two-bit fields
// quarter turns of a DQPSK dibit (d0 + 2 d1): 00 -> 0, 10 -> pi/2 clockwise, 01 -> pi/2, 11 -> pi (DQPSKEncode order 1, -j, j, -1)
__device__ __forceinline__ uint32_t dq(uint32_t d) { return (0x9Cu >> (2 * d)) & 3u; }
// quarter turns of a CCK phi2..phi4 dibit at 11 Mbps (d0 + 2 d1): 1, -1, j, -j
__device__ __forceinline__ uint32_t cq(uint32_t d) { return (0xD8u >> (2 * d)) & 3u; }
// last_phase code <-> quarter turns
__device__ __forceinline__ uint32_t code_of_angle(uint32_t a) { return (0x78u >> (2 * a)) & 3u; }

// the zero-input scrambler step s -> M s, and M^e for e = 0..126 on the seven basis vectors (the register cycles with period 127)
struct ScrPow { uint8_t c[127][7]; };
constexpr ScrPow make_scr_pow()
{
    ScrPow P{};
    for (int i = 0; i < 7; i++) {
        uint32_t s = 1u << i;
        for (int e = 0; e < 127; e++) { P.c[e][i] = (uint8_t)s; s = (s >> 1) | (((s ^ (s >> 3)) & 1u) << 6); }
    }
    return P;
}
__device__ __constant__ ScrPow kScrPow = make_scr_pow();
__device__ __forceinline__ uint32_t scr_adv(uint32_t s, uint32_t e)
{
    uint32_t r = 0;
#pragma unroll
    for (int i = 0; i < 7; i++) r ^= ((s >> i) & 1u) ? (uint32_t)kScrPow.c[e][i] : 0u;
    return r;
}
// TSc741 on one byte, four bits at a time (the shortest feedback is four bits back).  r: the last seven output bits, oldest in bit 0.
__device__ __forceinline__ uint32_t scramble8(uint32_t x, uint32_t& r)
{
    const uint32_t lo = (x ^ r ^ (r >> 3)) & 15u;
    r = (r >> 4) | (lo << 3);
    const uint32_t hi = ((x >> 4) ^ r ^ (r >> 3)) & 15u;
    r = (r >> 4) | (hi << 3);
    return lo | (hi << 4);
}

// four samples of one chip step from the angles of chips m-4..m (w: two bits each, chip m-4 lowest) of which `valid` exist
__device__ __forceinline__ uint2 shape4(uint32_t w, uint32_t valid)
{
    int re[4] = { 0, 0, 0, 0 }, im[4] = { 0, 0, 0, 0 };
#pragma unroll
    for (int p = 0; p < 5; p++) {
        const uint32_t a = (w >> (2 * p)) & 3u;
        const int c = ((valid >> p) & 1u) == 0 ? 0 : a == 0 ? 1 : a == 2 ? -1 : 0;
        const int s = ((valid >> p) & 1u) == 0 ? 0 : a == 1 ? 1 : a == 3 ? -1 : 0;
#pragma unroll
        for (int k = 0; k < 4; k++) { re[k] += c * kTx11bTaps[4 * (4 - p) + k]; im[k] += s * kTx11bTaps[4 * (4 - p) + k]; }
    }
    uint32_t h[4];
#pragma unroll
    for (int k = 0; k < 4; k++)                                                  // TPackSample16to8: saturating pack, no shift
        h[k] = ((uint32_t)min(max(re[k], -128), 127) & 0xFFu) | (((uint32_t)min(max(im[k], -128), 127) & 0xFFu) << 8);
    return make_uint2(h[0] | (h[1] << 16), h[2] | (h[3] << 16));
}
}  // namespace

__global__ void __launch_bounds__(kThreads) k_tx11b(Tx11bArgs A)
{
    __shared__ uint2 s_lut[1024];
    __shared__ uint32_t s_sym[kTileSyms];
    __shared__ alignas(16) uint8_t s_byte[kMaxBytes + 8];     // PPDU bytes, scrambled in place
    __shared__ uint8_t s_ph[kMaxBytes + 8];                   // quarter turns before each byte
    __shared__ uint32_t s_scan[kThreads];
    __shared__ uint32_t s_crc[256];
    __shared__ uint32_t s_z[6 * 8 * 16];
    __shared__ uint32_t s_crcw[2];
    const uint32_t f = blockIdx.x, g = blockIdx.y, G = gridDim.y;
    const int tid = threadIdx.x;
    const uint32_t L = A.len[f];
    Tx11bPlan P;
    // (a byte load goes through the vector unit: said to be wave-uniform, the kind and the whole plan derived from it stay in scalar registers)
    const uint32_t kind = A.preamble ? (uint32_t)__builtin_amdgcn_readfirstlane((int)A.preamble[f]) : 0u;
    if (!tx11b_plan(L, A.rate[f], P, kind)) return;                              // an unsupported frame: nothing is written
    const uint32_t H1 = P.hb1, HB = P.hb, HS = P.hsyms, HC = P.hchips;          // header: DBPSK bytes, bytes, symbols, chips
    // PPDU byte b lives at s_byte[24 - HB + b]: MPDU and FCS start at s_byte + 24 for either kind (a fixed, aligned place for the FCS waves' reads)
    uint8_t* const ppdu = s_byte + (24 - HB);
    const uint32_t M = L + HB + 4, N = P.nchips, Q = (N + 6) / 2;                    // bytes, chips, 16-byte chunks (two chip steps each)
    auto chip_of_byte = [&](uint32_t b) { return b < H1 ? 88 * b : b < HB ? 88 * H1 + 44 * (b - H1) : HC + (b - HB) * P.cpb; };
    auto byte_ceil = [&](uint32_t c) { return c <= 88 * H1 ? (c + 87) / 88 : c <= HC ? H1 + (c - 88 * H1 + 43) / 44 : HB + (c - HC + P.cpb - 1) / P.cpb; };
    const uint32_t B0 = byte_ceil((uint32_t)((uint64_t)N * g / G)), B1 = byte_ceil((uint32_t)((uint64_t)N * (g + 1) / G));
    if (B0 >= B1) return;                                                        // (more runs than bytes)
    const uint32_t q0 = chip_of_byte(B0) / 2, q1 = B1 == M ? Q : chip_of_byte(B1) / 2;

    // the shaper table: chip angles a0..a4 (chips m-4..m) -> four samples
    for (int i = tid; i < 1024; i += kThreads) s_lut[i] = shape4((uint32_t)i, 31u);
    // PPDU bytes [0, B1)
    if (tid == 0) {
        const uint32_t size = L + 4;
        uint32_t us, ext = 0;
        if (P.cpb == 88) us = size * 8;
        else if (P.cpb == 44) us = size * 4;
        else if (P.cpb == 16) us = (size * 16 + 10) / 11;
        else { us = (size * 8 + 10) / 11; ext = us * 11 - size * 8 >= 8 ? 1u : 0u; }
        uint8_t h[8] = { (uint8_t)P.sfd, (uint8_t)(P.sfd >> 8), (uint8_t)P.code, (uint8_t)(ext << 7), (uint8_t)us, (uint8_t)(us >> 8), 0, 0 };
        uint32_t c = 0xFFFFu;                                                    // CRC-16 of SIGNAL..LENGTH: reflected 0x8408, init 0xFFFF, inverted
        for (int i = 2; i < 6; i++) {
            c ^= h[i];
            for (int k = 0; k < 8; k++) c = (c & 1u) ? (c >> 1) ^ 0x8408u : c >> 1;
        }
        c = ~c & 0xFFFFu;
        h[6] = (uint8_t)c; h[7] = (uint8_t)(c >> 8);
        for (uint32_t i = 0; i + 8 < HB; i++) ppdu[i] = (uint8_t)P.sync;
        for (uint32_t i = 0; i < 8; i++) s_byte[16 + i] = h[i];
    }
    const uint8_t* mp = A.mpdu + A.off[f];
    const uint32_t nm = min(B1, HB + L) > HB ? min(B1, HB + L) - HB : 0u;
    for (uint32_t i = tid; i < nm; i += kThreads) s_byte[24 + i] = mp[i];
    const bool need_fcs = B1 > HB + L;
    if (need_fcs) {
        s_crc[tid] = A.T.crc[tid];
        for (int i = tid; i < 6 * 8 * 16; i += kThreads) s_z[i] = A.T.crcz[i];
    }
    __syncthreads();
    if (need_fcs) {                                                              // FCS = CalcCRC32 of the MPDU, little-endian
        if (tid < 128) tx_fcs_waves<2>(s_byte + 24, L, s_crc, s_z, tid, s_crcw);   // two waves (dev_tx.h)
        __syncthreads();
        if (tid == 0) {
            const uint32_t fcs = tx_fcs_join<2>(s_z, s_crcw);                    // a run that ends inside the FCS stores only its bytes
            for (uint32_t k = 0; k < 4 && HB + L + k < B1; k++) s_byte[24 + L + k] = (uint8_t)(fcs >> (8 * k));
        }
        __syncthreads();
    }

    // scrambler: lane t takes bytes [t K, t K + K).  Pass 1 from state 0 (lane 0: the seed), then an inclusive scan of
    // y_t = M^(8 K) y_(t-1) ^ e_t, then pass 2 from the true entry state.
    const uint32_t K = (B1 + kThreads - 1) / kThreads;
    const uint32_t blo = min((uint32_t)tid * K, B1), bhi = min(blo + K, B1);
    uint32_t r = tid == 0 ? P.seed : 0u;                                        // DOT11B_PLCP_{LONG,SHORT}_TX_SCRAMBLER_REGISTER
    for (uint32_t b = blo; b < bhi; b++) (void)scramble8(ppdu[b], r);
    uint32_t y = r;
    const uint32_t e8k = (8 * K) % 127;
    for (uint32_t d = 1; d < (uint32_t)kThreads; d <<= 1) {
        s_scan[tid] = y;
        __syncthreads();
        if ((uint32_t)tid >= d) y ^= scr_adv(s_scan[tid - d], (e8k * d) % 127);
        __syncthreads();
    }
    s_scan[tid] = y;
    __syncthreads();
    r = tid == 0 ? P.seed : s_scan[tid - 1];
    // pass 2 scrambles in place and sums the run's phase increments (quarter turns a byte adds to the differential phase)
    uint32_t sum = 0;
    for (uint32_t b = blo; b < bhi; b++) {
        const uint32_t v = scramble8(ppdu[b], r);
        ppdu[b] = (uint8_t)v;
        uint32_t inc;
        if (b < H1 || (b >= HB && P.cpb == 88)) inc = 2 * (__popc(v) & 1);       // DBPSK: pi per one bit
        else if (b < HB || P.cpb == 44) inc = dq(v & 3) + dq((v >> 2) & 3) + dq((v >> 4) & 3) + dq(v >> 6);
        else if (P.cpb == 16) inc = dq(v & 3) + dq((v >> 4) & 3) + 2;            // two symbols, the second one odd
        else inc = dq(v & 3) + 2 * ((b - HB) & 1);                              // odd PSDU symbols: pi more
        s_ph[b] = (uint8_t)inc;
        sum += inc;
    }
    __syncthreads();                                                             // (s_scan is read above)
    for (uint32_t d = 1; d < (uint32_t)kThreads; d <<= 1) {
        s_scan[tid] = sum;
        __syncthreads();
        if ((uint32_t)tid >= d) sum += s_scan[tid - d];
        __syncthreads();
    }
    s_scan[tid] = sum;
    __syncthreads();
    // the preamble reads only the low bit of last_phase (m_Coding_LUT[b][m_reg & 1]): the frame starts at 0 or pi
    uint32_t ph = ((A.phase_in ? A.phase_in[f] : 0u) & 1u) * 2 + (tid ? s_scan[tid - 1] : 0u);
    for (uint32_t b = blo; b < bhi; b++) {
        const uint32_t inc = s_ph[b];
        s_ph[b] = (uint8_t)(ph & 3u);
        ph += inc;
    }
    if (A.phase_out && bhi == M && blo < M) A.phase_out[f] = (uint8_t)code_of_angle(ph & 3u);

    // symbols: 0..HS-1 the header's (8 H1 DBPSK bits, then the short header's DQPSK dibits), then the data symbols
    const uint32_t nsyms = HS + (L + 4) * P.spb;
    const uint32_t spb_sh = P.spb == 8 ? 3u : P.spb == 4 ? 2u : P.spb == 2 ? 1u : 0u;
    auto sym_of_chip = [&](uint32_t c) { return c < HC ? c / 11 : HS + (P.ls == 8 ? (c - HC) >> 3 : (c - HC) / 11); };
    auto sym_start = [&](uint32_t s) { return s < HS ? 11 * s : HC + (s - HS) * P.ls; };
    auto sym_len = [&](uint32_t s) { return s < HS ? 11u : P.ls; };
    auto sym_word = [&](uint32_t s) -> uint32_t {                               // the absolute chip angles of symbol s, chip 0 lowest
        const uint32_t S1 = 8 * H1;                                              // the header's DBPSK symbols
        const uint32_t b = s < S1 ? s >> 3 : s < HS ? H1 + ((s - S1) >> 2) : HB + ((s - HS) >> spb_sh);
        const uint32_t i = s < S1 ? s & 7u : s < HS ? (s - S1) & 3u : (s - HS) & (P.spb - 1);
        const uint32_t v = ppdu[b], p = s_ph[b];
        if (s < S1 || (s >= HS && P.cpb == 88)) {                                          // DBPSK: the bits up to this one flip the phase
            const uint32_t a = (p + 2 * (__popc(v & ((2u << i) - 1u)) & 1)) & 3u;
            return kBarker22 ^ (a * kRep11);
        }
        if (s < HS || P.cpb == 44) {                                             // DQPSK: dibits 0..i
            uint32_t a = p;
            for (uint32_t k = 0; k <= i; k++) a += dq((v >> (2 * k)) & 3u);
            return kBarker22 ^ ((a & 3u) * kRep11);
        }
        uint32_t a, p2, p3, p4;
        if (P.cpb == 16) {                                                       // CCK 5.5: d0 d1 -> phi1, d2 -> phi2 = pi/2 + d2 pi, phi3 = 0, d3 -> phi4 = d3 pi
            const uint32_t nib = (v >> (4 * i)) & 15u;
            a = p + dq(v & 3u) + (i ? dq((v >> 4) & 3u) + 2 : 0u);
            p2 = 1 + 2 * ((nib >> 2) & 1u); p3 = 0; p4 = 2 * (nib >> 3);
        } else {                                                                 // CCK 11: d0 d1 -> phi1, d2..d7 -> phi2..phi4
            a = p + dq(v & 3u) + 2 * ((b - HB) & 1u);
            p2 = cq((v >> 2) & 3u); p3 = cq((v >> 4) & 3u); p4 = cq(v >> 6);
        }
        const uint32_t o[8] = { p2 + p3 + p4, p3 + p4, p2 + p4, p4 + 2, p2 + p3, p3, p2 + 2, 0 };
        uint32_t w = 0;
#pragma unroll
        for (int c = 0; c < 8; c++) w |= ((a + o[c]) & 3u) << (2 * c);
        return w;
    };

    int8_t* const base = A.out + 2 * A.out_off[f];
    const uintptr_t align = reinterpret_cast<uintptr_t>(base);
    for (uint32_t qa = q0; qa < q1; qa += kTileChunks) {
        const uint32_t qb = min(qa + kTileChunks, q1);
        const uint32_t clo = 2 * qa >= 4 ? 2 * qa - 4 : 0u, chi = min(2 * qb - 1, N - 1);
        const uint32_t sa = clo < N ? sym_of_chip(clo) : nsyms, sb = clo < N ? sym_of_chip(chi) + 1 : nsyms;
        __syncthreads();                                                         // the previous tile's readers are done (and s_ph is final)
        for (uint32_t s = sa + tid; s < sb; s += kThreads) s_sym[s - sa] = sym_word(s);
        __syncthreads();
        for (uint32_t q = qa + tid; q < qb; q += kThreads) {
            const uint32_t n = 2 * q;                                            // chip steps n, n+1: chips n-4 .. n+1
            uint2 v0, v1;
            if (n >= 4 && n + 1 < N) {
                const uint32_t c = n - 4, s0 = sym_of_chip(c), l0 = c - sym_start(s0), s1 = sym_of_chip(n + 1);
                uint32_t w = s_sym[s0 - sa] >> (2 * l0);
                if (s1 != s0) w |= s_sym[s1 - sa] << (2 * (sym_len(s0) - l0));
                v0 = s_lut[w & 0x3FFu];
                v1 = s_lut[(w >> 2) & 0x3FFu];
            } else {                                                             // the first two and the last chunks: chips outside 0..N-1 are zero
                uint32_t w = 0, valid = 0;
                for (int k = 0; k < 6; k++) {
                    const int64_t c = (int64_t)n - 4 + k;
                    if (c < 0 || c >= (int64_t)N) continue;
                    const uint32_t s = sym_of_chip((uint32_t)c);
                    w |= ((s_sym[s - sa] >> (2 * ((uint32_t)c - sym_start(s)))) & 3u) << (2 * k);
                    valid |= 1u << k;
                }
                v0 = shape4(w, valid & 31u);
                v1 = shape4(w >> 2, valid >> 1);
            }
            int8_t* o = base + 16 * (size_t)q;
            if ((align & 15u) == 0) {
                *reinterpret_cast<uint4*>(o) = make_uint4(v0.x, v0.y, v1.x, v1.y);
            } else if ((align & 1u) == 0) {                                      // (a frame placed at a sample offset that is not a multiple of eight)
                const uint32_t h[4] = { v0.x, v0.y, v1.x, v1.y };
                for (int k = 0; k < 4; k++) { reinterpret_cast<uint16_t*>(o)[2 * k] = (uint16_t)h[k]; reinterpret_cast<uint16_t*>(o)[2 * k + 1] = (uint16_t)(h[k] >> 16); }
            } else {
                const uint32_t h[4] = { v0.x, v0.y, v1.x, v1.y };
                for (int k = 0; k < 16; k++) o[k] = (int8_t)(h[k >> 2] >> (8 * (k & 3)));
            }
        }
    }
}

}  // namespace sora
