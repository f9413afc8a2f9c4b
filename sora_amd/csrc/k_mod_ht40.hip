// k_mod_ht40.hip -- the bricks of the 40 MHz HT 2x2 modulation graph (what k_tx_ht40.hip fuses: sora_hip_tx_ht40, _joint, _gi) that the 802.11a stages of k_mod.hip do
// not already serve, as stand-alone, batched stages, one C entry point each (include/sora_hip.h).  PARITY UNPINNED, as for the transmitter: the reference has no 40 MHz
// graph; every brick is defined by the project's integer model (tests/mod_ht40_model.py) and equals it and the fused kernels bit for bit.  Bits are packed in bytes, LSB
// first; N_b40 = ceil(108 N_BPSC / 8) = 14 / 27 / 54 / 81 bytes per stream and symbol, rows back to back.
//   k_mod_ht40_parse              the stream parser on 216 N_BPSC coded bits (tx_parse11n_index)          uchar x 27 N_BPSC -> 2 x uchar x N_b40
//   k_mod_ht40_interleave         the HT interleaver, N_COL 18, N_ROT 29 (deint40_index inverted)        uchar x N_b40 -> uchar x N_b40
//   k_mod_ht40_interleave_stream  the same map reading a frame's coded stream by bit address             contiguous bits -> rows of N_b40
//   k_mod_ht40_map                Gray map, odd integers x level40(N_BPSC)                               uchar x N_b40 -> COMPLEX16 x 108
//   k_mod_ht40_sig_map            L-SIG + HT-SIG with their pilots, on both halves of the channel        uchar x 18 -> COMPLEX16 x 3 x 128
//   k_mod_ht40_add_pilot          data at data_bin40(c), pilots at +-11, +-25, +-53                      COMPLEX16 x 108 -> COMPLEX16 x 128
//   k_mod_ht40_ifft               the reference's fixed-point IFFT<128>, natural order                   COMPLEX16 x 128 -> COMPLEX16 x 128
//   k_mod_ht40_add_gi             the last 32 (long) or 16 (short) samples in front                      COMPLEX16 x 128 -> COMPLEX16 x 160 / 144
//   k_mod_ht40_preamble           the fixed fields from k_tx_ht40_preamble's table                       -> 2 x COMPLEX16 x 640 / 480
// The arithmetic is dev_tx.h's and dev_ht40.h's (what k_tx_ht40 runs); here are the port formats and the streaming shape of k_mod11n.hip: a workgroup owns a tile of 32
// whole symbols (a multiple of 16 bytes whatever the row), moves it between HBM and LDS 16 bytes per lane and reshuffles inside the symbols in LDS; the guard interval,
// the preamble, the pilot stage and the SIG mapper move 16 bytes per lane per load and store.  k_tx_ht40.hip keeps its constants in its own anonymous namespace and is
// not touched: the amplitudes and the carrier rules it shares with this file are restated below, each with a pointer to the original.
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "dev_tx.h"
#include "dev_ht40.h"
#include "host_stage.h"

namespace sora {

constexpr int kModHt40Syms = 32;                                                 // symbols per workgroup tile of the byte-wide stages and the mapper
__host__ __device__ constexpr int mod_ht40_row(int nb) { return (108 * nb + 7) / 8; }   // N_b40

namespace {
constexpr int kSigAmp40 = kTxHt40Amp;       // k_tx_ht40.hip: kAmp, an L-SIG / HT-SIG carrier and their pilots
constexpr int kPilot40 = 12288;             // k_tx_ht40.hip: kPilot = 2 d(1)
__device__ __forceinline__ int level40(int nb) { return nb <= 2 ? 6144 : nb == 4 ? 4000 : 2214; }   // k_tx_ht40.hip: level40, rint(A LEVEL / 128)

// ---- nbytes contiguous bytes between global memory at ANY alignment and LDS: the LDS copy keeps the address's offset inside its 16-byte word (byte b of the run is LDS
// byte (g & 15) + b), so every 16-byte word that lies wholly inside the run moves as one load or store and the ragged ends go byte by byte.  Nothing outside the run is
// read or written.
__device__ __forceinline__ int tile_misalign(const void* g) { return (int)(reinterpret_cast<uintptr_t>(g) & 15u); }
__device__ __forceinline__ void tile_load_any(uint32_t* s, const uint8_t* g, int nbytes, int tid)
{
    const int mis = tile_misalign(g), total = mis + nbytes;
    const uint8_t* base = g - mis;
    for (int q = tid; q < (total + 15) / 16; q += 256) {
        if (16 * q >= mis && 16 * q + 16 <= total) reinterpret_cast<uint4*>(s)[q] = reinterpret_cast<const uint4*>(base)[q];
        else for (int b = max(16 * q, mis); b < min(16 * q + 16, total); b++) reinterpret_cast<uint8_t*>(s)[b] = base[b];
    }
}
__device__ __forceinline__ void tile_store_any(uint8_t* g, const uint32_t* s, int nbytes, int tid)
{
    const int mis = tile_misalign(g), total = mis + nbytes;
    uint8_t* base = g - mis;
    for (int q = tid; q < (total + 15) / 16; q += 256) {
        if (16 * q >= mis && 16 * q + 16 <= total) reinterpret_cast<uint4*>(base)[q] = reinterpret_cast<const uint4*>(s)[q];
        else for (int b = max(16 * q, mis); b < min(16 * q + 16, total); b++) base[b] = reinterpret_cast<const uint8_t*>(s)[b];
    }
}

// byte q of a tile of interleaved rows: row q / SB, positions 8 (q % SB) .. + 7; position p < NCB takes coded bit s_inv[p] of its symbol, whose bit 0 is bit
// bit0 + sym * pitch of the LDS copy (rows: pitch 8 SB; a stream: pitch NCB).  Positions at or behind NCB (BPSK's last half byte) are 0.
template <int NCB, int SB>
__device__ __forceinline__ unsigned interleave40_byte(const uint8_t* b, const uint16_t* s_inv, int q, uint32_t bit0, uint32_t pitch)
{
    const int sym = q / SB, p0 = 8 * (q - sym * SB);
    const uint32_t base = bit0 + (uint32_t)sym * pitch;
    unsigned o = 0;
#pragma unroll
    for (int t = 0; t < 8; t++) {
        if (p0 + t < NCB) { const uint32_t a = base + s_inv[p0 + t]; o |= ((b[a >> 3] >> (a & 7u)) & 1u) << t; }
    }
    return o;
}
}  // namespace

// ---- the stream parser: output bit j < 108 N_BPSC of stream s is coded bit tx_parse11n_index(S, s, j) of the symbol's 216 N_BPSC.  BPSK's 14th byte carries four bits; its
// upper half is 0 on both outputs.  A thread makes byte q of both outputs.
template <int NB>
__global__ void __launch_bounds__(256) k_mod_ht40_parse(const uint8_t* __restrict__ in, uint8_t* __restrict__ out0, uint8_t* __restrict__ out1, uint32_t n)
{
    constexpr int IB = 27 * NB, OB = mod_ht40_row(NB), S = NB == 1 ? 1 : NB / 2;
    __shared__ alignas(16) uint32_t s_in[kModHt40Syms * IB / 4];
    __shared__ alignas(16) uint32_t s_out[2][kModHt40Syms * OB / 4];
    const int tid = threadIdx.x;
    const uint32_t s0 = blockIdx.x * kModHt40Syms;
    const int ns = (int)min((uint32_t)kModHt40Syms, n - s0);
    mod_tile_load(s_in, in + (size_t)s0 * IB, ns * IB, tid);
    __syncthreads();
    for (int q = tid; q < ns * OB; q += 256) {
        const int sym = q / OB, j0 = 8 * (q - sym * OB);
        const uint32_t base = (uint32_t)sym * IB * 8;
        unsigned o0 = 0, o1 = 0;
#pragma unroll
        for (int t = 0; t < 8; t++) {
            if (j0 + t < 108 * NB) {
                o0 |= tx_gen_bit(s_in, base + (uint32_t)tx_parse11n_index(S, 0, j0 + t)) << t;
                o1 |= tx_gen_bit(s_in, base + (uint32_t)tx_parse11n_index(S, 1, j0 + t)) << t;
            }
        }
        reinterpret_cast<uint8_t*>(s_out[0])[q] = (uint8_t)o0;
        reinterpret_cast<uint8_t*>(s_out[1])[q] = (uint8_t)o1;
    }
    __syncthreads();
    mod_tile_store(out0 + (size_t)s0 * OB, s_out[0], ns * OB, tid);
    mod_tile_store(out1 + (size_t)s0 * OB, s_out[1], ns * OB, tid);
}
template __global__ void k_mod_ht40_parse<1>(const uint8_t*, uint8_t*, uint8_t*, uint32_t);
template __global__ void k_mod_ht40_parse<2>(const uint8_t*, uint8_t*, uint8_t*, uint32_t);
template __global__ void k_mod_ht40_parse<4>(const uint8_t*, uint8_t*, uint8_t*, uint32_t);
template __global__ void k_mod_ht40_parse<6>(const uint8_t*, uint8_t*, uint8_t*, uint32_t);

// ---- the HT interleaver for 40 MHz: bit k < 108 N_BPSC of a row goes to bit r(k) = deint40_index(N_BPSC, iss, k) (the receiver's de-interleaver reads the same map the
// other way round); the inverse is built once per workgroup in LDS, a thread makes whole output bytes.  BPSK's input bits 108..111 are not read, its output bits 108..111 are 0.
template <int NB>
__global__ void __launch_bounds__(256) k_mod_ht40_interleave(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, int iss, uint32_t n)
{
    constexpr int NCB = 108 * NB, SB = mod_ht40_row(NB);
    __shared__ alignas(16) uint32_t s_in[kModHt40Syms * SB / 4];
    __shared__ alignas(16) uint32_t s_out[kModHt40Syms * SB / 4];
    __shared__ uint16_t s_inv[NCB];
    const int tid = threadIdx.x;
    const uint32_t s0 = blockIdx.x * kModHt40Syms;
    const int ns = (int)min((uint32_t)kModHt40Syms, n - s0), nbytes = ns * SB;
    for (int k = tid; k < NCB; k += 256) s_inv[deint40_index(NB, iss, k)] = (uint16_t)k;
    mod_tile_load(s_in, in + (size_t)s0 * SB, nbytes, tid);
    __syncthreads();
    for (int q = tid; q < nbytes; q += 256)
        reinterpret_cast<uint8_t*>(s_out)[q] = (uint8_t)interleave40_byte<NCB, SB>(reinterpret_cast<const uint8_t*>(s_in), s_inv, q, 0u, 8u * SB);
    __syncthreads();
    mod_tile_store(out + (size_t)s0 * SB, s_out, nbytes, tid);
}
template __global__ void k_mod_ht40_interleave<1>(const uint8_t*, uint8_t*, int, uint32_t);
template __global__ void k_mod_ht40_interleave<2>(const uint8_t*, uint8_t*, int, uint32_t);
template __global__ void k_mod_ht40_interleave<4>(const uint8_t*, uint8_t*, int, uint32_t);
template __global__ void k_mod_ht40_interleave<6>(const uint8_t*, uint8_t*, int, uint32_t);

// ---- the same map on a frame's contiguous coded stream: workgroup (f, y) takes passes of 32 symbols of frame f, y, y + gridDim.y, ..; symbol j reads bits 108 N_BPSC j
// onward of the stream at in + in_off[f] (any alignment; at BPSK an odd symbol starts mid-byte) and makes row first[f] + j of `out`.  A pass's input bits and its output
// rows are contiguous runs: tile_load_any / tile_store_any.  Rows that no frame owns are not written.
template <int NB>
__global__ void __launch_bounds__(256) k_mod_ht40_interleave_stream(const uint8_t* __restrict__ in, const uint32_t* __restrict__ in_off, const uint32_t* __restrict__ first,
        const uint32_t* __restrict__ nsym, uint8_t* __restrict__ out, int iss, uint32_t nframes)
{
    constexpr int NCB = 108 * NB, SB = mod_ht40_row(NB);
    __shared__ alignas(16) uint32_t s_in[(kModHt40Syms * NCB / 8 + 32) / 4];     // the pass's bits, a partial byte, the run's offset in its first 16-byte word
    __shared__ alignas(16) uint32_t s_out[(kModHt40Syms * SB + 16) / 4];
    __shared__ uint16_t s_inv[NCB];
    const uint32_t f = blockIdx.x;
    if (f >= nframes) return;
    const int tid = threadIdx.x;
    const uint32_t nf = nsym[f], sf = first[f];
    const uint8_t* src = in + in_off[f];
    for (int k = tid; k < NCB; k += 256) s_inv[deint40_index(NB, iss, k)] = (uint16_t)k;
    for (uint32_t t0 = blockIdx.y * (uint32_t)kModHt40Syms; t0 < nf; t0 += gridDim.y * (uint32_t)kModHt40Syms) {   // (uniform per workgroup)
        const int ns = (int)min((uint32_t)kModHt40Syms, nf - t0);
        const uint64_t b0 = (uint64_t)NCB * t0;                                  // first bit of the pass in the frame's stream
        const uint8_t* g = src + (b0 >> 3);
        const int sub = (int)(b0 & 7u), nin = (sub + ns * NCB + 7) / 8;
        uint8_t* dst = out + ((size_t)sf + t0) * SB;
        const int nbytes = ns * SB, mo = tile_misalign(dst);
        __syncthreads();                                                         // the pass before has left LDS; s_inv is complete
        tile_load_any(s_in, g, nin, tid);
        __syncthreads();
        const uint32_t bit0 = 8u * (uint32_t)tile_misalign(g) + (uint32_t)sub;
        for (int q = tid; q < nbytes; q += 256)
            reinterpret_cast<uint8_t*>(s_out)[mo + q] = (uint8_t)interleave40_byte<NCB, SB>(reinterpret_cast<const uint8_t*>(s_in), s_inv, q, bit0, (uint32_t)NCB);
        __syncthreads();
        tile_store_any(dst, s_out, nbytes, tid);
    }
}
template __global__ void k_mod_ht40_interleave_stream<1>(const uint8_t*, const uint32_t*, const uint32_t*, const uint32_t*, uint8_t*, int, uint32_t);
template __global__ void k_mod_ht40_interleave_stream<2>(const uint8_t*, const uint32_t*, const uint32_t*, const uint32_t*, uint8_t*, int, uint32_t);
template __global__ void k_mod_ht40_interleave_stream<4>(const uint8_t*, const uint32_t*, const uint32_t*, const uint32_t*, uint8_t*, int, uint32_t);
template __global__ void k_mod_ht40_interleave_stream<6>(const uint8_t*, const uint32_t*, const uint32_t*, const uint32_t*, uint8_t*, int, uint32_t);

// ---- the mapper: carrier c < 108 of a symbol takes bits c N_BPSC .. of its row, the first half for I and the second for Q (tx_axis_level; BPSK: +-d on I), d =
// level40(N_BPSC).  A thread makes four carriers in a row and stores them as one 16-byte word: 27 per symbol.
template <int NB>
__global__ void __launch_bounds__(256) k_mod_ht40_map(const uint8_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t n)
{
    constexpr int SB = mod_ht40_row(NB), M = NB == 1 ? 1 : NB / 2;
    __shared__ alignas(16) uint32_t s_in[kModHt40Syms * SB / 4];
    const int tid = threadIdx.x;
    const uint32_t s0 = blockIdx.x * kModHt40Syms;
    const int ns = (int)min((uint32_t)kModHt40Syms, n - s0);
    mod_tile_load(s_in, in + (size_t)s0 * SB, ns * SB, tid);
    __syncthreads();
    const int d = level40(NB), d2 = 2 * d, lvl0 = -((1 << M) - 1) * d;
    const uint32_t off[3] = { 0u, 1u, 2u };
    uint4* o4 = reinterpret_cast<uint4*>(out + (size_t)s0 * 108);
    for (int q = tid; q < ns * 27; q += 256) {                                   // carriers 4 w .. 4 w + 3 of symbol sym
        const int sym = q / 27, w = q - 27 * sym;
        uint32_t v[4];
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const uint32_t bit0 = (uint32_t)sym * (8 * SB) + (uint32_t)(4 * w + t) * NB;
            if (NB == 1) v[t] = pack(mk(tx_gen_bit(s_in, bit0) ? d : -d, 0));
            else v[t] = pack(mk(tx_axis_level(s_in, bit0, off, M, d2, lvl0), tx_axis_level(s_in, bit0 + M, off, M, d2, lvl0)));
        }
        o4[q] = uint4{v[0], v[1], v[2], v[3]};
    }
}
template __global__ void k_mod_ht40_map<1>(const uint8_t*, uint32_t*, uint32_t);
template __global__ void k_mod_ht40_map<2>(const uint8_t*, uint32_t*, uint32_t);
template __global__ void k_mod_ht40_map<4>(const uint8_t*, uint32_t*, uint32_t);
template __global__ void k_mod_ht40_map<6>(const uint8_t*, uint32_t*, uint32_t);

// ---- L-SIG + HT-SIG: the 144 interleaved bits of a frame -> three complete symbols of 128 bins.  Position c < 48 of symbol s sits at legacy carrier leg(c) (-26..26
// without 0, +-7, +-21: carrier_bin48), +-16384 on I (s = 0, L-SIG) or Q (HT-SIG); the pilots +, +, +, - x 16384 on I at -21, -7, 7, 21; legacy carrier k goes to bin k - 32
// as it is and to bin k + 32 times j (k_tx_ht40.hip: put_dup40, leg_carrier).  A tile of 32 frames (576 bytes); a thread makes four bins in a row: 96 words per frame.
__global__ void __launch_bounds__(256) k_mod_ht40_sig_map(const uint8_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t n)
{
    __shared__ alignas(16) uint32_t s_in[kModHt40Syms * 18 / 4];
    const int tid = threadIdx.x;
    const uint32_t f0 = blockIdx.x * kModHt40Syms;
    const int nf = (int)min((uint32_t)kModHt40Syms, n - f0);
    mod_tile_load(s_in, in + (size_t)f0 * 18, nf * 18, tid);
    __syncthreads();
    uint4* o4 = reinterpret_cast<uint4*>(out + (size_t)f0 * 384);
    for (int q = tid; q < nf * 96; q += 256) {
        const int fr = q / 96, r = q - 96 * fr, s = r >> 5, w = r & 31;
        uint32_t v[4];
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const int b = 4 * w + t, sb = b < 64 ? b : b - 128;                  // the bin as a carrier of the 40 MHz channel, -64..63
            const bool upper = sb >= 0;
            const int k = upper ? sb - 32 : sb + 32;                             // the legacy carrier of that half
            int re = 0, im = 0;
            if (k >= -26 && k <= 26 && k != 0) {
                if (k == -21 || k == -7 || k == 7 || k == 21) re = k == 21 ? -kSigAmp40 : kSigAmp40;
                else {
                    const int c = k < 0 ? (k + 26) - (k > -21) - (k > -7) : 24 + (k - 1) - (k > 7) - (k > 21);
                    const int a = tx_gen_bit(s_in, (uint32_t)(144 * fr + 48 * s + c)) ? kSigAmp40 : -kSigAmp40;
                    if (s == 0) re = a; else im = a;
                }
            }
            v[t] = upper ? pack(mk(-im, re)) : pack(mk(re, im));
        }
        o4[q] = uint4{v[0], v[1], v[2], v[3]};
    }
}

// ---- data carriers and pilots onto the 128 bins: 32 lanes per symbol, 8 symbols per pass of a workgroup; the 108 carriers arrive as 27 16-byte loads, bins 4 e .. 4 e + 3
// leave as one store.  Data carrier c at data_bin40(c) (carriers -58..-2 and 2..58 without the pilots'), pilots (12288, 0) at carriers +-11, +-25, +-53 (k_tx_ht40.hip's
// symbol loop), the 14 other bins 0.  The frame tables are k_mod11n_add_pilot's.
__global__ void __launch_bounds__(256) k_mod_ht40_add_pilot(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, const uint32_t* __restrict__ first,
        const uint32_t* __restrict__ nsym, uint32_t nframes)
{
    __shared__ alignas(16) uint32_t s_all[8][108];
    const uint32_t f = blockIdx.x;
    if (f >= nframes) return;
    const int g = threadIdx.x >> 5, e = threadIdx.x & 31;
    uint32_t* s = s_all[g];
    const uint32_t sf = first[f], ns = nsym[f];
    int src[4];                                                                  // bin 4 e + q: carrier index in the input, -1 = pilot, -2 = zero
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const int b = 4 * e + q, k = b < 64 ? b : b - 128, a = k < 0 ? -k : k;
        if (a == 11 || a == 25 || a == 53) src[q] = -1;
        else if (a < 2 || a > 58) src[q] = -2;
        else src[q] = k < 0 ? (k + 58) - (k > -53) - (k > -25) - (k > -11) : 54 + (k - 2) - (k > 11) - (k > 25) - (k > 53);
    }
    for (uint32_t t0 = blockIdx.y * 8u; t0 < ns; t0 += gridDim.y * 8u) {        // (uniform per workgroup)
        const uint32_t t = t0 + (uint32_t)g;
        const bool active = t < ns;
        const size_t sym = (size_t)sf + t;
        uint4 v = uint4{0, 0, 0, 0};
        if (active && e < 27) v = reinterpret_cast<const uint4*>(in + sym * 108)[e];
        wave_lds_sync();
        if (e < 27) reinterpret_cast<uint4*>(s)[e] = v;
        wave_lds_sync();
        uint32_t o[4];
#pragma unroll
        for (int q = 0; q < 4; q++) o[q] = src[q] >= 0 ? s[src[q]] : src[q] == -1 ? pack(mk(kPilot40, 0)) : 0u;
        if (active) reinterpret_cast<uint4*>(out + sym * 128)[e] = uint4{o[0], o[1], o[2], o[3]};
    }
}

// ---- IFFT<128> of 128 bins in natural order: k_mod11n_ifft's shape -- 32 lanes per symbol, 8 symbols per tile, 4 tiles per workgroup, every tile's load in flight
// before the first butterfly.  Lane e brings bins 4 e .. 4 e + 3 as one 16-byte load into the group's swizzled buffer (fft128_swz: no stage meets a bank conflict);
// tx_ifft128<true> transforms in place; lane e stores time samples 4 e .. 4 e + 3 as they are.
constexpr int kIfftHt40Tiles = 4;
__global__ void __launch_bounds__(256) k_mod_ht40_ifft(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t n, Tables T)
{
    __shared__ alignas(16) uint32_t s_all[8][128];
    const int g = threadIdx.x >> 5, e = threadIdx.x & 31;
    const Fft128Tw tw = fft128_twiddles(T, e);
    uint32_t* s = s_all[g];
    uint4 v[kIfftHt40Tiles];
#pragma unroll
    for (int t = 0; t < kIfftHt40Tiles; t++) {
        const uint32_t i = (blockIdx.x * kIfftHt40Tiles + t) * 8 + g;
        v[t] = i < n ? reinterpret_cast<const uint4*>(in)[(size_t)i * 32 + e] : uint4{0, 0, 0, 0};
    }
#pragma unroll
    for (int t = 0; t < kIfftHt40Tiles; t++) {
        const uint32_t i = (blockIdx.x * kIfftHt40Tiles + t) * 8 + g;
        wave_lds_sync();
        {
            const uint32_t w[4] = { v[t].x, v[t].y, v[t].z, v[t].w };
#pragma unroll
            for (int q = 0; q < 4; q++) s[fft128_swz(4 * e + q)] = w[q];
        }
        tx_ifft128<true>(s, e, tw);
        wave_lds_sync();
        if (i < n) {
            const uint32_t n0 = (uint32_t)(4 * e);
            reinterpret_cast<uint4*>(out + (size_t)i * 128)[e] =
                uint4{ tx_tsample<true>(s, n0), tx_tsample<true>(s, n0 + 1), tx_tsample<true>(s, n0 + 2), tx_tsample<true>(s, n0 + 3) };
        }
    }
}

// ---- the guard interval: 32 + cp 16-byte words per symbol, the last cp of the 32 input words first, then the 32 (cp = 8: long, 160 samples; cp = 4: short, 144); a
// lane moves one output word
__global__ void __launch_bounds__(256) k_mod_ht40_add_gi(const uint4* __restrict__ in, uint4* __restrict__ out, uint32_t cp, uint64_t nwords)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nwords) return;
    const uint32_t per = 32u + cp;
    const uint64_t sym = i / per;
    const uint32_t w = (uint32_t)(i - per * sym);
    out[i] = in[32 * sym + (w < cp ? 32u - cp + w : w - cp)];
}

// ---- the fixed fields: per chain `nw` 16-byte words from word `w0` of the chain's 280 in the table k_tx_ht40_preamble builds ([2][1120] samples), ncopies times back to
// back; a lane moves one word of both chains
__global__ void __launch_bounds__(256) k_mod_ht40_preamble(const uint4* __restrict__ table, uint4* __restrict__ out0, uint4* __restrict__ out1, uint32_t w0, uint32_t nw,
        uint64_t nwords)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nwords) return;
    const uint32_t w = w0 + (uint32_t)(i % nw);
    out0[i] = table[w];
    out1[i] = table[kTxHt40Preamble / 4 + w];
}

}  // namespace sora

using namespace sora;

// ---- the stage entry points (host_stage.h: the prologue and helpers every stage shares).  As the receive stages of this graph do (k_ht40_stages.hip), a bad n_bpsc,
// spatial_stream or gi is refused before the count is looked at.  sora_hip_preamble_ht40 stands beside sora_hip_tx_ht40, whose table it copies.
#define HT40_STREAM(who, iss) \
    if ((iss) < 0 || (iss) > 1) return sora_internal_fail(SORA_ERR_INVALID_PARAM, who ": spatial_stream must be 0 or 1", 0);

int sora_hip_stream_parse_ht40(const uint8_t* d_in, uint8_t* d_out0, uint8_t* d_out1, int n_bpsc, size_t nsym, void* stream)
{
    STAGE_NBPSC("sora_hip_stream_parse_ht40", n_bpsc)
    STAGE_ENTRY("sora_hip_stream_parse_ht40", !d_in || !d_out0 || !d_out1, nsym)
    if (!aligned16(d_in, d_out0, d_out1)) return sora_internal_fail(SORA_ERR_INVALID_PARAM, "sora_hip_stream_parse_ht40: buffers must be 16-byte aligned", 0);
    const dim3 grid((unsigned)((nsym + kModHt40Syms - 1) / kModHt40Syms));
    STAGE_BY_NBPSC(n_bpsc, k_mod_ht40_parse, grid, (hipStream_t)stream, d_in, d_out0, d_out1, (uint32_t)nsym)
    return launch_result("k_mod_ht40_parse");
}

int sora_hip_interleave_ht40(const uint8_t* d_in, uint8_t* d_out, int n_bpsc, int spatial_stream, size_t nsym, void* stream)
{
    STAGE_NBPSC("sora_hip_interleave_ht40", n_bpsc)
    HT40_STREAM("sora_hip_interleave_ht40", spatial_stream)
    STAGE_ENTRY("sora_hip_interleave_ht40", !d_in || !d_out, nsym)
    if (!aligned16(d_in, d_out)) return sora_internal_fail(SORA_ERR_INVALID_PARAM, "sora_hip_interleave_ht40: buffers must be 16-byte aligned", 0);
    const dim3 grid((unsigned)((nsym + kModHt40Syms - 1) / kModHt40Syms));
    STAGE_BY_NBPSC(n_bpsc, k_mod_ht40_interleave, grid, (hipStream_t)stream, d_in, d_out, spatial_stream, (uint32_t)nsym)
    return launch_result("k_mod_ht40_interleave");
}

int sora_hip_interleave_ht40_stream(const uint8_t* d_in, const uint32_t* d_in_off, const uint32_t* d_first, const uint32_t* d_nsym, uint8_t* d_out, int n_bpsc,
                                    int spatial_stream, size_t nframes, void* stream)
{
    STAGE_NBPSC("sora_hip_interleave_ht40_stream", n_bpsc)
    HT40_STREAM("sora_hip_interleave_ht40_stream", spatial_stream)
    STAGE_ENTRY("sora_hip_interleave_ht40_stream", !d_in || !d_in_off || !d_first || !d_nsym || !d_out, nframes)
    if (!aligned16(d_out)) return sora_internal_fail(SORA_ERR_INVALID_PARAM, "sora_hip_interleave_ht40_stream: d_out must be 16-byte aligned", 0);
    // (sora_hip_add_pilot11a's grid: a batch of few frames gets several workgroups per frame, each striding over the frame's passes of 32 symbols)
    const unsigned gy = nframes >= 2048 ? 1u : (unsigned)std::min<size_t>(64, 2048 / nframes);
    const dim3 grid((unsigned)nframes, gy);
    STAGE_BY_NBPSC(n_bpsc, k_mod_ht40_interleave_stream, grid, (hipStream_t)stream, d_in, d_in_off, d_first, d_nsym, d_out, spatial_stream, (uint32_t)nframes)
    return launch_result("k_mod_ht40_interleave_stream");
}

int sora_hip_map_ht40(const uint8_t* d_in, sora_complex16* d_out, int n_bpsc, size_t nsym, void* stream)
{
    STAGE_NBPSC("sora_hip_map_ht40", n_bpsc)
    STAGE_ENTRY("sora_hip_map_ht40", !d_in || !d_out, nsym)
    if (!aligned16(d_in, d_out)) return sora_internal_fail(SORA_ERR_INVALID_PARAM, "sora_hip_map_ht40: buffers must be 16-byte aligned", 0);
    const dim3 grid((unsigned)((nsym + kModHt40Syms - 1) / kModHt40Syms));
    STAGE_BY_NBPSC(n_bpsc, k_mod_ht40_map, grid, (hipStream_t)stream, d_in, u32(d_out), (uint32_t)nsym)
    return launch_result("k_mod_ht40_map");
}

int sora_hip_sig_map_ht40(const uint8_t* d_in, sora_complex16* d_out, size_t nframes, void* stream)
{
    STAGE_ENTRY("sora_hip_sig_map_ht40", !d_in || !d_out, nframes)
    if (!aligned16(d_in, d_out)) return sora_internal_fail(SORA_ERR_INVALID_PARAM, "sora_hip_sig_map_ht40: buffers must be 16-byte aligned", 0);
    hipLaunchKernelGGL(k_mod_ht40_sig_map, dim3((unsigned)((nframes + kModHt40Syms - 1) / kModHt40Syms)), dim3(256), 0, (hipStream_t)stream, d_in, u32(d_out),
                       (uint32_t)nframes);
    return launch_result("k_mod_ht40_sig_map");
}

int sora_hip_add_pilot_ht40(const sora_complex16* d_in, sora_complex16* d_out, const uint32_t* d_first, const uint32_t* d_nsym, size_t nframes, void* stream)
{
    STAGE_ENTRY("sora_hip_add_pilot_ht40", !d_in || !d_out || !d_first || !d_nsym, nframes)
    if (!aligned16(d_in, d_out)) return sora_internal_fail(SORA_ERR_INVALID_PARAM, "sora_hip_add_pilot_ht40: buffers must be 16-byte aligned", 0);
    const unsigned gy = nframes >= 2048 ? 1u : (unsigned)std::min<size_t>(64, 2048 / nframes);
    hipLaunchKernelGGL(k_mod_ht40_add_pilot, dim3((unsigned)nframes, gy), dim3(256), 0, (hipStream_t)stream, u32(d_in), u32(d_out), d_first, d_nsym, (uint32_t)nframes);
    return launch_result("k_mod_ht40_add_pilot");
}

int sora_hip_ifft_ht40(const sora_complex16* d_in, sora_complex16* d_out, size_t nsym, void* stream)
{
    STAGE_ENTRY("sora_hip_ifft_ht40", !d_in || !d_out, nsym)
    if (!aligned16(d_in, d_out)) return sora_internal_fail(SORA_ERR_INVALID_PARAM, "sora_hip_ifft_ht40: buffers must be 16-byte aligned", 0);
    Tables T; if (const int rc = stage_tables(&T)) return rc;
    hipLaunchKernelGGL(k_mod_ht40_ifft, dim3((unsigned)((nsym + 31) / 32)), dim3(256), 0, (hipStream_t)stream, u32(d_in), u32(d_out), (uint32_t)nsym, T);
    return launch_result("k_mod_ht40_ifft");
}

int sora_hip_add_gi_ht40(const sora_complex16* d_in, sora_complex16* d_out, int gi, size_t nsym, void* stream)
{
    if (gi != 0 && gi != 1) return sora_internal_fail(SORA_ERR_INVALID_PARAM, "sora_hip_add_gi_ht40: gi must be 0 (long) or 1 (short)", 0);
    STAGE_ENTRY("sora_hip_add_gi_ht40", !d_in || !d_out, nsym)
    if (!aligned16(d_in, d_out)) return sora_internal_fail(SORA_ERR_INVALID_PARAM, "sora_hip_add_gi_ht40: buffers must be 16-byte aligned", 0);
    const uint32_t cp = gi ? kHt40ShortCp / 4 : 8u;
    const uint64_t nwords = (uint64_t)nsym * (32u + cp);
    hipLaunchKernelGGL(k_mod_ht40_add_gi, dim3((unsigned)((nwords + 255) / 256)), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const uint4*>(d_in),
                       reinterpret_cast<uint4*>(d_out), cp, nwords);
    return launch_result("k_mod_ht40_add_gi");
}
