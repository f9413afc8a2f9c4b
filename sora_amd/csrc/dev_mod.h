// dev_mod.h -- what the OFDM modulation stages of k_mod.hip (802.11a), k_mod11n.hip (802.11n 20 MHz) and k_mod_ht40.hip (40 MHz HT) share, each thing once: the tile
// shape and its moves, and the bodies of the stream parser, the interleaver, the mapper, the pilot stage, the IFFT, the guard interval and the preamble copy.  A graph's
// kernel is a few lines that give a body its widths (carriers per symbol, lanes per symbol) and its policies (an index map, a carrier plan, where bins land, what is
// emitted); the arithmetic is dev_tx.h's.  Workgroups of 256 threads throughout.
#pragma once
#include "kernels.h"
#include "dev_tx.h"

namespace sora {

// ---- the tile: 32 whole symbols (or frames) per workgroup of the byte-wide stages and the mappers, a multiple of 16 bytes whatever the row
constexpr int kModTile = 32;
__host__ __device__ constexpr int mod_row(int carriers, int nb) { return (carriers * nb + 7) / 8; }   // bytes per symbol row: 6 N_BPSC (48 carriers), N_b (52), N_b40 (108)

// a kernel template's 1 / 2 / 4 / 6 instances (N_BPSC), behind its definition: MOD_INSTANCES(kernel, its parameter types)
#define MOD_INSTANCES(kernel, ...) \
    template __global__ void kernel<1>(__VA_ARGS__); template __global__ void kernel<2>(__VA_ARGS__); \
    template __global__ void kernel<4>(__VA_ARGS__); template __global__ void kernel<6>(__VA_ARGS__);

// ---- a tile of nbytes contiguous bytes between 16-byte aligned global memory and LDS: 16 bytes per lane, the ragged end of a last tile byte by byte
__device__ __forceinline__ void mod_tile_load(uint32_t* s, const uint8_t* g, int nbytes, int tid)
{
    for (int q = tid; q < (nbytes + 15) / 16; q += 256) {
        if (16 * q + 16 <= nbytes) reinterpret_cast<uint4*>(s)[q] = reinterpret_cast<const uint4*>(g)[q];
        else for (int b = 16 * q; b < 16 * q + 16; b++) reinterpret_cast<uint8_t*>(s)[b] = b < nbytes ? g[b] : (uint8_t)0;
    }
}
__device__ __forceinline__ void mod_tile_store(uint8_t* g, const uint32_t* s, int nbytes, int tid)
{
    for (int q = tid; q < (nbytes + 15) / 16; q += 256) {
        if (16 * q + 16 <= nbytes) reinterpret_cast<uint4*>(g)[q] = reinterpret_cast<const uint4*>(s)[q];
        else for (int b = 16 * q; b < nbytes; b++) g[b] = reinterpret_cast<const uint8_t*>(s)[b];
    }
}
// ---- the same at ANY alignment: the LDS copy keeps the address's offset inside its 16-byte word (byte b of the run is LDS byte (g & 15) + b), so every 16-byte word
// that lies wholly inside the run moves as one load or store and the ragged ends go byte by byte.  Nothing outside the run is read or written.
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

// ---- the stream parser (TStreamParser*_12), C carriers per stream: output bit j < C N_BPSC of stream s is coded bit tx_parse11n_index(S, s, j) of the symbol's
// 2 C N_BPSC.  BPSK's last byte carries four bits; its upper half is 0 on both outputs (the brick's half-byte table holds four bits of one input byte,
// `lookuptable2`).  A thread makes byte q of both outputs.
template <int C, int NB>
__device__ __forceinline__ void mod_parse_tile(const uint8_t* __restrict__ in, uint8_t* __restrict__ out0, uint8_t* __restrict__ out1, uint32_t n)
{
    constexpr int IB = C * NB / 4, OB = mod_row(C, NB), S = NB == 1 ? 1 : NB / 2;
    __shared__ alignas(16) uint32_t s_in[kModTile * IB / 4];
    __shared__ alignas(16) uint32_t s_out[2][kModTile * OB / 4];
    const int tid = threadIdx.x;
    const uint32_t s0 = blockIdx.x * kModTile;
    const int ns = (int)min((uint32_t)kModTile, n - s0);
    mod_tile_load(s_in, in + (size_t)s0 * IB, ns * IB, tid);
    __syncthreads();
    for (int q = tid; q < ns * OB; q += 256) {
        const int sym = q / OB, j0 = 8 * (q - sym * OB);
        const uint32_t base = (uint32_t)sym * IB * 8;
        unsigned o0 = 0, o1 = 0;
#pragma unroll
        for (int t = 0; t < 8; t++) {
            if (j0 + t < C * NB) {
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

// ---- the interleavers.  An index map says where coded bit k of a symbol goes (the receiver's de-interleaver reads the same map the other way round); a workgroup
// inverts it into s_inv once and a thread makes whole output bytes.  Each graph's file states its map as a functor: map(k) is the position of bit k, and
// Map::kOrsPadBits says whether the pad bits behind a BPSK row are ORed in (mod_interleave_pad_bits: the 802.11n brick's quirk) or not read.
template <int NCB, class Map>
__device__ __forceinline__ void mod_invert_map(uint16_t* s_inv, const Map map, int tid)
{
    for (unsigned k = tid; k < (unsigned)NCB; k += 256) s_inv[map((int)k)] = (uint16_t)k;   // (an unsigned counter: the closed-form maps' divisions stay unsigned ones)
}
// the byte at positions p0 .. p0 + 7 of an interleaved row: position p < NCB takes coded bit s_inv[p] of its symbol, whose bit 0 is bit `bit0` behind byte `byte0` of b
// (a tile of rows: the row's first byte, bit 0; a stream: byte 0, the symbol's bit address).  Positions at or behind NCB (BPSK's last half byte) are 0.
template <int NCB>
__device__ __forceinline__ unsigned mod_interleave_byte(const uint8_t* b, const uint16_t* s_inv, int p0, int byte0, uint32_t bit0)
{
    unsigned o = 0;
#pragma unroll
    for (int t = 0; t < 8; t++) {
        if (p0 + t < NCB) { const uint32_t a = bit0 + s_inv[p0 + t]; o |= ((b[byte0 + (a >> 3)] >> (a & 7u)) & 1u) << t; }
    }
    return o;
}
// The 802.11n brick's quirk (Map::kOrsPadBits): its table is indexed by whole input bytes, so at BPSK k runs to 55 -- input bits 52..55, behind the symbol's 52, are
// ORed onto the positions map(52..55) < 52, which four other bits own as well.  What of that falls into the byte at positions p0 .. p0 + 7 of the row b.
template <int NCB, int SB, class Map>
__device__ __forceinline__ unsigned mod_interleave_pad_bits(const uint8_t* b, const Map map, int p0)
{
    unsigned o = 0;
#pragma unroll
    for (int k = NCB; k < 8 * SB; k++) {
        const int r = map(k);
        if ((r >> 3) == (p0 >> 3)) o |= ((b[k >> 3] >> (k & 7)) & 1u) << (r & 7);
    }
    return o;
}
// a tile of rows of C carriers
template <int C, int NB, class Map>
__device__ __forceinline__ void mod_interleave_tile(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, uint32_t n, const Map map)
{
    constexpr int NCB = C * NB, SB = mod_row(C, NB);
    __shared__ alignas(16) uint32_t s_in[kModTile * SB / 4];
    __shared__ alignas(16) uint32_t s_out[kModTile * SB / 4];
    __shared__ uint16_t s_inv[NCB];
    const int tid = threadIdx.x;
    const uint32_t s0 = blockIdx.x * kModTile;
    const int ns = (int)min((uint32_t)kModTile, n - s0), nbytes = ns * SB;
    mod_invert_map<NCB>(s_inv, map, tid);
    mod_tile_load(s_in, in + (size_t)s0 * SB, nbytes, tid);
    __syncthreads();
    const uint8_t* b = reinterpret_cast<const uint8_t*>(s_in);
    for (int q = tid; q < nbytes; q += 256) {
        const int sym = q / SB, p0 = 8 * (q - sym * SB);
        unsigned o = mod_interleave_byte<NCB>(b, s_inv, p0, sym * SB, 0u);
        if (Map::kOrsPadBits) o |= mod_interleave_pad_bits<NCB, SB>(b + sym * SB, map, p0);
        reinterpret_cast<uint8_t*>(s_out)[q] = (uint8_t)o;
    }
    __syncthreads();
    mod_tile_store(out + (size_t)s0 * SB, s_out, nbytes, tid);
}

// ---- the mappers (TMap11a*<MOD>), C carriers per symbol: carrier c takes bits c N_BPSC .. of its row, the first half for I and the second for Q (tx_axis_level; BPSK:
// +-mod on I).  A thread makes four carriers in a row and stores them as one 16-byte word, C / 4 per symbol.
template <int C, int NB>
__device__ __forceinline__ void mod_map_tile(const uint8_t* __restrict__ in, uint32_t* __restrict__ out, int mod, uint32_t n)
{
    constexpr int SB = mod_row(C, NB), M = NB == 1 ? 1 : NB / 2, W = C / 4;
    constexpr bool kString = C % 8 == 0;                                         // 48 carriers: no row ends in pad bits, whatever N_BPSC -- the tile's bits are one string
    __shared__ alignas(16) uint32_t s_in[kModTile * SB / 4];
    const int tid = threadIdx.x;
    const uint32_t s0 = blockIdx.x * kModTile;
    const int ns = (int)min((uint32_t)kModTile, n - s0);
    mod_tile_load(s_in, in + (size_t)s0 * SB, ns * SB, tid);
    __syncthreads();
    const int d2 = 2 * mod, lvl0 = -((1 << M) - 1) * mod;
    const uint32_t off[3] = { 0u, 1u, 2u };
    uint4* o4 = reinterpret_cast<uint4*>(out + (size_t)s0 * C);
    for (int q = tid; q < ns * W; q += 256) {                                    // carriers 4 w .. 4 w + 3 of symbol sym
        const int sym = q / W, w = q - W * sym;
        uint32_t v[4];
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const uint32_t bit0 = kString ? (uint32_t)(4 * q + t) * NB : (uint32_t)sym * (8 * SB) + (uint32_t)(4 * w + t) * NB;
            if (NB == 1) v[t] = pack(mk(tx_gen_bit(s_in, bit0) ? mod : -mod, 0));
            else v[t] = pack(mk(tx_axis_level(s_in, bit0, off, M, d2, lvl0), tx_axis_level(s_in, bit0 + M, off, M, d2, lvl0)));   // (short)(l * kmod): pack wraps
        }
        o4[q] = uint4{v[0], v[1], v[2], v[3]};
    }
}

// ---- the pilot stages: LANES lanes per symbol, 256 / LANES symbols per pass of a workgroup; a symbol's P::kCarriers data carriers arrive as 16-byte loads, its 4 LANES
// bins leave as one 16-byte store per lane, bins 4 e .. 4 e + 3.  Workgroup (f, y) takes passes y, y + gridDim.y, .. of frame f: symbols first[f] .. + nsym[f] of the
// buffers; the symbol at index t of that range is at position j = pos0[f] + t of its frame (pos0 null: 0).  The policy P is the carrier plan:
//   P::source(b)     what bin b holds, decided once per lane: >= 0 the data carrier's index in the input; < 0 a kind of the policy's own (a pilot, nothing)
//   p.word(k, b, j)  the word of bin b of kind k < 0 in the symbol at position j
template <int LANES, class P>
__device__ __forceinline__ void mod_pilot_frames(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, const uint32_t* __restrict__ first,
        const uint32_t* __restrict__ nsym, const uint32_t* __restrict__ pos0, uint32_t nframes, const P p)
{
    constexpr int G = 256 / LANES, W = P::kCarriers / 4;
    __shared__ alignas(16) uint32_t s_all[G][P::kCarriers];
    const uint32_t f = blockIdx.x;
    if (f >= nframes) return;
    const int g = threadIdx.x / LANES, e = threadIdx.x % LANES;
    uint32_t* s = s_all[g];
    const uint32_t sf = first[f], ns = nsym[f], p0 = pos0 ? pos0[f] : 0u;
    int src[4];
#pragma unroll
    for (int q = 0; q < 4; q++) src[q] = P::source(4 * e + q);
    for (uint32_t t0 = blockIdx.y * (uint32_t)G; t0 < ns; t0 += gridDim.y * (uint32_t)G) {   // (uniform per workgroup: every lane keeps the barriers company)
        const uint32_t t = t0 + (uint32_t)g;
        const bool active = t < ns;
        const size_t sym = (size_t)sf + t;
        uint4 v = uint4{0, 0, 0, 0};
        if (active && e < W) v = reinterpret_cast<const uint4*>(in + sym * P::kCarriers)[e];
        wave_lds_sync();
        if (e < W) reinterpret_cast<uint4*>(s)[e] = v;
        wave_lds_sync();
        const uint32_t j = p0 + t;
        uint32_t o[4];
#pragma unroll
        for (int q = 0; q < 4; q++) o[q] = src[q] >= 0 ? s[src[q]] : p.word(src[q], 4 * e + q, j);
        if (active) reinterpret_cast<uint4*>(out + sym * (4 * LANES))[e] = uint4{o[0], o[1], o[2], o[3]};
    }
}

// ---- the IFFTs: 32 lanes per symbol, 8 symbols per tile, kModIfftTiles tiles per workgroup, every tile's load in flight before the first butterfly (k_fft128_batch's
// shape).  Place::kLanes lanes bring four bins each as one 16-byte load; lane e puts its four words (zeros where it brought none) at bins Place::bin0(e) .. + 3 of the
// group's swizzled 128-word buffer (fft128_swz: no stage meets a bank conflict; the swizzle moves them one by one); tx_ifft128<true> transforms in place;
// Emit::store writes the symbol.
constexpr int kModIfftTiles = 4;
constexpr int kModIfftSyms = 8 * kModIfftTiles;                                  // symbols per workgroup
struct ModPlace64 {                        // 64 bins around DC: bins 0 .. 31 / 32 .. 63 go to 0 .. 31 / 96 .. 127, lanes 16 .. 31 clear the 64 bins between
    static constexpr int kLanes = 16;
    static __device__ __forceinline__ int bin0(int e) { return e < 16 ? bin128(4 * e) : 32 + 4 * (e - 16); }
};
struct ModPlace128 {                       // 128 bins in natural order
    static constexpr int kLanes = 32;
    static __device__ __forceinline__ int bin0(int e) { return 4 * e; }
};
struct ModEmitPlain {                      // TIFFTxOnly: lane e stores time samples 4 e .. 4 e + 3 as they are -- no shift, no guard interval, no window
    static __device__ __forceinline__ void store(uint32_t* __restrict__ out, uint32_t i, const uint32_t* s, int e)
    {
        const uint32_t n0 = (uint32_t)(4 * e);
        reinterpret_cast<uint4*>(out + (size_t)i * 128)[e] = uint4{ tx_tsample<true>(s, n0), tx_tsample<true>(s, n0 + 1), tx_tsample<true>(s, n0 + 2), tx_tsample<true>(s, n0 + 3) };
    }
};
struct ModEmitGiWindow {                   // TIFFTx: 160 samples, output sample i = time sample (i + 96) & 127, >> 4, so lane e stores samples 4 e .. 4 e + 3 and, for
    // e < 8, the same four time samples as 128 + 4 e .. (the guard interval is the symbol's last 32 samples in front): each output sample is written once, 16 bytes per
    // lane.  Samples 0, 1, 158 and 159 are halved (the window).
    static __device__ __forceinline__ uint4 quad(const uint32_t* s, int e, int sh01, int sh23)
    {
        const uint32_t n0 = (uint32_t)(4 * e + 96);
        return uint4{ pk_sra(tx_tsample<true>(s, n0), sh01), pk_sra(tx_tsample<true>(s, n0 + 1), sh01), pk_sra(tx_tsample<true>(s, n0 + 2), sh23), pk_sra(tx_tsample<true>(s, n0 + 3), sh23) };
    }
    static __device__ __forceinline__ void store(uint32_t* __restrict__ out, uint32_t i, const uint32_t* s, int e)
    {
        uint4* o = reinterpret_cast<uint4*>(out + (size_t)i * 160);
        o[e] = quad(s, e, e == 0 ? 5 : 4, 4);
        if (e < 8) o[32 + e] = quad(s, e, 4, e == 7 ? 5 : 4);
    }
};
template <class Place, class Emit>
__device__ __forceinline__ void mod_ifft_tiles(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t n, const Tables& T)
{
    __shared__ alignas(16) uint32_t s_all[8][128];
    const int g = threadIdx.x >> 5, e = threadIdx.x & 31;
    const Fft128Tw tw = fft128_twiddles(T, e);
    uint32_t* s = s_all[g];
    uint4 v[kModIfftTiles];
#pragma unroll
    for (int t = 0; t < kModIfftTiles; t++) {
        const uint32_t i = (blockIdx.x * kModIfftTiles + t) * 8 + g;
        v[t] = (i < n && e < Place::kLanes) ? reinterpret_cast<const uint4*>(in)[(size_t)i * Place::kLanes + e] : uint4{0, 0, 0, 0};
    }
#pragma unroll
    for (int t = 0; t < kModIfftTiles; t++) {
        const uint32_t i = (blockIdx.x * kModIfftTiles + t) * 8 + g;
        wave_lds_sync();
        {
            const int b0 = Place::bin0(e);
            const uint32_t w[4] = { v[t].x, v[t].y, v[t].z, v[t].w };
#pragma unroll
            for (int q = 0; q < 4; q++) s[fft128_swz(b0 + q)] = w[q];
        }
        tx_ifft128<true>(s, e, tw);
        wave_lds_sync();
        if (i < n) Emit::store(out, i, s, e);
    }
}

// ---- the guard interval (TAddGI): 32 + cp 16-byte words per symbol, the last cp of the 32 input words first, then the 32 (cp = 8: long, 160 samples; cp = 4: short,
// 144); a lane moves one output word
__device__ __forceinline__ void mod_add_gi_word(const uint4* __restrict__ in, uint4* __restrict__ out, uint32_t cp, uint64_t nwords)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nwords) return;
    const uint32_t per = 32u + cp;
    const uint64_t sym = i / per;
    const uint32_t w = (uint32_t)(i - per * sym);
    out[i] = in[32 * sym + (w < cp ? 32u - cp + w : w - cp)];
}

// ---- the fixed fields of a two-chain transmitter (LSrc / HTSrc): per chain `nw` 16-byte words from word `w0` of the chain's `chain` words in the transmitter's table,
// ncopies times back to back; a lane moves one word of both chains
__device__ __forceinline__ void mod_preamble_word(const uint4* __restrict__ table, uint32_t chain, uint4* __restrict__ out0, uint4* __restrict__ out1, uint32_t w0,
        uint32_t nw, uint64_t nwords)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nwords) return;
    const uint32_t w = w0 + (uint32_t)(i % nw);
    out0[i] = table[w];
    out1[i] = table[chain + w];
}

}  // namespace sora
