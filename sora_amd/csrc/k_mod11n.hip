// k_mod11n.hip -- the bricks of the 802.11n 2x2 modulation graphs (kernel/bb/demod11/fb11nmod_config.hpp: CreatePreambleGraph11n, CreateSigGraph11n, CreateModGraph11n) that
// the 802.11a stages of k_mod.hip do not already serve, as stand-alone, batched stages, one C entry point each (include/sora_hip.h), with the reference bricks' port
// formats: bits packed in bytes, LSB first, as the pins carry them.  N_b = ceil(52 N_BPSC / 8) = 7 / 13 / 26 / 39 bytes per stream and symbol.
//   k_mod11n_parse       TStreamParser{BPSK,QPSK,QAM16,QAM64}_12  (Brick11/src/streamparser.hpp, _b_stream_parser.h)   uchar x 13 N_BPSC -> 2 x uchar x N_b
//   k_mod11n_interleave  T11nInterleave*_S1 / _S2                 (interleave.hpp:17-123; N_COL 13, N_ROT 11)           uchar x N_b -> uchar x N_b
//   k_mod11n_map         TMap11a*<MOD> behind them                (mapper11a.hpp:8-300)                                 uchar x N_b -> COMPLEX16 x 52
//   k_mod11n_sig_map     TSigMap11n                               (mapper11n.hpp)                                       uchar x 18 -> COMPLEX16 x 144
//   k_mod11n_add_pilot   T11nAddPilot<iss>                        (pilot_11n.hpp:7-82, _b_dot11_pilot.h)                COMPLEX16 x 52 -> COMPLEX16 x 64
//   k_mod11n_ifft        TIFFTxOnly                               (fft.hpp:63-103)                                      COMPLEX16 x 64 -> COMPLEX16 x 128
//   k_mod11n_csd         TCSD<ncsd>                               (csd.hpp)                                             COMPLEX16 x 128 -> COMPLEX16 x 128
//   k_mod11n_add_gi      TAddGI                                   (gi.hpp)                                              COMPLEX16 x 128 -> COMPLEX16 x 160
//   k_mod11n_preamble    LSrc / HTSrc                             (preamble11n.hpp)                                     -> 2 x COMPLEX16 x 640 / 480
// The arithmetic is dev_tx.h's, dev_11n.h's and dev_pilot11a.h's (what k_tx11n runs); here are the port formats and the streaming shape of k_mod.hip.  The symbol rows of 7,
// 13, 26, 39 or 13 N_BPSC bytes are aligned to nothing, so a workgroup owns a tile of 32 whole symbols (a multiple of 16 bytes whatever the row), moves it between HBM and
// LDS 16 bytes per lane, and reshuffles inside the symbols in LDS.  The parser and the interleaver are index maps (tx_parse11n_index, deint11n_index inverted in LDS), not
// the bricks' 256-entry tables.  CSD, GI and the preamble are moves of 16 bytes per lane: the rotation is by whole 16-byte words.
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "dev_tx.h"
#include "dev_11n.h"
#include "host_stage.h"

namespace sora {

constexpr int kMod11nSyms = 32;                                                  // symbols per workgroup tile of the byte-wide stages and the mapper
__host__ __device__ constexpr int mod11n_row(int nb) { return (52 * nb + 7) / 8; }  // N_b

// ---- TStreamParser*_12: output bit j < 52 N_BPSC of stream s is coded bit tx_parse11n_index(S, s, j) of the symbol.  BPSK's seventh byte carries four bits; its upper
// half is 0 on both outputs (the brick's half-byte table holds four bits of one input byte, `lookuptable2`).  A thread makes byte q of both outputs.
template <int NB>
__global__ void __launch_bounds__(256) k_mod11n_parse(const uint8_t* __restrict__ in, uint8_t* __restrict__ out0, uint8_t* __restrict__ out1, uint32_t n)
{
    constexpr int IB = 13 * NB, OB = mod11n_row(NB), S = NB == 1 ? 1 : NB / 2;
    __shared__ alignas(16) uint32_t s_in[kMod11nSyms * IB / 4];
    __shared__ alignas(16) uint32_t s_out[2][kMod11nSyms * OB / 4];
    const int tid = threadIdx.x;
    const uint32_t s0 = blockIdx.x * kMod11nSyms;
    const int ns = (int)min((uint32_t)kMod11nSyms, n - s0);
    mod_tile_load(s_in, in + (size_t)s0 * IB, ns * IB, tid);
    __syncthreads();
    for (int q = tid; q < ns * OB; q += 256) {
        const int sym = q / OB, j0 = 8 * (q - sym * OB);
        const uint32_t base = (uint32_t)sym * IB * 8;
        unsigned o0 = 0, o1 = 0;
#pragma unroll
        for (int t = 0; t < 8; t++) {
            if (j0 + t < 52 * NB) {
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
template __global__ void k_mod11n_parse<1>(const uint8_t*, uint8_t*, uint8_t*, uint32_t);
template __global__ void k_mod11n_parse<2>(const uint8_t*, uint8_t*, uint8_t*, uint32_t);
template __global__ void k_mod11n_parse<4>(const uint8_t*, uint8_t*, uint8_t*, uint32_t);
template __global__ void k_mod11n_parse<6>(const uint8_t*, uint8_t*, uint8_t*, uint32_t);

// ---- T11nInterleave*_S1 / _S2: bit k of a symbol goes to bit r(k) = deint11n_index(N_BPSC, iss, k) (the receiver's de-interleaver reads the same map the other way
// round); inverted in LDS, a thread makes whole output bytes.  The brick's table is indexed by whole input bytes, so for BPSK k runs to 55: input bits 52..55 are ORed
// onto the positions r(52..55) < 52, which four other bits own as well, and output bits 52..55 are 0.
template <int NB>
__global__ void __launch_bounds__(256) k_mod11n_interleave(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, int iss, uint32_t n)
{
    constexpr int NCB = 52 * NB, SB = mod11n_row(NB);
    __shared__ alignas(16) uint32_t s_in[kMod11nSyms * SB / 4];
    __shared__ alignas(16) uint32_t s_out[kMod11nSyms * SB / 4];
    __shared__ uint16_t s_inv[NCB];
    const int tid = threadIdx.x;
    const uint32_t s0 = blockIdx.x * kMod11nSyms;
    const int ns = (int)min((uint32_t)kMod11nSyms, n - s0), nbytes = ns * SB;
    for (int k = tid; k < NCB; k += 256) s_inv[deint11n_index(NB, iss, k)] = (uint16_t)k;
    mod_tile_load(s_in, in + (size_t)s0 * SB, nbytes, tid);
    __syncthreads();
    const uint8_t* b = reinterpret_cast<const uint8_t*>(s_in);
    for (int q = tid; q < nbytes; q += 256) {
        const int sym = q / SB, p0 = 8 * (q - sym * SB);
        unsigned o = 0;
#pragma unroll
        for (int t = 0; t < 8; t++) {
            if (p0 + t < NCB) { const int k = s_inv[p0 + t]; o |= ((b[sym * SB + (k >> 3)] >> (k & 7)) & 1u) << t; }
        }
        if (NB == 1) {
#pragma unroll
            for (int k = NCB; k < 8 * SB; k++) {                                 // the four bits behind the symbol's 52
                const int r = deint11n_index(NB, iss, k);
                if ((r >> 3) == (p0 >> 3)) o |= ((b[sym * SB + (k >> 3)] >> (k & 7)) & 1u) << (r & 7);
            }
        }
        reinterpret_cast<uint8_t*>(s_out)[q] = (uint8_t)o;
    }
    __syncthreads();
    mod_tile_store(out + (size_t)s0 * SB, s_out, nbytes, tid);
}
template __global__ void k_mod11n_interleave<1>(const uint8_t*, uint8_t*, int, uint32_t);
template __global__ void k_mod11n_interleave<2>(const uint8_t*, uint8_t*, int, uint32_t);
template __global__ void k_mod11n_interleave<4>(const uint8_t*, uint8_t*, int, uint32_t);
template __global__ void k_mod11n_interleave<6>(const uint8_t*, uint8_t*, int, uint32_t);

// ---- TMap11a*<MOD> behind the 11n interleavers: carrier c < 52 of a symbol takes bits c N_BPSC .. of its N_b bytes, the first half for I and the second for Q
// (tx_axis_level; BPSK: +-MOD on I).  The BPSK brick maps all 56 bits of the 7 bytes and T11nAddPilot drops the last four carriers: the stage makes the 52.  A thread
// makes four carriers in a row and stores them as one 16-byte word: 13 per symbol.
template <int NB>
__global__ void __launch_bounds__(256) k_mod11n_map(const uint8_t* __restrict__ in, uint32_t* __restrict__ out, int mod, uint32_t n)
{
    constexpr int SB = mod11n_row(NB), M = NB == 1 ? 1 : NB / 2;
    __shared__ alignas(16) uint32_t s_in[kMod11nSyms * SB / 4];
    const int tid = threadIdx.x;
    const uint32_t s0 = blockIdx.x * kMod11nSyms;
    const int ns = (int)min((uint32_t)kMod11nSyms, n - s0);
    mod_tile_load(s_in, in + (size_t)s0 * SB, ns * SB, tid);
    __syncthreads();
    const int d2 = 2 * mod, lvl0 = -((1 << M) - 1) * mod;
    const uint32_t off[3] = { 0u, 1u, 2u };
    uint4* o4 = reinterpret_cast<uint4*>(out + (size_t)s0 * 52);
    for (int q = tid; q < ns * 13; q += 256) {                                   // carriers 4 w .. 4 w + 3 of symbol sym
        const int sym = q / 13, w = q - 13 * sym;
        uint32_t v[4];
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const uint32_t bit0 = (uint32_t)sym * (8 * SB) + (uint32_t)(4 * w + t) * NB;
            if (NB == 1) v[t] = pack(mk(tx_gen_bit(s_in, bit0) ? mod : -mod, 0));
            else v[t] = pack(mk(tx_axis_level(s_in, bit0, off, M, d2, lvl0), tx_axis_level(s_in, bit0 + M, off, M, d2, lvl0)));   // (short)(l * kmod): pack wraps
        }
        o4[q] = uint4{v[0], v[1], v[2], v[3]};
    }
}
template __global__ void k_mod11n_map<1>(const uint8_t*, uint32_t*, int, uint32_t);
template __global__ void k_mod11n_map<2>(const uint8_t*, uint32_t*, int, uint32_t);
template __global__ void k_mod11n_map<4>(const uint8_t*, uint32_t*, int, uint32_t);
template __global__ void k_mod11n_map<6>(const uint8_t*, uint32_t*, int, uint32_t);

// ---- TSigMap11n: the 144 coded bits of L-SIG + HT-SIG, bytes 0..5 MapBPSK (+-30339 on I), bytes 6..17 MapQBPSK (+-30339 on Q).  A tile of 32 frames (576 bytes); a
// thread makes four carriers: 36 16-byte words per frame.
__global__ void __launch_bounds__(256) k_mod11n_sig_map(const uint8_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t n)
{
    __shared__ alignas(16) uint32_t s_in[kMod11nSyms * 18 / 4];
    const int tid = threadIdx.x;
    const uint32_t f0 = blockIdx.x * kMod11nSyms;
    const int nf = (int)min((uint32_t)kMod11nSyms, n - f0);
    mod_tile_load(s_in, in + (size_t)f0 * 18, nf * 18, tid);
    __syncthreads();
    uint4* o4 = reinterpret_cast<uint4*>(out + (size_t)f0 * 144);
    for (int q = tid; q < nf * 36; q += 256) {                                   // the tile's bits are one string: 144 per frame, carrier = bit
        const bool on_q = q % 36 >= 12;                                          // bytes 6..17 of the frame
        uint32_t v[4];
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const int a = tx_gen_bit(s_in, (uint32_t)(4 * q + t)) ? kBpsk11n : -kBpsk11n;
            v[t] = on_q ? pack(mk(0, a)) : pack(mk(a, 0));
        }
        o4[q] = uint4{v[0], v[1], v[2], v[3]};
    }
}

// ---- T11nAddPilot<iss>: k_mod_add_pilot's shape -- 16 lanes per symbol, 16 symbols per pass of a workgroup; the 52 carriers arrive as thirteen 16-byte loads, bins
// 4 e .. 4 e + 3 leave as one store.  Data on bins 36..63 then 1..28 without +-7 and +-21; the pilots of symbol n of its frame (pos0[f] + its index in the table's
// range) are tx_pilot11n(iss, n, k) at 43, 57, 7, 21; every other bin 0.
__global__ void __launch_bounds__(256) k_mod11n_add_pilot(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, const uint32_t* __restrict__ first,
        const uint32_t* __restrict__ nsym, const uint32_t* __restrict__ pos0, uint32_t nframes, int iss)
{
    __shared__ alignas(16) uint32_t s_all[16][52];
    const uint32_t f = blockIdx.x;
    if (f >= nframes) return;
    const int g = threadIdx.x >> 4, e = threadIdx.x & 15;
    uint32_t* s = s_all[g];
    const uint32_t sf = first[f], ns = nsym[f], p0 = pos0 ? pos0[f] : 0u;
    int src[4];                                                                  // bin 4 e + q: carrier index in the input, -1 - k = pilot k, -5 = zero
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const int b = 4 * e + q;
        if (b == 43) src[q] = -1; else if (b == 57) src[q] = -2; else if (b == 7) src[q] = -3; else if (b == 21) src[q] = -4;
        else if (b >= 1 && b <= 28) src[q] = 26 + (b - 1) - (b > 7) - (b > 21);
        else if (b >= 36) src[q] = b - 36 - (b > 43) - (b > 57);
        else src[q] = -5;
    }
    for (uint32_t t0 = blockIdx.y * 16u; t0 < ns; t0 += gridDim.y * 16u) {      // (uniform per workgroup: every lane keeps the barriers company)
        const uint32_t t = t0 + (uint32_t)g;
        const bool active = t < ns;
        const size_t sym = (size_t)sf + t;
        uint4 v = uint4{0, 0, 0, 0};
        if (active && e < 13) v = reinterpret_cast<const uint4*>(in + sym * 52)[e];
        wave_lds_sync();
        if (e < 13) reinterpret_cast<uint4*>(s)[e] = v;
        wave_lds_sync();
        const uint32_t j = p0 + t;
        uint32_t o[4];
#pragma unroll
        for (int q = 0; q < 4; q++) o[q] = src[q] >= 0 ? s[src[q]] : src[q] > -5 ? pack(mk(tx_pilot11n(iss, j, -1 - src[q]), 0)) : 0u;
        if (active) reinterpret_cast<uint4*>(out + sym * 64)[e] = uint4{o[0], o[1], o[2], o[3]};
    }
}

// ---- TIFFTxOnly: k_mod_ifftx's shape -- 32 lanes per symbol, 8 symbols per tile, 4 tiles per workgroup, every tile's load in flight before the first butterfly.  Lanes
// 0 .. 15 bring bins 4 e .. 4 e + 3 as one 16-byte load and put them at bins 0 .. 31 / 96 .. 127 of the group's swizzled 128-word buffer, lanes 16 .. 31 clear the 64
// bins between; tx_ifft128<true> transforms in place; lane e stores time samples 4 e .. 4 e + 3 as they are: no shift, no guard interval, no window.
constexpr int kIfft11nTiles = 4;
__global__ void __launch_bounds__(256) k_mod11n_ifft(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t n, Tables T)
{
    __shared__ alignas(16) uint32_t s_all[8][128];
    const int g = threadIdx.x >> 5, e = threadIdx.x & 31;
    const Fft128Tw tw = fft128_twiddles(T, e);
    uint32_t* s = s_all[g];
    uint4 v[kIfft11nTiles];
#pragma unroll
    for (int t = 0; t < kIfft11nTiles; t++) {
        const uint32_t i = (blockIdx.x * kIfft11nTiles + t) * 8 + g;
        v[t] = (i < n && e < 16) ? reinterpret_cast<const uint4*>(in)[(size_t)i * 16 + e] : uint4{0, 0, 0, 0};
    }
#pragma unroll
    for (int t = 0; t < kIfft11nTiles; t++) {
        const uint32_t i = (blockIdx.x * kIfft11nTiles + t) * 8 + g;
        wave_lds_sync();
        {
            const int b0 = e < 16 ? bin128(4 * e) : 32 + 4 * (e - 16);               // four bins in a row on the 128-point grid; the swizzle moves them one by one
            const uint32_t w[4] = { v[t].x, v[t].y, v[t].z, v[t].w };
#pragma unroll
            for (int q = 0; q < 4; q++) s[fft128_swz(b0 + q)] = w[q];
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

// ---- TCSD<ncsd>: output sample (i + 4 ncsd) mod 128 is input sample i -- 16-byte word (w + ncsd) mod 32 of a symbol is its input word w; a lane moves one word
__global__ void __launch_bounds__(256) k_mod11n_csd(const uint4* __restrict__ in, uint4* __restrict__ out, int ncsd, uint64_t nwords)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nwords) return;
    out[(i & ~(uint64_t)31) | ((i + (uint64_t)ncsd) & 31u)] = in[i];
}

// ---- TAddGI: 40 words per symbol, the last 8 of the 32 input words first, then the 32; a lane moves one output word
__global__ void __launch_bounds__(256) k_mod11n_add_gi(const uint4* __restrict__ in, uint4* __restrict__ out, uint64_t nwords)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nwords) return;
    const uint64_t sym = i / 40;
    const uint32_t w = (uint32_t)(i - 40 * sym);
    out[i] = in[32 * sym + (w < 8 ? 24 + w : w - 8)];
}

// ---- LSrc / HTSrc: per chain `nw` 16-byte words from word `w0` of the chain's 280 in the table k_tx11n copies its fixed fields from ([2][1120] samples), ncopies times
// back to back; a lane moves one word of both chains
__global__ void __launch_bounds__(256) k_mod11n_preamble(const uint4* __restrict__ table, uint4* __restrict__ out0, uint4* __restrict__ out1, uint32_t w0, uint32_t nw,
        uint64_t nwords)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nwords) return;
    const uint32_t w = w0 + (uint32_t)(i % nw);
    out0[i] = table[w];
    out1[i] = table[kTx11nPreamble / 4 + w];
}

}  // namespace sora

using namespace sora;

// ---- the stage entry points (host_stage.h: the prologue and helpers every stage shares).  sora_hip_preamble11n stands beside sora_hip_tx11n, whose table it copies
int sora_hip_stream_parse11n(const uint8_t* d_in, uint8_t* d_out0, uint8_t* d_out1, int n_bpsc, size_t nsym, void* stream)
{
    STAGE_ENTRY("sora_hip_stream_parse11n", !d_in || !d_out0 || !d_out1, nsym)
    STAGE_NBPSC("sora_hip_stream_parse11n", n_bpsc)
    if (!aligned16(d_in, d_out0, d_out1)) return sora_internal_fail(SORA_ERR_INVALID_PARAM, "sora_hip_stream_parse11n: buffers must be 16-byte aligned", 0);
    const dim3 grid((unsigned)((nsym + 31) / 32));
    STAGE_BY_NBPSC(n_bpsc, k_mod11n_parse, grid, (hipStream_t)stream, d_in, d_out0, d_out1, (uint32_t)nsym)
    return launch_result("k_mod11n_parse");
}

int sora_hip_interleave11n(const uint8_t* d_in, uint8_t* d_out, int n_bpsc, int spatial_stream, size_t nsym, void* stream)
{
    STAGE_ENTRY("sora_hip_interleave11n", !d_in || !d_out, nsym)
    STAGE_NBPSC("sora_hip_interleave11n", n_bpsc)
    if (spatial_stream < 0 || spatial_stream > 1) return sora_internal_fail(SORA_ERR_INVALID_PARAM, "sora_hip_interleave11n: spatial_stream must be 0 or 1", 0);
    if (!aligned16(d_in, d_out)) return sora_internal_fail(SORA_ERR_INVALID_PARAM, "sora_hip_interleave11n: buffers must be 16-byte aligned", 0);
    const dim3 grid((unsigned)((nsym + 31) / 32));
    STAGE_BY_NBPSC(n_bpsc, k_mod11n_interleave, grid, (hipStream_t)stream, d_in, d_out, spatial_stream, (uint32_t)nsym)
    return launch_result("k_mod11n_interleave");
}

int sora_hip_map11n(const uint8_t* d_in, sora_complex16* d_out, int n_bpsc, int mod, size_t nsym, void* stream)
{
    STAGE_ENTRY("sora_hip_map11n", !d_in || !d_out, nsym)
    STAGE_NBPSC("sora_hip_map11n", n_bpsc)
    if (mod < 0 || mod > 32767) return sora_internal_fail(SORA_ERR_INVALID_PARAM, "sora_hip_map11n: mod must be 0 .. 32767", 0);
    if (!aligned16(d_in, d_out)) return sora_internal_fail(SORA_ERR_INVALID_PARAM, "sora_hip_map11n: buffers must be 16-byte aligned", 0);
    if (mod == 0) mod = n_bpsc == 1 ? 30339 : n_bpsc == 2 ? 21453 : n_bpsc == 4 ? 9594 : 4681;   // fb11nmod_config.hpp:121-128
    const dim3 grid((unsigned)((nsym + 31) / 32));
    STAGE_BY_NBPSC(n_bpsc, k_mod11n_map, grid, (hipStream_t)stream, d_in, u32(d_out), mod, (uint32_t)nsym)
    return launch_result("k_mod11n_map");
}

int sora_hip_sig_map11n(const uint8_t* d_in, sora_complex16* d_out, size_t nframes, void* stream)
{
    STAGE_ENTRY("sora_hip_sig_map11n", !d_in || !d_out, nframes)
    if (!aligned16(d_in, d_out)) return sora_internal_fail(SORA_ERR_INVALID_PARAM, "sora_hip_sig_map11n: buffers must be 16-byte aligned", 0);
    hipLaunchKernelGGL(k_mod11n_sig_map, dim3((unsigned)((nframes + 31) / 32)), dim3(256), 0, (hipStream_t)stream, d_in, u32(d_out), (uint32_t)nframes);
    return launch_result("k_mod11n_sig_map");
}

int sora_hip_add_pilot11n(const sora_complex16* d_in, sora_complex16* d_out, const uint32_t* d_first, const uint32_t* d_nsym, const uint32_t* d_pos0,
                          size_t nframes, int spatial_stream, void* stream)
{
    STAGE_ENTRY("sora_hip_add_pilot11n", !d_in || !d_out || !d_first || !d_nsym, nframes)
    if (spatial_stream < 0 || spatial_stream > 1) return sora_internal_fail(SORA_ERR_INVALID_PARAM, "sora_hip_add_pilot11n: spatial_stream must be 0 or 1", 0);
    if (!aligned16(d_in, d_out)) return sora_internal_fail(SORA_ERR_INVALID_PARAM, "sora_hip_add_pilot11n: buffers must be 16-byte aligned", 0);
    // (sora_hip_add_pilot11a's grid: a batch of few frames gets several workgroups per frame, each striding over the frame's passes of 16 symbols)
    const unsigned gy = nframes >= 2048 ? 1u : (unsigned)std::min<size_t>(64, 2048 / nframes);
    hipLaunchKernelGGL(k_mod11n_add_pilot, dim3((unsigned)nframes, gy), dim3(256), 0, (hipStream_t)stream, u32(d_in), u32(d_out), d_first, d_nsym, d_pos0, (uint32_t)nframes,
                       spatial_stream);
    return launch_result("k_mod11n_add_pilot");
}

int sora_hip_ifft_only11n(const sora_complex16* d_in, sora_complex16* d_out, size_t nsym, void* stream)
{
    STAGE_ENTRY("sora_hip_ifft_only11n", !d_in || !d_out, nsym)
    if (!aligned16(d_in, d_out)) return sora_internal_fail(SORA_ERR_INVALID_PARAM, "sora_hip_ifft_only11n: buffers must be 16-byte aligned", 0);
    Tables T; if (const int rc = stage_tables(&T)) return rc;
    hipLaunchKernelGGL(k_mod11n_ifft, dim3((unsigned)((nsym + 31) / 32)), dim3(256), 0, (hipStream_t)stream, u32(d_in), u32(d_out), (uint32_t)nsym, T);
    return launch_result("k_mod11n_ifft");
}

int sora_hip_csd11n(const sora_complex16* d_in, sora_complex16* d_out, int ncsd, size_t nsym, void* stream)
{
    STAGE_ENTRY("sora_hip_csd11n", !d_in || !d_out, nsym)
    if (ncsd < 1 || ncsd > 31) return sora_internal_fail(SORA_ERR_INVALID_PARAM, "sora_hip_csd11n: ncsd must be 1 .. 31", 0);
    if (d_in == d_out) return sora_internal_fail(SORA_ERR_INVALID_PARAM, "sora_hip_csd11n: out of place only", 0);
    if (!aligned16(d_in, d_out)) return sora_internal_fail(SORA_ERR_INVALID_PARAM, "sora_hip_csd11n: buffers must be 16-byte aligned", 0);
    const uint64_t nwords = (uint64_t)nsym * 32;
    hipLaunchKernelGGL(k_mod11n_csd, dim3((unsigned)((nwords + 255) / 256)), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const uint4*>(d_in),
                       reinterpret_cast<uint4*>(d_out), ncsd, nwords);
    return launch_result("k_mod11n_csd");
}

int sora_hip_add_gi11n(const sora_complex16* d_in, sora_complex16* d_out, size_t nsym, void* stream)
{
    STAGE_ENTRY("sora_hip_add_gi11n", !d_in || !d_out, nsym)
    if (!aligned16(d_in, d_out)) return sora_internal_fail(SORA_ERR_INVALID_PARAM, "sora_hip_add_gi11n: buffers must be 16-byte aligned", 0);
    const uint64_t nwords = (uint64_t)nsym * 40;
    hipLaunchKernelGGL(k_mod11n_add_gi, dim3((unsigned)((nwords + 255) / 256)), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const uint4*>(d_in),
                       reinterpret_cast<uint4*>(d_out), nwords);
    return launch_result("k_mod11n_add_gi");
}
