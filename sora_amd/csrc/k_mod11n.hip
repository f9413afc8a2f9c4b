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
// The arithmetic is dev_tx.h's, dev_11n.h's and dev_pilot11a.h's (what k_tx11n runs).  The symbol rows of 7, 13, 26, 39 or 13 N_BPSC bytes are aligned to nothing, so a
// workgroup owns a tile of 32 whole symbols (a multiple of 16 bytes whatever the row), moves it between HBM and LDS 16 bytes per lane, and reshuffles inside the symbols
// in LDS: the tile shape and the bodies of the parser, the interleaver, the mapper, the pilot stage, the IFFT, the guard interval and the preamble copy are dev_mod.h's,
// which the 802.11a and 40 MHz HT graphs instantiate too; here are this graph's widths and policies.  The parser and the interleaver are index maps (tx_parse11n_index,
// deint11n_index inverted in LDS), not the bricks' 256-entry tables.  CSD, GI and the preamble are moves of 16 bytes per lane: the rotation is by whole 16-byte words.
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "dev_tx.h"
#include "dev_mod.h"
#include "dev_11n.h"
#include "host_stage.h"

namespace sora {

// ---- TStreamParser*_12: mod_parse_tile, 52 carriers per stream; BPSK's seventh byte carries four bits
template <int NB>
__global__ void __launch_bounds__(256) k_mod11n_parse(const uint8_t* __restrict__ in, uint8_t* __restrict__ out0, uint8_t* __restrict__ out1, uint32_t n)
{
    mod_parse_tile<52, NB>(in, out0, out1, n);
}
MOD_INSTANCES(k_mod11n_parse, const uint8_t*, uint8_t*, uint8_t*, uint32_t)

// ---- T11nInterleave*_S1 / _S2: mod_interleave_tile; bit k of a symbol goes to bit r(k) = deint11n_index(N_BPSC, iss, k).  The brick's table is indexed by whole input
// bytes, so for BPSK k runs to 55: input bits 52..55 are ORed onto the positions r(52..55) < 52 (kOrsPadBits), and output bits 52..55 are 0.
template <int NB>
struct ModMap11n {
    static constexpr bool kOrsPadBits = true;
    int iss;
    __device__ __forceinline__ int operator()(int k) const { return deint11n_index(NB, iss, k); }
};
template <int NB>
__global__ void __launch_bounds__(256) k_mod11n_interleave(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, int iss, uint32_t n)
{
    mod_interleave_tile<52, NB>(in, out, n, ModMap11n<NB>{ iss });
}
MOD_INSTANCES(k_mod11n_interleave, const uint8_t*, uint8_t*, int, uint32_t)

// ---- TMap11a*<MOD> behind the 11n interleavers: mod_map_tile on the 52 carriers of a symbol's N_b bytes, 13 words per symbol.  The BPSK brick maps all 56 bits of
// the 7 bytes and T11nAddPilot drops the last four carriers: the stage makes the 52.
template <int NB>
__global__ void __launch_bounds__(256) k_mod11n_map(const uint8_t* __restrict__ in, uint32_t* __restrict__ out, int mod, uint32_t n)
{
    mod_map_tile<52, NB>(in, out, mod, n);
}
MOD_INSTANCES(k_mod11n_map, const uint8_t*, uint32_t*, int, uint32_t)

// ---- TSigMap11n: the 144 coded bits of L-SIG + HT-SIG, bytes 0..5 MapBPSK (+-30339 on I), bytes 6..17 MapQBPSK (+-30339 on Q).  A tile of 32 frames (576 bytes); a
// thread makes four carriers: 36 16-byte words per frame.
__global__ void __launch_bounds__(256) k_mod11n_sig_map(const uint8_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t n)
{
    __shared__ alignas(16) uint32_t s_in[kModTile * 18 / 4];
    const int tid = threadIdx.x;
    const uint32_t f0 = blockIdx.x * kModTile;
    const int nf = (int)min((uint32_t)kModTile, n - f0);
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

// ---- T11nAddPilot<iss>: mod_pilot_frames, 16 lanes per symbol; the 52 carriers arrive as thirteen 16-byte loads.  Data on bins 36..63 then 1..28 without +-7 and
// +-21; the pilots of the symbol at position n of its frame are tx_pilot11n(iss, n, k) at 43, 57, 7, 21; every other bin 0.
struct ModPilots11n {
    static constexpr int kCarriers = 52;
    int iss;
    static __device__ __forceinline__ int source(int b)                          // -1 - k = pilot k, -5 = zero
    {
        int src;
        if (b == 43) src = -1; else if (b == 57) src = -2; else if (b == 7) src = -3; else if (b == 21) src = -4;
        else if (b >= 1 && b <= 28) src = 26 + (b - 1) - (b > 7) - (b > 21);
        else if (b >= 36) src = b - 36 - (b > 43) - (b > 57);
        else src = -5;
        return src;
    }
    __device__ __forceinline__ uint32_t word(int kind, int, uint32_t j) const { return kind > -5 ? pack(mk(tx_pilot11n(iss, j, -1 - kind), 0)) : 0u; }
};
__global__ void __launch_bounds__(256) k_mod11n_add_pilot(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, const uint32_t* __restrict__ first,
        const uint32_t* __restrict__ nsym, const uint32_t* __restrict__ pos0, uint32_t nframes, int iss)
{
    mod_pilot_frames<16>(in, out, first, nsym, pos0, nframes, ModPilots11n{ iss });
}

// ---- TIFFTxOnly: mod_ifft_tiles from 64 bins to the 128 time samples as they are
__global__ void __launch_bounds__(256) k_mod11n_ifft(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t n, Tables T)
{
    mod_ifft_tiles<ModPlace64, ModEmitPlain>(in, out, n, T);
}

// ---- TCSD<ncsd>: output sample (i + 4 ncsd) mod 128 is input sample i -- 16-byte word (w + ncsd) mod 32 of a symbol is its input word w; a lane moves one word
__global__ void __launch_bounds__(256) k_mod11n_csd(const uint4* __restrict__ in, uint4* __restrict__ out, int ncsd, uint64_t nwords)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nwords) return;
    out[(i & ~(uint64_t)31) | ((i + (uint64_t)ncsd) & 31u)] = in[i];
}

// ---- TAddGI: mod_add_gi_word at the long guard interval, 40 words per symbol
__global__ void __launch_bounds__(256) k_mod11n_add_gi(const uint4* __restrict__ in, uint4* __restrict__ out, uint64_t nwords)
{
    mod_add_gi_word(in, out, 8u, nwords);
}

// ---- LSrc / HTSrc: mod_preamble_word from the table k_tx11n copies its fixed fields from ([2][1120] samples)
__global__ void __launch_bounds__(256) k_mod11n_preamble(const uint4* __restrict__ table, uint4* __restrict__ out0, uint4* __restrict__ out1, uint32_t w0, uint32_t nw,
        uint64_t nwords)
{
    mod_preamble_word(table, kTx11nPreamble / 4, out0, out1, w0, nw, nwords);
}

}  // namespace sora

using namespace sora;

// ---- the stage entry points (host_stage.h: the prologue and helpers every stage shares).  sora_hip_preamble11n stands beside sora_hip_tx11n, whose table it copies
int sora_hip_stream_parse11n(const uint8_t* d_in, uint8_t* d_out0, uint8_t* d_out1, int n_bpsc, size_t nsym, void* stream)
{
    STAGE_ENTRY("sora_hip_stream_parse11n", !d_in || !d_out0 || !d_out1, nsym)
    STAGE_NBPSC("sora_hip_stream_parse11n", n_bpsc)
    STAGE_ALIGNED16("sora_hip_stream_parse11n", d_in, d_out0, d_out1)
    const dim3 grid(stage_tiles(nsym, kModTile));
    STAGE_BY_NBPSC(n_bpsc, k_mod11n_parse, grid, (hipStream_t)stream, d_in, d_out0, d_out1, (uint32_t)nsym)
    return launch_result("k_mod11n_parse");
}

int sora_hip_interleave11n(const uint8_t* d_in, uint8_t* d_out, int n_bpsc, int spatial_stream, size_t nsym, void* stream)
{
    STAGE_ENTRY("sora_hip_interleave11n", !d_in || !d_out, nsym)
    STAGE_NBPSC("sora_hip_interleave11n", n_bpsc)
    STAGE_STREAM01("sora_hip_interleave11n", spatial_stream)
    STAGE_ALIGNED16("sora_hip_interleave11n", d_in, d_out)
    const dim3 grid(stage_tiles(nsym, kModTile));
    STAGE_BY_NBPSC(n_bpsc, k_mod11n_interleave, grid, (hipStream_t)stream, d_in, d_out, spatial_stream, (uint32_t)nsym)
    return launch_result("k_mod11n_interleave");
}

int sora_hip_map11n(const uint8_t* d_in, sora_complex16* d_out, int n_bpsc, int mod, size_t nsym, void* stream)
{
    STAGE_ENTRY("sora_hip_map11n", !d_in || !d_out, nsym)
    STAGE_NBPSC("sora_hip_map11n", n_bpsc)
    if (mod < 0 || mod > 32767) return sora_internal_fail(SORA_ERR_INVALID_PARAM, "sora_hip_map11n: mod must be 0 .. 32767", 0);
    STAGE_ALIGNED16("sora_hip_map11n", d_in, d_out)
    if (mod == 0) mod = n_bpsc == 1 ? 30339 : n_bpsc == 2 ? 21453 : n_bpsc == 4 ? 9594 : 4681;   // fb11nmod_config.hpp:121-128
    const dim3 grid(stage_tiles(nsym, kModTile));
    STAGE_BY_NBPSC(n_bpsc, k_mod11n_map, grid, (hipStream_t)stream, d_in, u32(d_out), mod, (uint32_t)nsym)
    return launch_result("k_mod11n_map");
}

int sora_hip_sig_map11n(const uint8_t* d_in, sora_complex16* d_out, size_t nframes, void* stream)
{
    STAGE_ENTRY("sora_hip_sig_map11n", !d_in || !d_out, nframes)
    STAGE_ALIGNED16("sora_hip_sig_map11n", d_in, d_out)
    hipLaunchKernelGGL(k_mod11n_sig_map, dim3(stage_tiles(nframes, kModTile)), dim3(256), 0, (hipStream_t)stream, d_in, u32(d_out), (uint32_t)nframes);
    return launch_result("k_mod11n_sig_map");
}

int sora_hip_add_pilot11n(const sora_complex16* d_in, sora_complex16* d_out, const uint32_t* d_first, const uint32_t* d_nsym, const uint32_t* d_pos0,
                          size_t nframes, int spatial_stream, void* stream)
{
    STAGE_ENTRY("sora_hip_add_pilot11n", !d_in || !d_out || !d_first || !d_nsym, nframes)
    STAGE_STREAM01("sora_hip_add_pilot11n", spatial_stream)
    STAGE_ALIGNED16("sora_hip_add_pilot11n", d_in, d_out)
    hipLaunchKernelGGL(k_mod11n_add_pilot, dim3((unsigned)nframes, stage_frame_grid(nframes)), dim3(256), 0, (hipStream_t)stream, u32(d_in), u32(d_out), d_first, d_nsym, d_pos0, (uint32_t)nframes,
                       spatial_stream);
    return launch_result("k_mod11n_add_pilot");
}

int sora_hip_ifft_only11n(const sora_complex16* d_in, sora_complex16* d_out, size_t nsym, void* stream)
{
    STAGE_ENTRY("sora_hip_ifft_only11n", !d_in || !d_out, nsym)
    STAGE_ALIGNED16("sora_hip_ifft_only11n", d_in, d_out)
    Tables T; if (const int rc = stage_tables(&T)) return rc;
    hipLaunchKernelGGL(k_mod11n_ifft, dim3(stage_tiles(nsym, kModIfftSyms)), dim3(256), 0, (hipStream_t)stream, u32(d_in), u32(d_out), (uint32_t)nsym, T);
    return launch_result("k_mod11n_ifft");
}

int sora_hip_csd11n(const sora_complex16* d_in, sora_complex16* d_out, int ncsd, size_t nsym, void* stream)
{
    STAGE_ENTRY("sora_hip_csd11n", !d_in || !d_out, nsym)
    if (ncsd < 1 || ncsd > 31) return sora_internal_fail(SORA_ERR_INVALID_PARAM, "sora_hip_csd11n: ncsd must be 1 .. 31", 0);
    if (d_in == d_out) return sora_internal_fail(SORA_ERR_INVALID_PARAM, "sora_hip_csd11n: out of place only", 0);
    STAGE_ALIGNED16("sora_hip_csd11n", d_in, d_out)
    const uint64_t nwords = (uint64_t)nsym * 32;
    hipLaunchKernelGGL(k_mod11n_csd, dim3(stage_tiles(nwords, 256)), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const uint4*>(d_in),
                       reinterpret_cast<uint4*>(d_out), ncsd, nwords);
    return launch_result("k_mod11n_csd");
}

int sora_hip_add_gi11n(const sora_complex16* d_in, sora_complex16* d_out, size_t nsym, void* stream)
{
    STAGE_ENTRY("sora_hip_add_gi11n", !d_in || !d_out, nsym)
    STAGE_ALIGNED16("sora_hip_add_gi11n", d_in, d_out)
    const uint64_t nwords = (uint64_t)nsym * 40;
    hipLaunchKernelGGL(k_mod11n_add_gi, dim3(stage_tiles(nwords, 256)), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const uint4*>(d_in),
                       reinterpret_cast<uint4*>(d_out), nwords);
    return launch_result("k_mod11n_add_gi");
}
