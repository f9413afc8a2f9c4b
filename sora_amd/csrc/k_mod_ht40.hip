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
// The arithmetic is dev_tx.h's and dev_ht40.h's (what k_tx_ht40 runs: the levels and the pilot value are dev_ht40.h's, the SIG amplitude kernels.h's kTxHt40Amp); the
// tile shape and the bodies of the parser, the interleaver, the mapper, the pilot stage, the IFFT, the guard interval and the preamble copy are dev_mod.h's, which the
// 802.11a and 802.11n graphs instantiate too.  Here are this graph's widths and policies, and the two stages only it has: the interleaver on a contiguous stream and the
// SIG mapper.
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "dev_tx.h"
#include "dev_mod.h"
#include "dev_ht40.h"
#include "host_stage.h"

namespace sora {

// ---- the stream parser: mod_parse_tile, 108 carriers per stream (216 N_BPSC coded bits per symbol); BPSK's 14th byte carries four bits
template <int NB>
__global__ void __launch_bounds__(256) k_mod_ht40_parse(const uint8_t* __restrict__ in, uint8_t* __restrict__ out0, uint8_t* __restrict__ out1, uint32_t n)
{
    mod_parse_tile<108, NB>(in, out0, out1, n);
}
MOD_INSTANCES(k_mod_ht40_parse, const uint8_t*, uint8_t*, uint8_t*, uint32_t)

// ---- the HT interleaver for 40 MHz: mod_interleave_tile; bit k < 108 N_BPSC of a row goes to bit r(k) = deint40_index(N_BPSC, iss, k).  BPSK's input bits 108..111 are
// not read, its output bits 108..111 are 0.
template <int NB>
struct ModMapHt40 {
    static constexpr bool kOrsPadBits = false;
    int iss;
    __device__ __forceinline__ int operator()(int k) const { return deint40_index(NB, iss, k); }
};
template <int NB>
__global__ void __launch_bounds__(256) k_mod_ht40_interleave(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, int iss, uint32_t n)
{
    mod_interleave_tile<108, NB>(in, out, n, ModMapHt40<NB>{ iss });
}
MOD_INSTANCES(k_mod_ht40_interleave, const uint8_t*, uint8_t*, int, uint32_t)

// ---- the same map on a frame's contiguous coded stream: workgroup (f, y) takes passes of 32 symbols of frame f, y, y + gridDim.y, ..; symbol j reads bits 108 N_BPSC j
// onward of the stream at in + in_off[f] (any alignment; at BPSK an odd symbol starts mid-byte) and makes row first[f] + j of `out`.  A pass's input bits and its output
// rows are contiguous runs: tile_load_any / tile_store_any.  Rows that no frame owns are not written.
template <int NB>
__global__ void __launch_bounds__(256) k_mod_ht40_interleave_stream(const uint8_t* __restrict__ in, const uint32_t* __restrict__ in_off, const uint32_t* __restrict__ first,
        const uint32_t* __restrict__ nsym, uint8_t* __restrict__ out, int iss, uint32_t nframes)
{
    constexpr int NCB = 108 * NB, SB = mod_row(108, NB);
    __shared__ alignas(16) uint32_t s_in[(kModTile * NCB / 8 + 32) / 4];     // the pass's bits, a partial byte, the run's offset in its first 16-byte word
    __shared__ alignas(16) uint32_t s_out[(kModTile * SB + 16) / 4];
    __shared__ uint16_t s_inv[NCB];
    const uint32_t f = blockIdx.x;
    if (f >= nframes) return;
    const int tid = threadIdx.x;
    const uint32_t nf = nsym[f], sf = first[f];
    const uint8_t* src = in + in_off[f];
    mod_invert_map<NCB>(s_inv, ModMapHt40<NB>{ iss }, tid);
    for (uint32_t t0 = blockIdx.y * (uint32_t)kModTile; t0 < nf; t0 += gridDim.y * (uint32_t)kModTile) {   // (uniform per workgroup)
        const int ns = (int)min((uint32_t)kModTile, nf - t0);
        const uint64_t b0 = (uint64_t)NCB * t0;                                  // first bit of the pass in the frame's stream
        const uint8_t* g = src + (b0 >> 3);
        const int sub = (int)(b0 & 7u), nin = (sub + ns * NCB + 7) / 8;
        uint8_t* dst = out + ((size_t)sf + t0) * SB;
        const int nbytes = ns * SB, mo = tile_misalign(dst);
        __syncthreads();                                                         // the pass before has left LDS; s_inv is complete
        tile_load_any(s_in, g, nin, tid);
        __syncthreads();
        const uint32_t bit0 = 8u * (uint32_t)tile_misalign(g) + (uint32_t)sub;
        for (int q = tid; q < nbytes; q += 256) {                                // row q / SB of the pass, positions 8 (q % SB) .. + 7
            const int sym = q / SB, p0 = 8 * (q - sym * SB);
            reinterpret_cast<uint8_t*>(s_out)[mo + q] = (uint8_t)mod_interleave_byte<NCB>(reinterpret_cast<const uint8_t*>(s_in), s_inv, p0, 0, bit0 + (uint32_t)sym * NCB);
        }
        __syncthreads();
        tile_store_any(dst, s_out, nbytes, tid);
    }
}
MOD_INSTANCES(k_mod_ht40_interleave_stream, const uint8_t*, const uint32_t*, const uint32_t*, const uint32_t*, uint8_t*, int, uint32_t)

// ---- the mapper: mod_map_tile on the 108 carriers of a symbol's row at d = level40(N_BPSC), 27 words per symbol
template <int NB>
__global__ void __launch_bounds__(256) k_mod_ht40_map(const uint8_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t n)
{
    mod_map_tile<108, NB>(in, out, level40(NB), n);
}
MOD_INSTANCES(k_mod_ht40_map, const uint8_t*, uint32_t*, uint32_t)

// ---- L-SIG + HT-SIG: the 144 interleaved bits of a frame -> three complete symbols of 128 bins.  Position c < 48 of symbol s sits at legacy carrier leg(c) (-26..26
// without 0, +-7, +-21: carrier_bin48), +-16384 on I (s = 0, L-SIG) or Q (HT-SIG); the pilots +, +, +, - x 16384 on I at -21, -7, 7, 21; legacy carrier k goes to bin k - 32
// as it is and to bin k + 32 times j (k_tx_ht40.hip: put_dup40, leg_carrier).  A tile of 32 frames (576 bytes); a thread makes four bins in a row: 96 words per frame.
__global__ void __launch_bounds__(256) k_mod_ht40_sig_map(const uint8_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t n)
{
    __shared__ alignas(16) uint32_t s_in[kModTile * 18 / 4];
    const int tid = threadIdx.x;
    const uint32_t f0 = blockIdx.x * kModTile;
    const int nf = (int)min((uint32_t)kModTile, n - f0);
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
                if (k == -21 || k == -7 || k == 7 || k == 21) re = k == 21 ? -kTxHt40Amp : kTxHt40Amp;
                else {
                    const int c = k < 0 ? (k + 26) - (k > -21) - (k > -7) : 24 + (k - 1) - (k > 7) - (k > 21);
                    const int a = tx_gen_bit(s_in, (uint32_t)(144 * fr + 48 * s + c)) ? kTxHt40Amp : -kTxHt40Amp;
                    if (s == 0) re = a; else im = a;
                }
            }
            v[t] = upper ? pack(mk(-im, re)) : pack(mk(re, im));
        }
        o4[q] = uint4{v[0], v[1], v[2], v[3]};
    }
}

// ---- data carriers and pilots onto the 128 bins: mod_pilot_frames, 32 lanes per symbol; the 108 carriers arrive as 27 16-byte loads.  Data carrier c at
// data_bin40(c) (carriers -58..-2 and 2..58 without the pilots'), pilots (kPilot40, 0) at carriers +-11, +-25, +-53 whatever the symbol's position (k_tx_ht40.hip's
// symbol loop), the 14 other bins 0.
struct ModPilotsHt40 {
    static constexpr int kCarriers = 108;
    static __device__ __forceinline__ int source(int b)                          // -1 = pilot, -2 = zero
    {
        const int k = b < 64 ? b : b - 128, a = k < 0 ? -k : k;
        if (a == 11 || a == 25 || a == 53) return -1;
        if (a < 2 || a > 58) return -2;
        return k < 0 ? (k + 58) - (k > -53) - (k > -25) - (k > -11) : 54 + (k - 2) - (k > 11) - (k > 25) - (k > 53);
    }
    __device__ __forceinline__ uint32_t word(int kind, int, uint32_t) const { return kind == -1 ? pack(mk(kPilot40, 0)) : 0u; }
};
__global__ void __launch_bounds__(256) k_mod_ht40_add_pilot(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, const uint32_t* __restrict__ first,
        const uint32_t* __restrict__ nsym, uint32_t nframes)
{
    mod_pilot_frames<32>(in, out, first, nsym, nullptr, nframes, ModPilotsHt40{});
}

// ---- IFFT<128> of 128 bins in natural order: mod_ifft_tiles to the 128 time samples as they are
__global__ void __launch_bounds__(256) k_mod_ht40_ifft(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t n, Tables T)
{
    mod_ifft_tiles<ModPlace128, ModEmitPlain>(in, out, n, T);
}

// ---- the guard interval: mod_add_gi_word at the frame's cp (8: long, 160 samples; 4: short, 144)
__global__ void __launch_bounds__(256) k_mod_ht40_add_gi(const uint4* __restrict__ in, uint4* __restrict__ out, uint32_t cp, uint64_t nwords)
{
    mod_add_gi_word(in, out, cp, nwords);
}

// ---- the fixed fields: mod_preamble_word from the table k_tx_ht40_preamble builds ([2][1120] samples)
__global__ void __launch_bounds__(256) k_mod_ht40_preamble(const uint4* __restrict__ table, uint4* __restrict__ out0, uint4* __restrict__ out1, uint32_t w0, uint32_t nw,
        uint64_t nwords)
{
    mod_preamble_word(table, kTxHt40Preamble / 4, out0, out1, w0, nw, nwords);
}

}  // namespace sora

using namespace sora;

// ---- the stage entry points (host_stage.h: the prologue and helpers every stage shares).  As the receive stages of this graph do (k_ht40_stages.hip), a bad n_bpsc,
// spatial_stream or gi is refused before the count is looked at.  sora_hip_preamble_ht40 stands beside sora_hip_tx_ht40, whose table it copies.
int sora_hip_stream_parse_ht40(const uint8_t* d_in, uint8_t* d_out0, uint8_t* d_out1, int n_bpsc, size_t nsym, void* stream)
{
    STAGE_NBPSC("sora_hip_stream_parse_ht40", n_bpsc)
    STAGE_ENTRY("sora_hip_stream_parse_ht40", !d_in || !d_out0 || !d_out1, nsym)
    STAGE_ALIGNED16("sora_hip_stream_parse_ht40", d_in, d_out0, d_out1)
    const dim3 grid(stage_tiles(nsym, kModTile));
    STAGE_BY_NBPSC(n_bpsc, k_mod_ht40_parse, grid, (hipStream_t)stream, d_in, d_out0, d_out1, (uint32_t)nsym)
    return launch_result("k_mod_ht40_parse");
}

int sora_hip_interleave_ht40(const uint8_t* d_in, uint8_t* d_out, int n_bpsc, int spatial_stream, size_t nsym, void* stream)
{
    STAGE_NBPSC("sora_hip_interleave_ht40", n_bpsc)
    STAGE_STREAM01("sora_hip_interleave_ht40", spatial_stream)
    STAGE_ENTRY("sora_hip_interleave_ht40", !d_in || !d_out, nsym)
    STAGE_ALIGNED16("sora_hip_interleave_ht40", d_in, d_out)
    const dim3 grid(stage_tiles(nsym, kModTile));
    STAGE_BY_NBPSC(n_bpsc, k_mod_ht40_interleave, grid, (hipStream_t)stream, d_in, d_out, spatial_stream, (uint32_t)nsym)
    return launch_result("k_mod_ht40_interleave");
}

int sora_hip_interleave_ht40_stream(const uint8_t* d_in, const uint32_t* d_in_off, const uint32_t* d_first, const uint32_t* d_nsym, uint8_t* d_out, int n_bpsc,
                                    int spatial_stream, size_t nframes, void* stream)
{
    STAGE_NBPSC("sora_hip_interleave_ht40_stream", n_bpsc)
    STAGE_STREAM01("sora_hip_interleave_ht40_stream", spatial_stream)
    STAGE_ENTRY("sora_hip_interleave_ht40_stream", !d_in || !d_in_off || !d_first || !d_nsym || !d_out, nframes)
    if (!aligned16(d_out)) return sora_internal_fail(SORA_ERR_INVALID_PARAM, "sora_hip_interleave_ht40_stream: d_out must be 16-byte aligned", 0);
    const dim3 grid((unsigned)nframes, stage_frame_grid(nframes));
    STAGE_BY_NBPSC(n_bpsc, k_mod_ht40_interleave_stream, grid, (hipStream_t)stream, d_in, d_in_off, d_first, d_nsym, d_out, spatial_stream, (uint32_t)nframes)
    return launch_result("k_mod_ht40_interleave_stream");
}

int sora_hip_map_ht40(const uint8_t* d_in, sora_complex16* d_out, int n_bpsc, size_t nsym, void* stream)
{
    STAGE_NBPSC("sora_hip_map_ht40", n_bpsc)
    STAGE_ENTRY("sora_hip_map_ht40", !d_in || !d_out, nsym)
    STAGE_ALIGNED16("sora_hip_map_ht40", d_in, d_out)
    const dim3 grid(stage_tiles(nsym, kModTile));
    STAGE_BY_NBPSC(n_bpsc, k_mod_ht40_map, grid, (hipStream_t)stream, d_in, u32(d_out), (uint32_t)nsym)
    return launch_result("k_mod_ht40_map");
}

int sora_hip_sig_map_ht40(const uint8_t* d_in, sora_complex16* d_out, size_t nframes, void* stream)
{
    STAGE_ENTRY("sora_hip_sig_map_ht40", !d_in || !d_out, nframes)
    STAGE_ALIGNED16("sora_hip_sig_map_ht40", d_in, d_out)
    hipLaunchKernelGGL(k_mod_ht40_sig_map, dim3(stage_tiles(nframes, kModTile)), dim3(256), 0, (hipStream_t)stream, d_in, u32(d_out),
                       (uint32_t)nframes);
    return launch_result("k_mod_ht40_sig_map");
}

int sora_hip_add_pilot_ht40(const sora_complex16* d_in, sora_complex16* d_out, const uint32_t* d_first, const uint32_t* d_nsym, size_t nframes, void* stream)
{
    STAGE_ENTRY("sora_hip_add_pilot_ht40", !d_in || !d_out || !d_first || !d_nsym, nframes)
    STAGE_ALIGNED16("sora_hip_add_pilot_ht40", d_in, d_out)
    hipLaunchKernelGGL(k_mod_ht40_add_pilot, dim3((unsigned)nframes, stage_frame_grid(nframes)), dim3(256), 0, (hipStream_t)stream, u32(d_in), u32(d_out), d_first, d_nsym, (uint32_t)nframes);
    return launch_result("k_mod_ht40_add_pilot");
}

int sora_hip_ifft_ht40(const sora_complex16* d_in, sora_complex16* d_out, size_t nsym, void* stream)
{
    STAGE_ENTRY("sora_hip_ifft_ht40", !d_in || !d_out, nsym)
    STAGE_ALIGNED16("sora_hip_ifft_ht40", d_in, d_out)
    Tables T; if (const int rc = stage_tables(&T)) return rc;
    hipLaunchKernelGGL(k_mod_ht40_ifft, dim3(stage_tiles(nsym, kModIfftSyms)), dim3(256), 0, (hipStream_t)stream, u32(d_in), u32(d_out), (uint32_t)nsym, T);
    return launch_result("k_mod_ht40_ifft");
}

int sora_hip_add_gi_ht40(const sora_complex16* d_in, sora_complex16* d_out, int gi, size_t nsym, void* stream)
{
    if (gi != 0 && gi != 1) return sora_internal_fail(SORA_ERR_INVALID_PARAM, "sora_hip_add_gi_ht40: gi must be 0 (long) or 1 (short)", 0);
    STAGE_ENTRY("sora_hip_add_gi_ht40", !d_in || !d_out, nsym)
    STAGE_ALIGNED16("sora_hip_add_gi_ht40", d_in, d_out)
    const uint32_t cp = gi ? kHt40ShortCp / 4 : 8u;
    const uint64_t nwords = (uint64_t)nsym * (32u + cp);
    hipLaunchKernelGGL(k_mod_ht40_add_gi, dim3(stage_tiles(nwords, 256)), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const uint4*>(d_in),
                       reinterpret_cast<uint4*>(d_out), cp, nwords);
    return launch_result("k_mod_ht40_add_gi");
}
