// k_mod.hip -- the bricks of the 802.11a modulation graph (kernel/bb/demod11/fb11amod_config.hpp:74-110) as stand-alone, batched stages, one C entry point each
// (include/sora_hip.h), with the reference bricks' port formats: bits packed in bytes, LSB first, as the pins carry them.
//   k_mod_scramble    T11aSc                         (Brick11/src/scramble.hpp:170-261)       uchar x 1 -> uchar x 1
//   k_mod_encode      TConvEncode_12 / _23 / _34     (conv_enc.hpp:18-330)                    uchar x 1 / 2 / 3 -> uchar x 2 / 3 / 4
//   k_mod_interleave  T11aInterleave*                (interleave.hpp:16-114)                  uchar x 6 N_BPSC -> the same
//   k_mod_map         TMap11a*<MOD>                  (mapper11a.hpp:8-300)                    uchar x 6 N_BPSC -> COMPLEX16 x 48
//   k_mod_add_pilot   T11aAddPilot<BPSK_MOD>         (pilot.hpp:30-118)                       COMPLEX16 x 48 -> COMPLEX16 x 64
//   k_mod_ifftx       TIFFTx                         (fft.hpp:7-61)                           COMPLEX16 x 64 -> COMPLEX16 x 160
//   k_mod_upsample    TUpsample40MTo44M              (sampling.hpp:8-32, 40MTo44M.hpp)        COMPLEX16 x 160 -> COMPLEX16 x 176
//   k_mod_pack16to8   TPackSample16to8               (brick/inc/stdbrick.hpp:415-445)         COMPLEX16 x 8 -> COMPLEX8 x 8
//   k_mod_preamble    TTS11aSrc                      (preamble11a.hpp:19-140)                 -> COMPLEX16 x 640
// The arithmetic is dev_tx.h's (what the fused transmitters run); here are the port formats and the streaming shape of k_stage.hip: a workgroup owns a tile of
// consecutive symbols, every access to a symbol buffer is a 16-byte-per-lane load or store of a contiguous tile, the reshuffling inside a symbol happens in LDS.  The tile
// shape and the bodies of the interleaver, the mapper, the pilot stage and the IFFT are dev_mod.h's, which the 802.11n and 40 MHz HT graphs instantiate too; here are this
// graph's widths and policies.  The byte-wide stages (scrambler, encoder) are one thread per output byte: every output bit is a closed form of its position.
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "dev_tx.h"
#include "dev_mod.h"
#include "host_stage.h"

namespace sora {

// ---- T11aSc: byte i of frame f = in ^ (the register after i + 1 steps), the register a phase of the period-127 cycle (tx_scramble); the tail byte keeps its two pad bits.
// chunks = workgroups per frame (the host's bound on the lengths / 256).
__global__ void __launch_bounds__(256) k_mod_scramble(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, const uint32_t* __restrict__ off, const uint32_t* __restrict__ len,
        const uint32_t* __restrict__ tail, const uint8_t* __restrict__ seed, uint32_t nframes, uint32_t chunks, Tables T)
{
    const uint32_t f = blockIdx.x / chunks, i = (blockIdx.x - f * chunks) * 256u + threadIdx.x;
    if (f >= nframes || i >= len[f]) return;
    const unsigned phase = T.scr_phase[seed[f] >> 1];                            // m_Reg = lut[m_Reg >> 1]: bit 0 of the stored register is never read
    const size_t at = (size_t)off[f] + i;
    unsigned c = in[at] ^ (phase == 255 ? 0u : T.scr_seq[(phase + 8u * (i % 127u)) % 127u]);
    if (tail && i == tail[f]) c &= 0xC0u;                                        // TAIL_SCRAMBLE
    out[at] = (uint8_t)c;
}

// ---- TConvEncode_*: the punctured coded stream packed LSB first IS the bricks' output (their tables shift the newest coded bit in at the top); output byte j holds coded
// bits 8 j .. 8 j + 7 of the frame, coded bit k = generator `which` at input bit il (tx_punct_offset), a xor of five of the seven input bits il - 6 .. il.  The eight bits
// of a byte span at most 6 input bits, so with the 6 before them and a byte's misalignment they lie in three input bytes.  Bursts of 1 / 2 / 3 bytes -> 2 / 3 / 4.
__global__ void __launch_bounds__(256) k_mod_encode(const uint8_t* __restrict__ in, const uint32_t* __restrict__ in_off, const uint32_t* __restrict__ len, int cr,
        uint8_t* __restrict__ out, const uint32_t* __restrict__ out_off, uint32_t nframes, uint32_t chunks)
{
    const uint32_t f = blockIdx.x / chunks, j = (blockIdx.x - f * chunks) * 256u + threadIdx.x;
    if (f >= nframes) return;
    const uint32_t bin = (uint32_t)cr + 1u, L = len[f], nin = L / bin * bin;     // bytes behind the last whole burst stay queued in the brick: no output
    if (j >= nin / bin * (bin + 1u)) return;
    const uint8_t* src = in + in_off[f];
    const uint32_t k0 = 8u * j;
    const int i0 = (int)(tx_punct_offset(cr, (int)k0, 0x80000000u) & 0x7FFFFFFFu) - 6, b0 = i0 >> 3;
    uint32_t w = 0;
#pragma unroll
    for (int t = 0; t < 3; t++) { const int b = b0 + t; if (b >= 0 && (uint32_t)b < nin) w |= (uint32_t)src[b] << (8 * t); }
    w >>= i0 - 8 * b0;                                                           // bit t = input bit i0 + t (0 before the frame: the register starts at 0)
    const uint32_t ga = (w >> 6) ^ (w >> 4) ^ (w >> 3) ^ (w >> 1) ^ w;           // bit d = generator A (133) at input bit i0 + 6 + d
    const uint32_t gb = (w >> 6) ^ (w >> 5) ^ (w >> 4) ^ (w >> 3) ^ w;           // generator B (171)
    unsigned o = 0;
#pragma unroll
    for (int b = 0; b < 8; b++) {
        const uint32_t p = tx_punct_offset(cr, (int)(k0 + b), 0x80000000u);
        const int d = (int)(p & 0x7FFFFFFFu) - 6 - i0;
        o |= ((((p >> 31) ? gb : ga) >> d) & 1u) << b;
    }
    out[(size_t)out_off[f] + j] = (uint8_t)o;
}

// ---- T11aInterleave*: bit k of a symbol goes to bit j(k) (T.deint holds j(k): the receiver's de-interleaver reads it the other way round): mod_interleave_tile
struct ModMap11a {
    static constexpr bool kOrsPadBits = false;                                   // 48 N_BPSC bits fill the row
    const uint16_t* row;                                                         // Tables::deint, one row of 288 per N_BPSC
    __device__ __forceinline__ int operator()(int k) const { return row[k]; }
};
template <int NB>
__global__ void __launch_bounds__(256) k_mod_interleave(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, uint32_t n, Tables T)
{
    constexpr int di = NB == 1 ? 0 : NB == 2 ? 1 : NB == 4 ? 2 : 3;
    mod_interleave_tile<48, NB>(in, out, n, ModMap11a{ T.deint + di * 288 });
}
MOD_INSTANCES(k_mod_interleave, const uint8_t*, uint8_t*, uint32_t, Tables)

// ---- TMap11a*<MOD>: mod_map_tile on the 48 carriers of a symbol's 6 N_BPSC bytes, 12 words per symbol
template <int NB>
__global__ void __launch_bounds__(256) k_mod_map(const uint8_t* __restrict__ in, uint32_t* __restrict__ out, int mod, uint32_t n)
{
    mod_map_tile<48, NB>(in, out, mod, n);
}
MOD_INSTANCES(k_mod_map, const uint8_t*, uint32_t*, int, uint32_t)

// ---- T11aAddPilot: mod_pilot_frames, 16 lanes per symbol; the 48 carriers arrive as twelve 16-byte loads.  The symbol at position j of its frame has polarity
// PilotSgn[127] for j = 0 and PilotSgn[(j - 1) mod 127] behind it: m_PilotIndex starts at 127 and wraps at 127.
struct ModPilots11a {
    static constexpr int kCarriers = 48;
    int mod;
    static __device__ __forceinline__ int source(int b)                          // -1 = a pilot, -2 = zero
    {
        if (b == 7 || b == 21 || b == 43 || b == 57) return -1;
        if (b >= 1 && b <= 26) return 24 + (b - 1) - (b > 7) - (b > 21);
        if (b >= 38) return b - 38 - (b > 43) - (b > 57);
        return -2;
    }
    __device__ __forceinline__ uint32_t word(int kind, int b, uint32_t j) const
    {
        const int p = pilot_sgn(j == 0 ? 127u : (j - 1u) % 127u) ? -mod : mod;
        return kind == -1 ? pack(mk(b == 21 ? -p : p, 0)) : 0u;
    }
};
__global__ void __launch_bounds__(256) k_mod_add_pilot(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, const uint32_t* __restrict__ first,
        const uint32_t* __restrict__ nsym, const uint32_t* __restrict__ pos0, uint32_t nframes, int mod)
{
    mod_pilot_frames<16>(in, out, first, nsym, pos0, nframes, ModPilots11a{ mod });
}

// ---- TIFFTx: mod_ifft_tiles from 64 bins to 160 samples, the guard interval in front and the window on its ends
__global__ void __launch_bounds__(256) k_mod_ifftx(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t n, Tables T)
{
    mod_ifft_tiles<ModPlace64, ModEmitGiWindow>(in, out, n, T);
}

// ---- TUpsample40MTo44M: y[11 m + r] = int16(mh(x[10 m + r - 1], S(r)) + mh(x[10 m + r], S(11 - r))) per 160-sample block, nothing carried between blocks (the closed form:
// sora_hip.h at sora_hip_tx11a44).  A tile of 8 blocks in LDS, 161 words each: x[160] is the next block's first sample where sees_next says so, else 0.
constexpr int kUpBlocks = 8;
__device__ __forceinline__ int mod_mulhrs(int a, int c) { return (__mul24(a, c) + 16384) >> 15; }   // _mm_mulhrs_epi16 (16-bit sample x 15-bit weight: a 24-bit multiply)
__global__ void __launch_bounds__(256) k_mod_upsample(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, const uint8_t* __restrict__ sees_next, uint32_t nblocks)
{
    __shared__ alignas(16) uint32_t s_x[kUpBlocks][164];
    const int tid = threadIdx.x;
    const uint32_t b0 = blockIdx.x * kUpBlocks;
    const int nb = (int)min((uint32_t)kUpBlocks, nblocks - b0);
    const uint4* in4 = reinterpret_cast<const uint4*>(in + (size_t)b0 * 160);
    for (int q = tid; q < nb * 40; q += 256) { const int blk = q / 40; reinterpret_cast<uint4*>(s_x[blk])[q - 40 * blk] = in4[q]; }
    if (tid < nb) {
        const uint32_t b = b0 + (uint32_t)tid;
        s_x[tid][160] = (sees_next && b + 1 < nblocks && sees_next[b]) ? in[(size_t)(b + 1) * 160] : 0u;
    }
    __syncthreads();
    // Lane t < 220 makes word w = t % 44 (outputs 4 w .. 4 w + 3) of blocks t / 44 and t / 44 + 5: which two inputs an output lies between and their weights depend on
    // w alone, so they are worked out once.
    if (tid >= 220) return;
    const int w = tid % 44;
    int ia[4], ib[4], cl[4], ch[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int j = 4 * w + k, m = j / 11, r = j - 11 * m;
        ib[k] = j - m; ia[k] = max(j - m - 1, 0);
        cl[k] = r * 32767 / 11; ch[k] = (11 - r) * 32767 / 11;
    }
    uint4* o4 = reinterpret_cast<uint4*>(out + (size_t)b0 * 176);
    for (int blk = tid / 44; blk < nb; blk += 5) {
        const uint32_t* x = s_x[blk];
        uint32_t y[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const cpx a = unpack(x[ia[k]]), c = unpack(x[ib[k]]);
            y[k] = pack(mk(mod_mulhrs(a.re, cl[k]) + mod_mulhrs(c.re, ch[k]), mod_mulhrs(a.im, cl[k]) + mod_mulhrs(c.im, ch[k])));         // (wraps like the brick's 16-bit add)
        }
        o4[blk * 44 + w] = uint4{y[0], y[1], y[2], y[3]};
    }
}

// ---- TPackSample16to8: _mm_packs_epi16 over bursts of 8 samples: a thread takes one burst, two 16-byte loads and one store
__device__ __forceinline__ uint32_t mod_sat8x2(uint32_t v)                       // COMPLEX16 -> COMPLEX8 in the low 16 bits
{
    const s16x2_t lo = { (short)-128, (short)-128 }, hi = { (short)127, (short)127 };
    const uint32_t c = __builtin_bit_cast(uint32_t, __builtin_elementwise_min(__builtin_elementwise_max(__builtin_bit_cast(s16x2_t, v), lo), hi));
    return (c & 0xFFu) | ((c >> 8) & 0xFF00u);
}
__global__ void __launch_bounds__(256) k_mod_pack16to8(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint64_t nbursts)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nbursts) return;
    const uint4 a = reinterpret_cast<const uint4*>(in)[2 * i], b = reinterpret_cast<const uint4*>(in)[2 * i + 1];
    reinterpret_cast<uint4*>(out)[i] = uint4{ mod_sat8x2(a.x) | (mod_sat8x2(a.y) << 16), mod_sat8x2(a.z) | (mod_sat8x2(a.w) << 16),
                                              mod_sat8x2(b.x) | (mod_sat8x2(b.y) << 16), mod_sat8x2(b.z) | (mod_sat8x2(b.w) << 16) };
}

// ---- TTS11aSrc: the 640 samples k_tx_preamble builds, in the 16 bits the source hands on (that kernel keeps them in LDS and writes their 8-bit form).  Every workgroup
// builds them (two IFFTs) and writes copies blockIdx.x, blockIdx.x + gridDim.x, ..
constexpr uint64_t mod_lts_bits()                                                // LTS_Positive_table (ieee80211const.h:23-28), entry i = bit i
{
    const int t[64] = { 0,1,0,0,1,1,0,1,0,1,0,0,0,0,0,1, 1,0,0,1,0,1,0,1,1,1,1,0,0,0,0,0, 0,0,0,0,0,0,1,1,0,0,1,1,0,1,0,1, 1,1,1,1,1,0,0,1,1,0,1,0,1,1,1,1 };
    uint64_t v = 0;
    for (int i = 0; i < 64; i++) v |= (uint64_t)t[i] << i;
    return v;
}
constexpr uint64_t kModLtsPos = mod_lts_bits();
__global__ void __launch_bounds__(64) k_mod_preamble(uint32_t* __restrict__ out, uint32_t ncopies, Tables T)
{
    constexpr int kMod = 10720;                                                  // bpsk_mod_11a
    __shared__ uint32_t s_f[2][128];
    __shared__ uint32_t s_t[2][128];
    __shared__ alignas(16) uint32_t s_lut[640];
    const int g = threadIdx.x >> 5, e = threadIdx.x & 31;
    auto sync = []() { __syncthreads(); };
    for (int i = e; i < 128; i += 32) s_f[g][i] = 0;
    sync();
    if (g == 0 && e < 12) {                                                      // short training symbol: 12 carriers
        const int m = (int)(uint16_t)(1.0 * kMod * 1.472);
        const int idx[12] = { 4, 8, 12, 16, 20, 24, 104, 108, 112, 116, 120, 124 };
        const int sg[12]  = { -1, -1, 1, 1, 1, 1, 1, -1, 1, -1, -1, 1 };
        const int v = w16(sg[e] * m); s_f[0][idx[e]] = pack(mk(v, v));
    }
    if (g == 1) {                                                                // long training symbol
        for (int i = 1 + e; i <= 26; i += 32) s_f[1][i] = pack(mk(((kModLtsPos >> i) & 1) ? kMod : -kMod, 0));
        for (int i = 64 - 26 + e; i < 64; i += 32) s_f[1][i + 64] = pack(mk(((kModLtsPos >> i) & 1) ? kMod : -kMod, 0));
    }
    sync();
    cpx x[4], y[4];
#pragma unroll
    for (int m = 0; m < 4; m++) x[m] = unpack(s_f[g][e + 32 * m]);
    fft128_group<true>(x, y, s_f[g], e, T, sync);
#pragma unroll
    for (int q = 0; q < 4; q++) s_t[g][e + 32 * q] = pack(sra(y[q], 4));
    sync();
    // STS: 128 samples repeated periodically over 320; LTS: GI2 (last 64 of the symbol) + two copies of 128; the first and last two samples of each half halved
    for (int i = threadIdx.x; i < 640; i += 64) {
        cpx v = unpack(i < 320 ? s_t[0][i & 127] : i < 384 ? s_t[1][64 + (i - 320)] : s_t[1][(i - 384) & 127]);
        if (i == 0 || i == 1 || i == 318 || i == 319 || i == 320 || i == 321 || i == 638 || i == 639) v = sra(v, 1);
        s_lut[i] = pack(v);
    }
    sync();
    for (uint32_t c = blockIdx.x; c < ncopies; c += gridDim.x) {
        uint4* o = reinterpret_cast<uint4*>(out + (size_t)c * 640);
        for (int q = threadIdx.x; q < 160; q += 64) o[q] = reinterpret_cast<const uint4*>(s_lut)[q];
    }
}

}  // namespace sora

using namespace sora;

// ---- the stage entry points (host_stage.h: the prologue and helpers every stage shares)
int sora_hip_scramble11a(const uint8_t* d_in, uint8_t* d_out, const uint32_t* d_off, const uint32_t* d_len, const uint32_t* d_tail, const uint8_t* d_seed,
                         size_t nframes, size_t max_len, void* stream)
{
    STAGE_ENTRY("sora_hip_scramble11a", !d_in || !d_out || !d_off || !d_len || !d_seed, nframes)
    if (max_len == 0) return SORA_OK;
    uint32_t chunks; unsigned grid;
    if (!stage_grid(nframes, max_len, &chunks, &grid)) return sora_internal_fail(SORA_ERR_CAPACITY, "sora_hip_scramble11a: nframes x max_len is too large for one call", 0);
    Tables T; if (const int rc = stage_tables(&T)) return rc;
    hipLaunchKernelGGL(k_mod_scramble, dim3(grid), dim3(256), 0, (hipStream_t)stream, d_in, d_out, d_off, d_len, d_tail, d_seed, (uint32_t)nframes, chunks, T);
    return launch_result("k_mod_scramble");
}

int sora_hip_conv_encode11a(const uint8_t* d_in, const uint32_t* d_in_off, const uint32_t* d_len, int code_rate, uint8_t* d_out, const uint32_t* d_out_off,
                            size_t nframes, size_t max_len, void* stream)
{
    STAGE_ENTRY("sora_hip_conv_encode11a", !d_in || !d_in_off || !d_len || !d_out || !d_out_off, nframes)
    if (code_rate != SORA_CR_12 && code_rate != SORA_CR_23 && code_rate != SORA_CR_34) return sora_internal_fail(SORA_ERR_INVALID_PARAM, "sora_hip_conv_encode11a: bad code rate", 0);
    if (max_len >= (1u << 27)) return sora_internal_fail(SORA_ERR_CAPACITY, "sora_hip_conv_encode11a: a frame of 128 MiB or more", 0);
    const size_t bin = (size_t)code_rate + 1, max_out = max_len / bin * (bin + 1);
    if (max_out == 0) return SORA_OK;
    uint32_t chunks; unsigned grid;
    if (!stage_grid(nframes, max_out, &chunks, &grid)) return sora_internal_fail(SORA_ERR_CAPACITY, "sora_hip_conv_encode11a: nframes x max_len is too large for one call", 0);
    hipLaunchKernelGGL(k_mod_encode, dim3(grid), dim3(256), 0, (hipStream_t)stream, d_in, d_in_off, d_len, code_rate, d_out, d_out_off, (uint32_t)nframes, chunks);
    return launch_result("k_mod_encode");
}

int sora_hip_interleave11a(const uint8_t* d_in, uint8_t* d_out, int n_bpsc, size_t nsym, void* stream)
{
    STAGE_ENTRY("sora_hip_interleave11a", !d_in || !d_out, nsym)
    STAGE_NBPSC("sora_hip_interleave11a", n_bpsc)
    STAGE_ALIGNED16("sora_hip_interleave11a", d_in, d_out)
    Tables T; if (const int rc = stage_tables(&T)) return rc;
    const dim3 grid(stage_tiles(nsym, kModTile));
    STAGE_BY_NBPSC(n_bpsc, k_mod_interleave, grid, (hipStream_t)stream, d_in, d_out, (uint32_t)nsym, T)
    return launch_result("k_mod_interleave");
}

int sora_hip_map11a(const uint8_t* d_in, sora_complex16* d_out, int n_bpsc, int mod, size_t nsym, void* stream)
{
    STAGE_ENTRY("sora_hip_map11a", !d_in || !d_out, nsym)
    STAGE_NBPSC("sora_hip_map11a", n_bpsc)
    if (mod < 0 || mod > 32767) return sora_internal_fail(SORA_ERR_INVALID_PARAM, "sora_hip_map11a: mod must be 0 .. 32767", 0);
    STAGE_ALIGNED16("sora_hip_map11a", d_in, d_out)
    if (mod == 0) mod = n_bpsc == 1 ? 10720 : n_bpsc == 2 ? (short)(10720 / 1.414) : n_bpsc == 4 ? (short)(10720 / 3.162) : (short)(10720 / 6.481);   // mapper11a.hpp:8-11
    const dim3 grid(stage_tiles(nsym, kModTile));
    STAGE_BY_NBPSC(n_bpsc, k_mod_map, grid, (hipStream_t)stream, d_in, u32(d_out), mod, (uint32_t)nsym)
    return launch_result("k_mod_map");
}

int sora_hip_add_pilot11a_from(const sora_complex16* d_in, sora_complex16* d_out, const uint32_t* d_first, const uint32_t* d_nsym, const uint32_t* d_pos0,
                               size_t nframes, int bpsk_mod, void* stream)
{
    STAGE_ENTRY("sora_hip_add_pilot11a", !d_in || !d_out || !d_first || !d_nsym, nframes)
    if (bpsk_mod < 0 || bpsk_mod > 32767) return sora_internal_fail(SORA_ERR_INVALID_PARAM, "sora_hip_add_pilot11a: bpsk_mod must be 0 .. 32767", 0);
    STAGE_ALIGNED16("sora_hip_add_pilot11a", d_in, d_out)
    hipLaunchKernelGGL(k_mod_add_pilot, dim3((unsigned)nframes, stage_frame_grid(nframes)), dim3(256), 0, (hipStream_t)stream, u32(d_in), u32(d_out), d_first, d_nsym, d_pos0, (uint32_t)nframes,
                       bpsk_mod ? bpsk_mod : 10720);
    return launch_result("k_mod_add_pilot");
}
int sora_hip_add_pilot11a(const sora_complex16* d_in, sora_complex16* d_out, const uint32_t* d_first, const uint32_t* d_nsym, size_t nframes, int bpsk_mod, void* stream)
{
    return sora_hip_add_pilot11a_from(d_in, d_out, d_first, d_nsym, nullptr, nframes, bpsk_mod, stream);
}

int sora_hip_ifftx11a(const sora_complex16* d_in, sora_complex16* d_out, size_t nsym, void* stream)
{
    STAGE_ENTRY("sora_hip_ifftx11a", !d_in || !d_out, nsym)
    STAGE_ALIGNED16("sora_hip_ifftx11a", d_in, d_out)
    Tables T; if (const int rc = stage_tables(&T)) return rc;
    hipLaunchKernelGGL(k_mod_ifftx, dim3(stage_tiles(nsym, kModIfftSyms)), dim3(256), 0, (hipStream_t)stream, u32(d_in), u32(d_out), (uint32_t)nsym, T);
    return launch_result("k_mod_ifftx");
}

int sora_hip_upsample40to44(const sora_complex16* d_in, sora_complex16* d_out, const uint8_t* d_sees_next, size_t nblocks, void* stream)
{
    STAGE_ENTRY("sora_hip_upsample40to44", !d_in || !d_out, nblocks)
    STAGE_ALIGNED16("sora_hip_upsample40to44", d_in, d_out)
    hipLaunchKernelGGL(k_mod_upsample, dim3(stage_tiles(nblocks, kUpBlocks)), dim3(256), 0, (hipStream_t)stream, u32(d_in), u32(d_out), d_sees_next, (uint32_t)nblocks);
    return launch_result("k_mod_upsample");
}

int sora_hip_pack16to8(const sora_complex16* d_in, int8_t* d_out, size_t nsamples, void* stream)
{
    // (counted in workgroups, 256 bursts of 8 samples each: what one launch is limited by; 0 exactly when nsamples is)
    STAGE_ENTRY("sora_hip_pack16to8", !d_in || !d_out, (nsamples + 2047) / 2048)
    if (nsamples % 8) return sora_internal_fail(SORA_ERR_INVALID_PARAM, "sora_hip_pack16to8: nsamples must be a multiple of 8 (the brick's burst)", 0);
    STAGE_ALIGNED16("sora_hip_pack16to8", d_in, d_out)
    const uint64_t nb = nsamples / 8;
    hipLaunchKernelGGL(k_mod_pack16to8, dim3(stage_tiles(nb, 256)), dim3(256), 0, (hipStream_t)stream, u32(d_in), u32(d_out), nb);
    return launch_result("k_mod_pack16to8");
}

int sora_hip_preamble11a(sora_complex16* d_out, size_t ncopies, void* stream)
{
    STAGE_ENTRY("sora_hip_preamble11a", !d_out, ncopies)
    if (!aligned16(d_out)) return sora_internal_fail(SORA_ERR_INVALID_PARAM, "sora_hip_preamble11a: the buffer must be 16-byte aligned", 0);
    Tables T; if (const int rc = stage_tables(&T)) return rc;
    hipLaunchKernelGGL(k_mod_preamble, dim3((unsigned)std::min<size_t>(ncopies, 2048)), dim3(64), 0, (hipStream_t)stream, u32(d_out), (uint32_t)ncopies, T);
    return launch_result("k_mod_preamble");
}
