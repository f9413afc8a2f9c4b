// k_11a.hip -- the front end of the 802.11a receive graph (CreateDemodGraph11a_40M, fb11ademod_config.hpp:169-232), brick by brick, as stage entry points
// (DESIGN.md section 7, f2b).  Everything behind them -- lts11a .. viterbi11a, desc11a, frame_sink11a -- are stages already.
//   k_11a_dc_remove            TDCRemoveEx<4>::Filter   (brick/inc/dc.hpp:46-86)        COMPLEX16 x 4  -> COMPLEX16 x 4     (k_11b_dc_remove's arithmetic)
//   k_11a_dc_estimate          TDCEstimator             (dc.hpp:99-165)                 COMPLEX16 x 4  -> (state)
//   k_11a_cca                  TCCA11a                  (Brick11/src/cca.hpp:104-441)   COMPLEX16 x 4  -> the gated bursts, (state)
//   k_11a_carrier_sense        TDCRemoveEx -> TCCA11a -> TDCEstimator, the loop closed  COMPLEX16 x 4  -> (state)
//   k_11a_data_symbol          T11aDataSymbol           (PHY_11a.hpp:361-430)           COMPLEX16 x 80 -> COMPLEX16 x 64
//   k_11a_viterbi_sig          T11aViterbiSig           (viterbi.hpp:8-49)              uchar x 48     -> uint
//   k_11a_plcp_parse           T11aPLCPParser           (PHY_11a.hpp:518-604)           uint           -> record
// The two carrier-sense kernels are one wave per stream, tiles of 64 bursts, one burst per lane and the next tile on its way.  While sync_state is no_energy the
// tile is worked position-parallel (dev_cs11a.h: cs11a_plain_span): every lane forms its burst's terms, the three windowed sums are wave prefix sums, the ballot of the
// carrier tests finds the next true one, and the bursts in front of it are consumed in closed form -- up to the estimator's next update in the fused form, behind which
// the estimate has changed and the pass is formed again (at most every eight gated bursts), or the burst that raises the time-out.  The events themselves -- a true
// carrier test with establish_sync, the locked phase with check_sync -- go burst by burst over a state every lane holds alike (cs11a_burst: the burst's words come out
// of the tile by v_readlane), with the lanes taking the sixteen cross-correlations, one pattern each.  The walk resumes from any record.
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "dev_11n.h"
#include "dev_cs11a.h"
#include "host_stage.h"

namespace sora {

__device__ __forceinline__ uint4 cs11a_fetch(const uint32_t* __restrict__ src, uint32_t b, uint32_t n)       // burst b of the stream, zero behind its end; no alignment
{
    if (b >= n) return uint4{ 0u, 0u, 0u, 0u };
    const uint32_t* p = src + 4 * (size_t)b;
    return uint4{ p[0], p[1], p[2], p[3] };
}

// ---- TDCRemoveEx<4>: a sample per lane.  The arithmetic is k_11b_dc_remove's (TDCRemove's sub); this one stops at max_n where a stream's d_n lies above it.
__global__ void __launch_bounds__(256) k_11a_dc_remove(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, const uint32_t* __restrict__ first, const uint32_t* __restrict__ nn,
        const uint32_t* __restrict__ out_first, const uint32_t* __restrict__ dc, uint32_t max_n)
{
    const uint32_t f = blockIdx.y, n = 4u * min(nn[f], max_n), d = dc[f];
    const uint32_t* s = in + first[f]; uint32_t* o = out + out_first[f];
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) o[i] = cs11a_sub16(s[i], d);
}

template <bool FUSED>
__device__ __forceinline__ void cs11a_walk(const uint32_t* __restrict__ in, const uint32_t* __restrict__ first, const uint32_t* __restrict__ nn, const uint32_t* __restrict__ out_first,
        uint32_t* __restrict__ state, uint32_t* __restrict__ out, uint32_t* __restrict__ used_out, uint32_t* __restrict__ npass_out, uint32_t max_n, uint32_t flags, const uint32_t* __restrict__ sts)
{
    const uint32_t f = blockIdx.x; const int lane = (int)threadIdx.x;
    uint32_t* st = state + (size_t)f * (FUSED ? kCs11aWords : kCca11aWords);
    const uint32_t n = min(nn[f], max_n);
    const uint32_t* src = in + first[f];
    uint32_t pat[16];
#pragma unroll
    for (int k = 0; k < 16; k++) pat[k] = sts[(lane & 15) * 16 + k];
    Cs11a S; cs11a_load(S, st, FUSED);
    const bool stop_on_timeout = (flags & SORA_CCA11A_STOP_ON_TIMEOUT) != 0;
    uint32_t used = 0, npass = 0;
    bool done = S.cca_state == 1u || n == 0;
    uint4 nxt = cs11a_fetch(src, (uint32_t)lane, done ? 0u : n);
    for (uint32_t t0 = 0; !done; t0 += 64) {
        const uint4 v = nxt;
        nxt = cs11a_fetch(src, t0 + 64 + (uint32_t)lane, n);
        const uint32_t nv = min(64u, n - t0);
        uint64_t gate = 0;
        for (uint32_t b = 0; b < nv; b++) {
            if (!S.sync) {                                     // the idle search: position-parallel up to the next event (dev_cs11a.h)
                bool hit, raised;
                const uint32_t e = cs11a_plain_span<FUSED>(S, v, b, nv, lane, hit, raised);
                if (e > b) gate |= (e == 64u ? ~0ull : (1ull << e) - 1ull) & ~((1ull << b) - 1ull);
                used += e - b; b = e;
                if (raised && stop_on_timeout) { done = true; break; }
                if (!hit) { b--; continue; }                   // behind a DC update or a raised time-out, or at the tile's end: the next pass
            }
            const int bl = (int)b;
            const uint32_t w[4] = { (uint32_t)__builtin_amdgcn_readlane((int)v.x, bl), (uint32_t)__builtin_amdgcn_readlane((int)v.y, bl),
                                    (uint32_t)__builtin_amdgcn_readlane((int)v.z, bl), (uint32_t)__builtin_amdgcn_readlane((int)v.w, bl) };
            bool raised;
            if (cs11a_burst<FUSED>(S, w, pat, raised)) gate |= 1ull << b;
            used++;
            if (S.cca_state == 1u || (raised && stop_on_timeout)) { done = true; break; }
        }
        if (!FUSED) {                                          // the bursts behind which sync_state is no_energy, compacted: what the brick hands to TDCEstimator
            if ((gate >> lane) & 1ull) {
                uint32_t* o = out + 4 * ((size_t)out_first[f] + npass + (uint32_t)__popcll(gate & ((1ull << lane) - 1ull)));
                o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
            }
            npass += (uint32_t)__popcll(gate);
        }
        if (t0 + 64 >= n) done = true;
    }
    if (lane == 0) {
        cs11a_store(S, st, FUSED);
        used_out[f] = used;
        if (!FUSED) npass_out[f] = npass;
    }
}

__global__ void __launch_bounds__(64) k_11a_cca(const uint32_t* __restrict__ in, const uint32_t* __restrict__ first, const uint32_t* __restrict__ n, const uint32_t* __restrict__ out_first,
        uint32_t* __restrict__ state, uint32_t* __restrict__ out, uint32_t* __restrict__ used, uint32_t* __restrict__ npass, uint32_t max_n, uint32_t flags, const uint32_t* __restrict__ sts)
{
    cs11a_walk<false>(in, first, n, out_first, state, out, used, npass, max_n, flags, sts);
}

__global__ void __launch_bounds__(64) k_11a_carrier_sense(const uint32_t* __restrict__ in, const uint32_t* __restrict__ first, const uint32_t* __restrict__ n, uint32_t* __restrict__ state,
        uint32_t* __restrict__ used, uint32_t max_n, uint32_t flags, const uint32_t* __restrict__ sts)
{
    cs11a_walk<true>(in, first, n, nullptr, state, nullptr, used, nullptr, max_n, flags, sts);
}

// ---- TDCEstimator: one wave per stream, a burst per lane.  The bursts' terms wrap at 16 bits, so a span's sum_dc is a difference of prefix sums; the updates
// (at most eight per 64 bursts) are walked over those.
__global__ void __launch_bounds__(64) k_11a_dc_estimate(const uint32_t* __restrict__ in, const uint32_t* __restrict__ first, const uint32_t* __restrict__ nn, uint32_t* __restrict__ state,
        uint32_t max_n)
{
    __shared__ uint32_t s_pre[64];
    const uint32_t f = blockIdx.x; const int lane = (int)threadIdx.x;
    uint32_t* st = state + (size_t)f * kDcEst11aWords;
    const uint32_t n = min(nn[f], max_n);
    const uint32_t* src = in + first[f];
    uint32_t cnt = st[0], sum = st[1], dc = st[2];
    for (uint32_t t0 = 0; t0 < n; t0 += 64) {
        const uint4 v = cs11a_fetch(src, t0 + (uint32_t)lane, n);
        const uint32_t p[4] = { v.x, v.y, v.z, v.w };
        uint32_t h = cs11a_dc_term(p);                                           // 0 behind the stream's end
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const uint32_t u = (uint32_t)__shfl_up((int)h, o); if (lane >= o) h = cs11a_add16(h, u); }
        wave_lds_sync();
        s_pre[lane] = h;
        wave_lds_sync();
        const uint32_t nv = min(64u, n - t0);
        uint32_t b = 0, base = 0;                                               // base: the prefix sum in front of burst b
        while (nv - b > cnt) {                                                   // burst b + cnt finds update_cnt == 0
            const uint32_t at = b + cnt, p1 = s_pre[at];
            sum = cs11a_add16(sum, cs11a_sub16(p1, base));
            dc = cs11a_add16(dc, cs11a_sra16(sum, 2));
            sum = 0; cnt = kCs11aDcInterval - 1u; base = p1; b = at + 1u;
        }
        sum = cs11a_add16(sum, cs11a_sub16(s_pre[nv - 1u], base)); cnt -= nv - b;
    }
    if (lane == 0) { st[0] = cnt; st[1] = sum; st[2] = dc; }
}

// ---- T11aDataSymbol: the cyclic prefix dropped (skip_cp = 8).  A thread moves four samples: one 16-byte load and store where both sides are 16-byte aligned.
__global__ void __launch_bounds__(256) k_11a_data_symbol(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, const uint32_t* __restrict__ first, const uint32_t* __restrict__ nsym,
        const uint32_t* __restrict__ out_first, uint32_t max_nsym)
{
    const uint32_t f = blockIdx.y, n = min(nsym[f], max_nsym);
    const size_t src = first[f], dst = (size_t)out_first[f] * 64;
    const bool vin = ((uintptr_t)(in + src) & 15) == 0, vout = ((uintptr_t)out & 15) == 0;
    for (uint32_t m = blockIdx.x * 256 + threadIdx.x; m < n * 16u; m += gridDim.x * 256) {
        const uint32_t k = m >> 4, j = m & 15u;
        const uint32_t* s = in + src + (size_t)k * 80 + 8 + 4 * j; uint32_t* d = out + dst + (size_t)k * 64 + 4 * j;
        const uint4 v = vin ? *reinterpret_cast<const uint4*>(s) : uint4{ s[0], s[1], s[2], s[3] };      // (80 k + 8 + 4 j samples keep the frame's alignment)
        if (vout) *reinterpret_cast<uint4*>(d) = v; else { d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w; }
    }
}

// ---- T11aViterbiSig: Viterbi_sig11 over 24 trellis steps and >> 6; a wave per SIGNAL symbol, a state per lane (dev_11n.h: viterbi_sig_wave)
__global__ void __launch_bounds__(256) k_11a_viterbi_sig(const uint8_t* __restrict__ soft, uint32_t* __restrict__ sig, uint32_t n)
{
    __shared__ uint8_t s_soft[4][48];
    __shared__ uint64_t s_dec[4][25];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint32_t i = blockIdx.x * 4 + w;
    if (i >= n) return;
    if (lane < 48) s_soft[w][lane] = soft[(size_t)i * 48 + lane];
    wave_lds_sync();
    const uint32_t v = (uint32_t)(viterbi_sig_wave<24>(s_soft[w], s_dec[w], lane) >> 6);
    if (lane == 0) sig[i] = v;
}

__global__ void __launch_bounds__(256) k_11a_plcp_parse(const uint32_t* __restrict__ sig, uint32_t* __restrict__ rec, uint32_t n)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    uint32_t r[5]; plcp_parse11a(sig[i], r);
#pragma unroll
    for (int k = 0; k < 5; k++) rec[5 * (size_t)i + k] = r[k];
}

}  // namespace sora

using namespace sora;

// ---- the stage entry points (host_stage.h: the prologue and helpers every stage shares)
static_assert(sizeof(sora_cca11a_state) == 4 * kCca11aWords && sizeof(sora_dcest11a_state) == 4 * kDcEst11aWords && sizeof(sora_cs11a_state) == 4 * kCs11aWords &&
              sizeof(sora_plcp11a_rec) == 20, "the 802.11a stage records are 32-bit words");
namespace {
inline uint32_t clamp_n(size_t max_n) { return max_n < (1u << 30) ? (uint32_t)max_n : (1u << 30); }
}  // namespace

int sora_hip_dc_remove11a(const sora_complex16* d_in, const uint32_t* d_first, const uint32_t* d_n, const uint32_t* d_out_first, const sora_complex16* d_dc,
                          sora_complex16* d_out, size_t nstreams, size_t max_n, void* stream)
{
    STAGE_ENTRY("sora_hip_dc_remove11a", !d_in || !d_first || !d_n || !d_out_first || !d_dc || !d_out, nstreams)
    if (max_n == 0) return SORA_OK;
    if (nstreams > 65535 || max_n >= (1u << 29)) return sora_internal_fail(SORA_ERR_CAPACITY, "sora_hip_dc_remove11a: at most 65535 streams of 2^29 bursts per call", 0);
    const uint32_t mn = clamp_n(max_n); const unsigned gx = (unsigned)((4ull * mn + 255) / 256);
    hipLaunchKernelGGL(k_11a_dc_remove, dim3(gx < 64 ? gx : 64, (unsigned)nstreams), dim3(256), 0, (hipStream_t)stream, u32(d_in),
                       u32(d_out), d_first, d_n, d_out_first, u32(d_dc), mn);
    return launch_result("k_11a_dc_remove");
}

int sora_hip_dc_estimate11a(const sora_complex16* d_in, const uint32_t* d_first, const uint32_t* d_n, sora_dcest11a_state* d_state, size_t nstreams, size_t max_n, void* stream)
{
    STAGE_ENTRY("sora_hip_dc_estimate11a", !d_in || !d_first || !d_n || !d_state, nstreams)
    if (max_n == 0) return SORA_OK;
    hipLaunchKernelGGL(k_11a_dc_estimate, dim3((unsigned)nstreams), dim3(64), 0, (hipStream_t)stream, u32(d_in), d_first, d_n, u32(d_state), clamp_n(max_n));
    return launch_result("k_11a_dc_estimate");
}

int sora_hip_cca11a(const sora_complex16* d_in, const uint32_t* d_first, const uint32_t* d_n, const uint32_t* d_out_first, sora_cca11a_state* d_state, sora_complex16* d_out,
                    uint32_t* d_used, uint32_t* d_npass, size_t nstreams, size_t max_n, unsigned flags, void* stream)
{
    STAGE_ENTRY("sora_hip_cca11a", !d_in || !d_first || !d_n || !d_out_first || !d_state || !d_out || !d_used || !d_npass, nstreams)
    if (flags & ~(unsigned)SORA_CCA11A_STOP_ON_TIMEOUT) return sora_internal_fail(SORA_ERR_INVALID_PARAM, "sora_hip_cca11a: unknown flag", 0);
    if (max_n == 0) return SORA_OK;
    Tables T; if (const int rc = stage_tables(&T)) return rc;
    hipLaunchKernelGGL(k_11a_cca, dim3((unsigned)nstreams), dim3(64), 0, (hipStream_t)stream, u32(d_in), d_first, d_n, d_out_first,
                       u32(d_state), u32(d_out), d_used, d_npass, clamp_n(max_n), (uint32_t)flags, T.sts);
    return launch_result("k_11a_cca");
}

int sora_hip_carrier_sense11a(const sora_complex16* d_in, const uint32_t* d_first, const uint32_t* d_n, sora_cs11a_state* d_state, uint32_t* d_used, size_t nstreams,
                              size_t max_n, unsigned flags, void* stream)
{
    STAGE_ENTRY("sora_hip_carrier_sense11a", !d_in || !d_first || !d_n || !d_state || !d_used, nstreams)
    if (flags & ~(unsigned)SORA_CCA11A_STOP_ON_TIMEOUT) return sora_internal_fail(SORA_ERR_INVALID_PARAM, "sora_hip_carrier_sense11a: unknown flag", 0);
    if (max_n == 0) return SORA_OK;
    Tables T; if (const int rc = stage_tables(&T)) return rc;
    hipLaunchKernelGGL(k_11a_carrier_sense, dim3((unsigned)nstreams), dim3(64), 0, (hipStream_t)stream, u32(d_in), d_first, d_n,
                       u32(d_state), d_used, clamp_n(max_n), (uint32_t)flags, T.sts);
    return launch_result("k_11a_carrier_sense");
}

int sora_hip_data_symbol11a(const sora_complex16* d_in, const uint32_t* d_first, const uint32_t* d_nsym, const uint32_t* d_out_first, sora_complex16* d_out, size_t nframes,
                            size_t max_nsym, void* stream)
{
    STAGE_ENTRY("sora_hip_data_symbol11a", !d_in || !d_first || !d_nsym || !d_out_first || !d_out, nframes)
    if (max_nsym == 0) return SORA_OK;
    if (nframes > 65535 || max_nsym > (1u << 27)) return sora_internal_fail(SORA_ERR_CAPACITY, "sora_hip_data_symbol11a: at most 65535 frames of 2^27 symbols per call", 0);
    const unsigned gx = (unsigned)((max_nsym * 16 + 255) / 256);
    hipLaunchKernelGGL(k_11a_data_symbol, dim3(gx < 64 ? gx : 64, (unsigned)nframes), dim3(256), 0, (hipStream_t)stream, u32(d_in),
                       u32(d_out), d_first, d_nsym, d_out_first, (uint32_t)max_nsym);
    return launch_result("k_11a_data_symbol");
}

int sora_hip_viterbi_sig11a(const uint8_t* d_soft, uint32_t* d_sig, size_t n, void* stream)
{
    STAGE_ENTRY("sora_hip_viterbi_sig11a", !d_soft || !d_sig, n)
    hipLaunchKernelGGL(k_11a_viterbi_sig, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, d_soft, d_sig, (uint32_t)n);
    return launch_result("k_11a_viterbi_sig");
}

int sora_hip_plcp_parse11a(const uint32_t* d_sig, sora_plcp11a_rec* d_rec, size_t n, void* stream)
{
    STAGE_ENTRY("sora_hip_plcp_parse11a", !d_sig || !d_rec, n)
    hipLaunchKernelGGL(k_11a_plcp_parse, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d_sig, u32(d_rec), (uint32_t)n);
    return launch_result("k_11a_plcp_parse");
}
