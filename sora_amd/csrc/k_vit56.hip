// k_vit56.hip -- the K=7 decoder at code rate 5/6 (SORA_CR_56: A1 B1 A2 B3 A4 B5 per five input bits; include/sora_hip.h): the kernel over a
// handle's FOURTH job list (k_viterbi56_11n, launched by trellis_launch56 of host_trellis.h), the same wave over a caller's arrays (k_viterbi56_11n_stage) and the stage
// entry point sora_hip_viterbi56_11n.  The window schedule is the 802.11n graph's T11aViterbi<.., 192, 36>; the layout is k_viterbi11n's (k_rx.hip): a wave holds the
// 64 states, two consecutive jobs of the list share it as 16-bit halves, four waves per workgroup with no traffic between them.  The forward pass is dev_vit56.h; the
// trellis kernels of the other three rates are not touched and never see such a job.
#include "kernels.h"
#include "dev_vit56.h"
#include "host_stage.h"

namespace sora {

namespace {
using F56 = VitForward56<192, 36>;
struct Job56 { uint32_t soft_off, nsoft, length, out_off; };                    // wave-uniform
// one wave: jobs A and B (B: any job when !hasB).  Nothing at or behind soft + span is read.
__device__ __forceinline__ void viterbi56_pair(const Job56& JA, const Job56& JB, bool hasB, const uint8_t* __restrict__ soft, uint32_t span, uint8_t* __restrict__ out)
{
    __shared__ uint16_t s_ring[4][F56::RG::kEntries];                           // 33 KB: survivor history, two copies of every block (RingGeom), per wave
    __shared__ __attribute__((aligned(16))) uint16_t s_ops[4][64];              // [wave][operand of the chunk][frame]
    auto side = [&](const Job56& J, bool has) {
        VitSide s;
        s.out = out + J.out_off; s.nsteps = has ? J.nsoft / F56::GB * F56::GS : 0u; s.tr_end = has ? J.length * 8u + 16u + 6u : 0u; s.done = s.nsteps == 0u;
        s.soft_off = J.soft_off; s.last = max(J.nsoft, 1u) - 1u; s.i0 = 0;
        return s;
    };
    const uint32_t w = threadIdx.x >> 6;
    F56 F;
    F.init(side(JA, true), side(JB, hasB), soft, span, s_ring[w], s_ops[w]);
    F.run();
}
}  // namespace

// The fourth list of a job table (host_trellis.h): njobs[3] jobs at jobs + 3 stride.  A wave beyond the list's pairs returns at once, so a launch over an empty list
// costs its dispatch.
__global__ void __launch_bounds__(256) k_viterbi56_11n(const VitJob* __restrict__ jobs, const uint32_t* __restrict__ njobs, uint32_t stride, const uint8_t* __restrict__ soft,
        uint32_t span, uint8_t* __restrict__ out)
{
    const uint32_t n = uni(njobs[3]), fa = uni((blockIdx.x * 4u + (threadIdx.x >> 6)) * 2u), fb = fa + 1u;
    if (fa >= n) return;
    jobs += 3 * (size_t)stride;
    auto load_job = [&](uint32_t f) { const VitJob& G = jobs[f]; return Job56{ uni(G.soft_off), uni(G.nsoft), uni(G.length), uni(G.out_off) }; };
    const bool hasB = fb < n;
    viterbi56_pair(load_job(fa), load_job(hasB ? fb : fa), hasB, soft, span, out);
}

// Job j of a stage call: nsoft[j] soft bytes at soft + soft_off[j] -> frame_len[j] + 2 decoded bytes at out + out_off[j].
__global__ void __launch_bounds__(256) k_viterbi56_11n_stage(const uint8_t* __restrict__ soft, uint32_t span, const uint32_t* __restrict__ soft_off,
        const uint32_t* __restrict__ nsoft, const uint16_t* __restrict__ frame_len, const uint32_t* __restrict__ out_off, uint32_t n, uint8_t* __restrict__ out)
{
    const uint32_t fa = uni((blockIdx.x * 4u + (threadIdx.x >> 6)) * 2u), fb = fa + 1u;
    if (fa >= n) return;
    auto load_job = [&](uint32_t f) { return Job56{ uni(soft_off[f]), uni(nsoft[f]), uni((uint32_t)frame_len[f]), uni(out_off[f]) }; };
    const bool hasB = fb < n;
    viterbi56_pair(load_job(fa), load_job(hasB ? fb : fa), hasB, soft, span, out);
}

}  // namespace sora

using namespace sora;

int sora_hip_viterbi56_11n(const uint8_t* d_soft, size_t soft_span_bytes, const uint32_t* d_soft_off, const uint32_t* d_nsoft, const uint16_t* d_frame_len,
                           uint8_t* d_out, const uint32_t* d_out_off, size_t n, void* stream)
{
    STAGE_ENTRY("sora_hip_viterbi56_11n", !d_soft || !d_soft_off || !d_nsoft || !d_frame_len || !d_out || !d_out_off, n)
    if (soft_span_bytes == 0) return sora_internal_fail(SORA_ERR_INVALID_PARAM, "sora_hip_viterbi56_11n: soft_span_bytes is 0", 0);
    if (soft_span_bytes >= (1ull << 32)) return sora_internal_fail(SORA_ERR_CAPACITY, "sora_hip_viterbi56_11n: batch too large", 0);
    hipLaunchKernelGGL(k_viterbi56_11n_stage, dim3(stage_tiles(n, 8)), dim3(256), 0, (hipStream_t)stream, d_soft, (uint32_t)soft_span_bytes, d_soft_off, d_nsoft, d_frame_len,
                       d_out_off, (uint32_t)n, d_out);
    return launch_result("k_viterbi56_11n_stage");
}
