// host_trellis.h -- host side of the K=7 decoder over a job table: which trellis kernel a call launches, with which grid, over which scratch arrays.  The kinds
// and their spelling in the ABI (lanes_per_pair), the launch geometry the kernels work out again on the device (dev_winplan.h), the window-parallel form's scratch
// arrays and the one function that enqueues the kernels.  Every handle and both stage entry points come through here.  Host code only.
#pragma once
#include <algorithm>
#include <optional>
#include "host_calls.h"
#include "kernels.h"
#include "dev_winplan.h"

namespace sora {

// ---- the kind
// Lanes64: k_viterbi / k_viterbi11n, 64 lanes per frame pair (k_rx.hip); Lanes16: k_viterbi16 / k_viterbi16_11n, 16 lanes per pair (k_vit16.hip);
// Windowed: k_viterbi16w* and behind it the proof k_win_redo*, which decodes serially what fails it (k_vitwin.hip)
enum class Trellis { Lanes64, Lanes16, Windowed };
// What a handle was told (*_set_trellis): a kind, or (no value) to choose by a policy of its own
using TrellisChoice = std::optional<Trellis>;
inline int trellis_abi(Trellis t) { return t == Trellis::Lanes16 ? 16 : t == Trellis::Windowed ? SORA_TRELLIS_WINDOWED : 64; }
inline int trellis_abi(const TrellisChoice& c) { return c ? trellis_abi(*c) : 0; }
// lanes_per_pair of an entry point: 0 (automatic), 16, 64 or SORA_TRELLIS_WINDOWED -> *out, else false
inline bool trellis_parse(int lanes_per_pair, TrellisChoice* out)
{
    if (lanes_per_pair == 0) *out = std::nullopt;
    else if (lanes_per_pair == 16) *out = Trellis::Lanes16;
    else if (lanes_per_pair == 64) *out = Trellis::Lanes64;
    else if (lanes_per_pair == SORA_TRELLIS_WINDOWED) *out = Trellis::Windowed;
    else return false;
    return true;
}

// ---- the geometry.  k_viterbi16w* and the proof kernels work the unit plan out again from (jobs, target, vstride): these are the host's half of that contract.
// units a call of the window-parallel trellis is cut into at least, frames permitting: one round of the chip's 2048 eight-unit trellis slots
constexpr uint32_t kWinUnitsTarget = 16384;
// waves a call may need on top of its units' eight per wave: a code-rate list of ONE frame is laid out with gaps (dev_winplan.h)
constexpr uint32_t kWinLoneWaves = 3 * kWinLonePad / 8;
// the window-parallel trellis of a call of `rows` frame rows: the units it is cut into at most (a frame has at most kWinMaxUnits windows) ...
inline uint64_t win_units(uint64_t rows) { return std::min<uint64_t>(std::max<uint64_t>(kWinUnitsTarget, rows), (uint64_t)kWinMaxUnits * rows); }
// ... its waves: eight units each, + a partly filled one per code-rate list + the lone layout's gaps
inline uint64_t win_waves(uint64_t rows) { return (win_units(rows) + 7) / 8 + 3 + kWinLoneWaves; }
// ... and its vectors per code-rate list (a call is cut into at most max(target, rows) units and a frame into at most 80: a single-capture handle needs 80 vectors
// per row, not the target's number)
inline uint32_t win_vstride(uint64_t rows) { return (uint32_t)(win_units(rows) + rows); }

// The job table a launch works over: three code-rate lists of `stride` jobs each behind a header of their three counts, holding at most n jobs together (a handle's
// call), or ONE list of exactly n jobs (the stage entry points: the serial kernels take n itself and no header; the windowed form reads hdr = {n, 0, 0}).
// packed3 (WIN = 256 only): the streams are the three-bit ones sora_hip_viterbi11a* packs into its caller's workspace, not a receive handle's pre-scaled bytes in its
// padded array (rx_types.h) -- the *_p3 instantiations of the same kernels, which clamp every fetch.
struct TrellisJobs { const VitJob* jobs; const uint32_t* hdr; uint32_t n, stride; bool single, packed3; };
inline TrellisJobs trellis_lists(const VitJob* jobs, const uint32_t* hdr, uint32_t n, uint32_t stride) { return TrellisJobs{ jobs, hdr, n, stride, false, false }; }
inline TrellisJobs trellis_single(const VitJob* jobs, const uint32_t* hdr, uint32_t n, bool packed3) { return TrellisJobs{ jobs, hdr, n, n, true, packed3 }; }
// workgroups of the kernels that take PAIRS of frames, four pairs each (k_viterbi*, k_win_redo*): at most ceil(n / 2) + 2 pairs over three lists, ceil(n / 2) of one
inline uint32_t trellis_pair_groups(const TrellisJobs& J) { return J.single ? (J.n + 7) / 8 : (J.n / 2 + 3 + 3) / 4; }
// one-wave workgroups of k_viterbi16*, eight frames each: at most ceil(n / 8) + 2 waves over three lists
inline uint32_t trellis_waves16(const TrellisJobs& J) { return (J.n + 7) / 8 + (J.single ? 0u : 2u); }
// one-wave workgroups of k_viterbi16w*, eight units each (one list: the slots of the plan itself, the lone layout's included)
inline uint32_t trellis_win_waves(const TrellisJobs& J)
{
    return J.single ? (win_slots(J.n, win_units_per_frame(J.n, kWinUnitsTarget)) + 7) / 8 : (uint32_t)win_waves(J.n);
}

// ---- the window-parallel trellis's scratch: the units' verification vectors (three code-rate lists of `stride` vectors) and the proof's record, kWinStatBanks banks
// of {boundaries compared, boundaries that differed, frames decoded again, units}.  One more counter follows the banks: the calls whose data field the 802.11a handle's
// k_win_redo_finish_pipe made again.  A handle's pipeline owns one (ensure / free); the stage entry points lay one over the caller's workspace (stride = win_vstride(n)).
constexpr size_t kWinStatsBytes = 4 * kWinStatBanks * sizeof(unsigned long long);
struct WinScratch {
    uint16_t* d_vecs = nullptr; unsigned long long* d_stats = nullptr; uint32_t stride = 0;

    unsigned long long* redone() const { return d_stats + kWinStatsBytes / sizeof(unsigned long long); }   // the counter behind the banks
    // On first use by a pipeline of a handle of cap_rows frame rows: the arrays, the counters zero.  Call it outside stream capture and before the launch.  The
    // counters are zeroed on zero_on, in front of the caller's kernels there, or (nullptr) before this returns; extra: the counter behind the banks as well.
    int ensure(uint64_t cap_rows, hipStream_t zero_on, bool extra)
    {
        if (d_vecs) return SORA_OK;
        stride = win_vstride(cap_rows);
        HIPCHK(hipMalloc((void**)&d_vecs, 3 * (size_t)kWinVecBytes * stride));
        HIPCHK(hipMalloc((void**)&d_stats, kWinStatsBytes + sizeof(unsigned long long)));
        const size_t bytes = kWinStatsBytes + (extra ? sizeof(unsigned long long) : 0);
        if (zero_on) HIPCHK(hipMemsetAsync(d_stats, 0, bytes, zero_on));
        else HIPCHK(hipMemset(d_stats, 0, bytes));
        return SORA_OK;
    }
    void free() { (void)hipFree(d_vecs); (void)hipFree(d_stats); d_vecs = nullptr; d_stats = nullptr; stride = 0; }
};
// out[4] += the record at d_stats, behind everything enqueued on st
inline int win_stats_add(const unsigned long long* d_stats, hipStream_t st, unsigned long long out[4])
{
    unsigned long long v[4 * kWinStatBanks];
    HIPCHK(hipMemcpyAsync(v, d_stats, sizeof v, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (unsigned i = 0; i < 4 * kWinStatBanks; i++) out[i & 3u] += v[i];
    return SORA_OK;
}
// *_window_stats of a handle: out[4] <- the records of its pipelines s[0, n) since its creation
template <typename P> inline int win_stats_sum(P* const* s, int n, int device, unsigned long long out[4])
{
    HIPCHK(hipSetDevice(device));
    for (int i = 0; i < 4; i++) out[i] = 0;
    for (int i = 0; i < n; i++) if (s[i] && s[i]->win.d_stats) { const int rc = win_stats_add(s[i]->win.d_stats, s[i]->stream, out); if (rc) return rc; }
    return SORA_OK;
}

// ---- the launch.  WIN names the decoder: 256 = the 802.11a graph's T11aViterbi<5000*8,48,256,24>, 192 = the 802.11n graph's T11aViterbi<5000*8,312,192,36>.
// The proof of the window-parallel trellis over J, and the serial decode of the pairs of frames that fail it (none, normally: its waves check and return)
template <int WIN> inline void trellis_proof(const TrellisJobs& J, const uint8_t* soft, uint8_t* out, const WinScratch& W, hipStream_t st)
{
    static_assert(WIN == 256 || WIN == 192, "the 802.11a (256) or the 802.11n (192) window schedule");
    if constexpr (WIN == 256)
        hipLaunchKernelGGL(J.packed3 ? k_win_redo_p3 : k_win_redo, dim3(trellis_pair_groups(J)), dim3(256), 0, st, J.jobs, J.hdr, J.stride, kWinUnitsTarget, W.stride,
                           (const uint16_t*)W.d_vecs, soft, out, W.d_stats);
    else
        hipLaunchKernelGGL(k_win_redo_11n, dim3(trellis_pair_groups(J)), dim3(256), 0, st, J.jobs, J.hdr, J.stride, kWinUnitsTarget, W.stride, (const uint16_t*)W.d_vecs, soft, out, W.d_stats);
}
// The trellis of kind `kind` over J on stream st: soft values at soft + VitJob::soft_off, decoded bytes to out + VitJob::out_off.  Windowed: W is the scratch (a
// handle's: ensure() has run), and proof = false leaves the proof to the caller (the 802.11a handle fuses it with its finisher).  The serial kinds need no W.
template <int WIN> inline void trellis_launch(Trellis kind, const TrellisJobs& J, const uint8_t* soft, uint8_t* out, hipStream_t st, const WinScratch& W = WinScratch(),
        bool proof = true)
{
    static_assert(WIN == 256 || WIN == 192, "the 802.11a (256) or the 802.11n (192) window schedule");
    const uint32_t* hdr = J.single ? nullptr : J.hdr;
    const uint32_t n1 = J.single ? J.n : 0u, stride = J.single ? 0u : J.stride;    // (the serial kernels: a header and a stride, or a count)
    if (kind == Trellis::Windowed) {
        if constexpr (WIN == 256)
            hipLaunchKernelGGL(J.packed3 ? k_viterbi16w_p3 : k_viterbi16w, dim3(trellis_win_waves(J)), dim3(64), 0, st, J.jobs, J.hdr, J.stride, kWinUnitsTarget, W.stride, soft, out,
                               W.d_vecs);
        else hipLaunchKernelGGL(k_viterbi16w_11n, dim3(trellis_win_waves(J)), dim3(64), 0, st, J.jobs, J.hdr, J.stride, kWinUnitsTarget, W.stride, soft, out, W.d_vecs);
        if (proof) trellis_proof<WIN>(J, soft, out, W, st);
    } else if (kind == Trellis::Lanes16) {
        if constexpr (WIN == 256) hipLaunchKernelGGL(J.packed3 ? k_viterbi16_p3 : k_viterbi16, dim3(trellis_waves16(J)), dim3(64), 0, st, J.jobs, hdr, n1, stride, soft, out);
        else hipLaunchKernelGGL(k_viterbi16_11n, dim3(trellis_waves16(J)), dim3(64), 0, st, J.jobs, hdr, n1, stride, soft, out);
    } else {
        if constexpr (WIN == 256) hipLaunchKernelGGL(J.packed3 ? k_viterbi_p3 : k_viterbi, dim3(trellis_pair_groups(J)), dim3(256), 0, st, J.jobs, hdr, n1, stride, soft, out);
        else hipLaunchKernelGGL(k_viterbi11n, dim3(trellis_pair_groups(J)), dim3(256), 0, st, J.jobs, hdr, n1, stride, soft, out);
    }
}

// ---- code rate 5/6 (SORA_CR_56; k_vit56.hip).  A handle's job table may have a FOURTH list: hdr[3] jobs at jobs + 3 * stride.  The three kinds above keep reading
// hdr[0..2] and never see it; this enqueues k_viterbi56_11n over it -- one kernel, 64 lanes per pair: a handle's *_set_trellis does not apply to the fourth list.  n: the
// most jobs the list can hold in this call; soft_bytes: the extent of the soft buffer (no byte at or behind it is read).  A launch over an empty list costs its dispatch.
inline void trellis_launch56(const TrellisJobs& J, const uint8_t* soft, size_t soft_bytes, uint8_t* out, hipStream_t st)
{
    hipLaunchKernelGGL(k_viterbi56_11n, dim3((J.n + 7) / 8), dim3(256), 0, st, J.jobs, J.hdr, J.stride, soft, (uint32_t)soft_bytes, out);
}

}  // namespace sora
