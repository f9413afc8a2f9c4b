// host_stage.h -- what every stand-alone stage entry point (sora_hip_<brick>(..., size_t count, void* stream), include/sora_hip.h) does in front of and behind its
// launch, each thing once.  An entry point reads top to bottom: STAGE_ENTRY, its own argument checks, its grid, its launch, launch_result.  Host code only.
#pragma once
#include "host_calls.h"
#include "kernels.h"

// The checks every stage shares, in the one order the header states: a null pointer is refused by name; a count of 0 is nothing to launch (true with or without a
// device); no device; a count the kernels' 32-bit indices cannot hold.  Returns from its caller.  who: the entry point's name, a string literal.
#define STAGE_ENTRY(who, nullcond, count) \
    if (nullcond) return sora_internal_fail(SORA_ERR_INVALID_PARAM, who ": null pointer", 0); \
    if ((count) == 0) return SORA_OK; \
    if (sora_hip_device_count() <= 0) return sora_internal_fail(SORA_ERR_NO_DEVICE, "no HIP device: this library has no CPU path", 0); \
    if ((count) >= (1ull << 31)) return sora_internal_fail(SORA_ERR_CAPACITY, who ": too many for one call", 0);
#define STAGE_NBPSC(who, nb) \
    if (!((nb) == 1 || (nb) == 2 || (nb) == 4 || (nb) == 6)) return sora_internal_fail(SORA_ERR_INVALID_PARAM, who ": n_bpsc must be 1, 2, 4 or 6", 0);
#define STAGE_STREAM01(who, iss) \
    if ((iss) < 0 || (iss) > 1) return sora_internal_fail(SORA_ERR_INVALID_PARAM, who ": spatial_stream must be 0 or 1", 0);
// the buffers a stage moves 16 bytes per lane
#define STAGE_ALIGNED16(who, ...) \
    if (!aligned16(__VA_ARGS__)) return sora_internal_fail(SORA_ERR_INVALID_PARAM, who ": buffers must be 16-byte aligned", 0);
// a kernel template's 1 / 2 / 4 / 6 instances, workgroups of 256 (nb has passed STAGE_NBPSC)
#define STAGE_BY_NBPSC(nb, kernel, grid, st, ...) \
    switch (nb) { \
    case 1: hipLaunchKernelGGL(kernel<1>, grid, dim3(256), 0, st, __VA_ARGS__); break; \
    case 2: hipLaunchKernelGGL(kernel<2>, grid, dim3(256), 0, st, __VA_ARGS__); break; \
    case 4: hipLaunchKernelGGL(kernel<4>, grid, dim3(256), 0, st, __VA_ARGS__); break; \
    default: hipLaunchKernelGGL(kernel<6>, grid, dim3(256), 0, st, __VA_ARGS__); break; \
    }

namespace sora {

// behind the launch(es) of `kernel`: SORA_OK, or the launch error under the kernel's name
inline int launch_result(const char* kernel)
{
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? SORA_OK : sora_internal_fail(SORA_ERR_HARDWARE_FAILED, kernel, (int)e);
}

template <class... P> inline bool aligned16(P... p) { return ((... | (uintptr_t)p) & 15) == 0; }
template <class... P> inline bool aligned4(P... p) { return ((... | (uintptr_t)p) & 3) == 0; }

// packed COMPLEX16 samples and the stages' records as the 32-bit words the kernels take
inline const uint32_t* u32(const void* p) { return static_cast<const uint32_t*>(p); }
inline uint32_t* u32(void* p) { return static_cast<uint32_t*>(p); }

// workgroups of 256 positions per frame, frames x chunks in one grid dimension; false: no position, or too many workgroups for one launch
inline bool stage_grid(size_t nframes, size_t max_items, uint32_t* chunks, unsigned* grid)
{
    const size_t c = (max_items + 255) / 256, g = nframes * c;
    if (c == 0 || g >= (1ull << 31)) return false;
    *chunks = (uint32_t)c; *grid = (unsigned)g;
    return true;
}

// workgroups of `per` items each for `count` of them (count has passed STAGE_ENTRY)
inline unsigned stage_tiles(size_t count, size_t per) { return (unsigned)((count + per - 1) / per); }
// gridDim.y of the stages whose workgroup (f, y) strides over the passes of frame f: the frames' lengths are device memory, so a batch of few frames gets several
// workgroups per frame
inline unsigned stage_frame_grid(size_t nframes) { return nframes >= 2048 ? 1u : (unsigned)std::min<size_t>(64, 2048 / nframes); }

// the current device's look-up tables (uploaded on first use)
inline int stage_tables(Tables* T)
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || sora_internal_tables(dev, T) != SORA_OK) return sora_internal_fail(SORA_ERR_HARDWARE_FAILED, "table upload failed", 0);
    return SORA_OK;
}

}  // namespace sora
