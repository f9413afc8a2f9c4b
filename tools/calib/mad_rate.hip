// mad_rate.hip -- the issue rate of the integer multiply-adds an index computation can compile to on gfx950: v_mad_u32_u24 (what __umul24 + add gives)
// against v_mad_u64_u32 (what a plain 32-bit a * b + c gives: the chip has no v_mad_u32) and v_lshl_add_u64 (a 64-bit base + index << k), with
// v_add_u32 as the full-rate yardstick.  Same method as valu_peak.hip: a long unrolled run of ONE instruction kind on independent registers, grid = all CUs x W
// waves per SIMD, rate = instructions x waves / wall time (HIP events).
//   hipcc --offload-arch=gfx950 -O3 -o mad_rate mad_rate.hip && ./mad_rate
#include <hip/hip_runtime.h>
#include <cstdio>

#define REP8(x) x x x x x x x x
#define REP64(x) REP8(REP8(x))

template <int KIND> __global__ void __launch_bounds__(256) k_probe(unsigned* out, int iters)
{
    unsigned a = threadIdx.x, b = a * 3 + 1, c = a ^ 0x55, d = a + 7, g = 0x00030003u, h = a * 7 + 1;
    unsigned long long w = a, x = b, y = c, z = d, base = h;
    for (int i = 0; i < iters; i++) {
        if (KIND == 0)          // v_add_u32
            asm volatile(REP64("v_add_u32 %0, %4, %0\n\tv_add_u32 %1, %4, %1\n\tv_add_u32 %2, %4, %2\n\tv_add_u32 %3, %4, %3\n\t") : "+v"(a), "+v"(b), "+v"(c), "+v"(d) : "v"(g));
        else if (KIND == 1)     // v_mad_u32_u24
            asm volatile(REP64("v_mad_u32_u24 %0, %4, %5, %0\n\tv_mad_u32_u24 %1, %4, %5, %1\n\tv_mad_u32_u24 %2, %4, %5, %2\n\tv_mad_u32_u24 %3, %4, %5, %3\n\t")
                         : "+v"(a), "+v"(b), "+v"(c), "+v"(d) : "v"(g), "v"(h));
        else if (KIND == 2)     // v_mad_u64_u32 (the carry-out goes to vcc)
            asm volatile(REP64("v_mad_u64_u32 %0, vcc, %4, %5, %0\n\tv_mad_u64_u32 %1, vcc, %4, %5, %1\n\tv_mad_u64_u32 %2, vcc, %4, %5, %2\n\tv_mad_u64_u32 %3, vcc, %4, %5, %3\n\t")
                         : "+v"(w), "+v"(x), "+v"(y), "+v"(z) : "v"(g), "v"(h) : "vcc");
        else if (KIND == 3)     // v_lshl_add_u64
            asm volatile(REP64("v_lshl_add_u64 %0, %0, 2, %4\n\tv_lshl_add_u64 %1, %1, 2, %4\n\tv_lshl_add_u64 %2, %2, 2, %4\n\tv_lshl_add_u64 %3, %3, 2, %4\n\t")
                         : "+v"(w), "+v"(x), "+v"(y), "+v"(z) : "v"(base));
        else                    // v_mul_lo_u32
            asm volatile(REP64("v_mul_lo_u32 %0, %4, %0\n\tv_mul_lo_u32 %1, %4, %1\n\tv_mul_lo_u32 %2, %4, %2\n\tv_mul_lo_u32 %3, %4, %3\n\t") : "+v"(a), "+v"(b), "+v"(c), "+v"(d) : "v"(h));
    }
    if (a + b + c + d + (unsigned)(w + x + y + z) == 0x12345u) out[0] = a;
}

struct Probe { const char* name; void (*k)(unsigned*, int); };

int main()
{
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, 0) != hipSuccess) { printf("no device\n"); return 1; }
    const int cus = prop.multiProcessorCount;
    unsigned* d;
    if (hipMalloc(&d, 4096) != hipSuccess) return 1;
    const Probe probes[] = { { "v_add_u32", k_probe<0> }, { "v_mad_u32_u24", k_probe<1> }, { "v_mad_u64_u32", k_probe<2> }, { "v_lshl_add_u64", k_probe<3> }, { "v_mul_lo_u32", k_probe<4> } };
    printf("# %s, %d CUs; G wave-instructions/s = instructions x waves / wall time (HIP events), ~25 ms per measurement after a warm-up of the same kernel\n", prop.name, cus);
    printf("%-20s %12s %12s %12s %12s\n", "kind", "1 w/SIMD", "2 w/SIMD", "4 w/SIMD", "8 w/SIMD");
    hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
    for (const Probe& p : probes) {
        printf("%-20s", p.name);
        for (int wps : { 1, 2, 4, 8 }) {
            const int blocks = cus * wps;                                         // 256-thread blocks: one wave per SIMD each
            int iters = 500;
            float ms = 0;
            for (int pass = 0; pass < 3; pass++) {                                // calibrate to ~25 ms, then warm, then measure
                hipEventRecord(e0, 0);
                hipLaunchKernelGGL(p.k, dim3(blocks), dim3(256), 0, 0, d, iters);
                hipEventRecord(e1, 0);
                if (hipDeviceSynchronize() != hipSuccess) { printf("\nkernel failed\n"); return 1; }
                hipEventElapsedTime(&ms, e0, e1);
                if (pass == 0) iters = (int)(iters * 25.0f / (ms > 0.01f ? ms : 0.01f)) + 1;
            }
            const double insts = (double)iters * 256.0 * (double)blocks * 4.0;
            printf(" %12.1f", insts / (ms * 1e-3) / 1e9);
        }
        printf("\n");
    }
    return 0;
}
