// dev_ht40.h -- what the 40 MHz HT receiver (k_ht40.hip) and transmitter (k_tx_ht40.hip) both state about the format, from IEEE 802.11n-2009
// clause 20: the HT-LTF sequence, the data carriers and the HT interleaver for 40 MHz.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sora {

static __constant__ int8_t kHtLtf40[117] = {    // carriers -58..58 (IEEE 802.11n-2009 eq. 20-24)
    1, 1, -1, -1, 1, 1, -1, 1, -1, 1, 1, 1, 1, 1, 1, -1, -1, 1, 1, -1, 1, -1, 1, 1, 1, 1, 1, 1, -1, -1, 1, 1, -1, 1, -1, 1, -1, -1, -1, -1, -1, 1, 1, -1, -1, 1, -1, 1, -1, 1, 1, 1, 1,
    -1, -1, -1, 1, 0, 0, 0, -1, 1, 1, -1,
    1, 1, -1, -1, 1, 1, -1, 1, -1, 1, 1, 1, 1, 1, 1, -1, -1, 1, 1, -1, 1, -1, 1, 1, 1, 1, 1, 1, -1, -1, 1, 1, -1, 1, -1, 1, -1, -1, -1, -1, -1, 1, 1, -1, -1, 1, -1, 1, -1, 1, 1, 1, 1 };
__device__ __forceinline__ int data_bin40(int c)          // data carrier c (0..107) -> FFT bin: -58..-2 then 2..58 without +-11, +-25, +-53
{
    int k;
    if (c < 54) { k = -58 + c; if (k >= -53) k++; if (k >= -25) k++; if (k >= -11) k++; }
    else { k = 2 + (c - 54); if (k >= 11) k++; if (k >= 25) k++; if (k >= 53) k++; }
    return k & 127;
}
__device__ __forceinline__ int deint40_index(int nb, int iss, int k)     // HT interleaver for 40 MHz: where coded bit k of stream iss sits in the symbol
{
    const int s = nb / 2 > 1 ? nb / 2 : 1, nrow = 6 * nb, np = 108 * nb;
    const int i = nrow * (k % 18) + k / 18;
    int j = s * (i / s) + (i + np - (18 * i) / np) % s;
    if (iss > 0) j = ((j - ((iss * 2) % 3 + 3 * (iss / 3)) * 29 * nb) % np + np) % np;
    return j;
}

}  // namespace sora
