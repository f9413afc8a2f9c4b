// dev_pilot11a.h -- the 802.11a pilot polarity sequence, stated once for the receive chain (dev_sym11a.h) and the transmitters (dev_tx.h, k_tx.hip, k_tx11n.hip).
#pragma once
#include <stdint.h>

namespace sora {

// pilot polarity (pilot.hpp:10-28, period 127): 1 <=> polarity -1 of symbol count i (127 -> 0 after the SIGNAL symbol)
struct PilotPolarity { uint8_t neg[128]; };
constexpr PilotPolarity kPilotPolarity = { {
    0,0,0,1,1,1,0,1, 1,1,1,0,0,1,0,1, 1,0,0,1,0,0,1,0, 0,0,0,0,0,1,0,0,
    0,1,0,0,1,1,0,0, 0,1,0,1,1,1,0,1, 0,1,1,0,1,1,0,0, 0,0,0,1,1,0,0,1,
    1,0,1,0,1,0,0,1, 1,1,0,0,1,1,1,1, 0,1,1,0,1,0,0,0, 0,1,0,1,0,1,0,1,
    1,1,1,1,0,1,0,0, 1,0,1,0,0,0,1,1, 0,1,1,1,0,0,0,1, 1,1,1,1,1,1,0,0 } };
// the same as a bit string: bit n of word n >> 5
constexpr uint32_t pilot_word(int w) { uint32_t v = 0; for (int j = 0; j < 32; j++) v |= (uint32_t)kPilotPolarity.neg[32 * w + j] << j; return v; }
constexpr uint32_t kPilotW0 = pilot_word(0), kPilotW1 = pilot_word(1), kPilotW2 = pilot_word(2), kPilotW3 = pilot_word(3);
static_assert(kPilotW0 == 0x2049a7b8u && kPilotW3 == 0x3f8ec52fu, "pilot polarity words");
// one bit of the sequence's four words: 1 <=> polarity -1 at symbol count `count` (0..127)
__device__ __forceinline__ unsigned pilot_sgn(unsigned count)
{
    const unsigned w = count < 32 ? kPilotW0 : count < 64 ? kPilotW1 : count < 96 ? kPilotW2 : kPilotW3;
    return (w >> (count & 31u)) & 1u;
}
// pilot k = 0..3 sits at carrier -21, -7, 7, 21; the 802.11a pilots are (1, 1, 1, -1) x polarity (pilot.hpp:76-118)
__device__ __forceinline__ int pilot_carrier(int k) { return k == 0 ? -21 : k == 1 ? -7 : k == 2 ? 7 : 21; }

}  // namespace sora
