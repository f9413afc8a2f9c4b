// dev_tx.h -- pieces shared by the transmitters (k_tx.hip: 802.11a, k_tx11n.hip: 802.11n 2x2).
#pragma once
#include <stdint.h>

namespace sora {

constexpr uint8_t kPilotSgnTx[128] = {         // pilot.hpp:10-28: 1 <=> polarity -1
    0,0,0,1,1,1,0,1, 1,1,1,0,0,1,0,1, 1,0,0,1,0,0,1,0, 0,0,0,0,0,1,0,0,
    0,1,0,0,1,1,0,0, 0,1,0,1,1,1,0,1, 0,1,1,0,1,1,0,0, 0,0,0,1,1,0,0,1,
    1,0,1,0,1,0,0,1, 1,1,0,0,1,1,1,1, 0,1,1,0,1,0,0,0, 0,1,0,1,0,1,0,1,
    1,1,1,1,0,1,0,0, 1,0,1,0,0,0,1,1, 0,1,1,1,0,0,0,1, 1,1,1,1,1,1,0,0 };

constexpr uint32_t pilot_word(int w) { uint32_t v = 0; for (int j = 0; j < 32; j++) v |= (uint32_t)kPilotSgnTx[32 * w + j] << j; return v; }   // bit n of word n >> 5 = kPilotSgnTx[n]
constexpr uint32_t kPilotW0 = pilot_word(0), kPilotW1 = pilot_word(1), kPilotW2 = pilot_word(2), kPilotW3 = pilot_word(3);
static_assert(kPilotW0 == 0x2049a7b8u && kPilotW3 == 0x3f8ec52fu, "pilot polarity words");

}  // namespace sora
