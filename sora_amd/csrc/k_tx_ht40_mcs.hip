// k_tx_ht40_mcs.hip -- the 40 MHz HT 2x2 transmitter with the gate at 15 (sora_hip_tx_ht40_mcs, sora_hip_tx_ht40_joint_mcs): the guard-aware
// body of dev_tx_ht40.h with M15 = true -- the gated plan (MCS 15: 64-QAM, N_DBPS 540 per stream / 1080 joint) and the puncture map that knows rate 5/6
// (tx_punct_offset56).  A file of its own: k_tx_ht40.hip's kernels are compiled among the functions they always were.
#include "dev_tx_ht40.h"

namespace sora {

__global__ void __launch_bounds__(256) k_tx_ht40_mcs(TxHt40Args A) { tx_ht40_body<false, true, true>(A); }
__global__ void __launch_bounds__(256) k_tx_ht40_joint_mcs(TxHt40Args A) { tx_ht40_body<true, true, true>(A); }


}  // namespace sora
