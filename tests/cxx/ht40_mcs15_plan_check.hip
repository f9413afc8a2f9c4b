// ht40_mcs15_plan_check.hip -- a stand-alone program over the host-side planning code of MCS 15 on the 40 MHz HT pair: tx_ht40_plan_mcs
// (sora_amd/csrc/kernels.h) in both codings, and ht40_ndbps / code_rate_ht40 (dev_11n.h).  It walks every MCS 0..31, every length 0..4100 and the gates 13..16 and holds
// the gated plan to a closed form written out here once more, to the existing plans where the gate is 14, and to the bounds the transmitter's LDS plan and the receive
// handle's buffers rest on.  Meant to be built with the host sanitizers and run on its own -- no device is touched:
//   hipcc --offload-arch=gfx950 -std=c++17 -Xarch_host -fsanitize=address,undefined -Isora_amd/csrc tests/cxx/ht40_mcs15_plan_check.hip -o ht40_mcs15_plan_check
#include <stdio.h>
#include <stdint.h>
#include "kernels.h"
#include "dev_11n.h"

using namespace sora;

int main()
{
    static const int nbs[8] = { 1, 2, 2, 4, 4, 6, 6, 6 }, crs[8] = { 0, 0, 2, 0, 2, 1, 2, 3 };
    static const uint32_t num[4] = { 1, 2, 3, 5 }, den[4] = { 2, 3, 4, 6 };
    unsigned long checked = 0;
    uint32_t max_bits[2] = { 0, 0 };
    for (int joint = 0; joint < 2; joint++)
        for (uint32_t gate = 13; gate <= 16; gate++)
            for (uint32_t mcs = 0; mcs < 32; mcs++)
                for (uint32_t len = 0; len <= 4100; len++) {
                    TxHt40Plan P{}, Q{};
                    const bool ok = tx_ht40_plan_mcs(len, mcs, gate, joint != 0, P);
                    const bool want = (gate == 14 || gate == 15) && mcs >= 8 && mcs <= gate && len >= 1 && len <= 3996;
                    if (ok != want) { printf("acceptance: joint %d gate %u mcs %u len %u -> %d\n", joint, gate, mcs, len, (int)ok); return 1; }
                    const bool old = joint ? tx_ht40_plan_joint(len, mcs, Q) : tx_ht40_plan(len, mcs, Q);
                    if (old != (mcs >= 8 && mcs <= 14 && len >= 1 && len <= 3996)) { printf("the ungated plan accepts MCS 15: mcs %u len %u\n", mcs, len); return 1; }
                    if (gate == 14 && (ok != old || (ok && (P.nb != Q.nb || P.cr != Q.cr || P.ndbps != Q.ndbps || P.nsym != Q.nsym)))) {
                        printf("gate 14 is not the existing plan: joint %d mcs %u len %u\n", joint, mcs, len); return 1; }
                    if (!ok) continue;
                    const int nb = nbs[mcs - 8], cr = crs[mcs - 8];
                    const uint32_t nd = (108u * (uint32_t)nb * num[cr] / den[cr]) << joint;
                    const uint32_t bits = 16u + 8u * (len + 4u) + 6u, nsym = (bits + nd - 1u) / nd;
                    if (P.nb != nb || P.cr != cr || (uint32_t)P.ndbps != nd || P.nsym != nsym || nd != (ht40_ndbps((uint32_t)nb, (uint32_t)cr) << joint) ||
                        code_rate_ht40(mcs) != (uint32_t)cr || nbpsc11n(mcs) != (uint32_t)nb) {
                        printf("plan: joint %d mcs %u len %u -> nb %d cr %d ndbps %d nsym %u\n", joint, mcs, len, P.nb, P.cr, P.ndbps, P.nsym); return 1; }
                    if (!(nsym * nd >= bits && (nsym - 1u) * nd < bits)) { printf("symbols: mcs %u len %u\n", mcs, len); return 1; }
                    // a symbol is a whole number of puncture periods on both sides of the encoder
                    if (mcs == 15 && ((108u * 6u << joint) % 6u != 0 || nd % 5u != 0 || nd / 5u * 6u != (648u << joint))) { printf("puncture periods\n"); return 1; }
                    if (mcs == 15 && nsym * nd > max_bits[joint]) max_bits[joint] = nsym * nd;
                    checked++;
                }
    // MCS 15's largest field: 32400 bits in both codings (60 symbols of 540, 30 of 1080) -- inside the 32561 / 33101 the transmitter's LDS plan asserts, and
    // inside kGen x 32 = 33280 generator bits; the receive handle's largest rate-5/6 job: 60 x 648 = 38880 soft bytes per stream, 77760 joint
    if (max_bits[0] != 32400u || max_bits[1] != 32400u || max_bits[0] > 32561u || max_bits[1] > 33101u) { printf("bounds: %u / %u bits\n", max_bits[0], max_bits[1]); return 1; }
    printf("ht40_mcs15_plan_check: %lu plans, largest MCS 15 field %u bits per stream, %u joint: OK\n", checked, max_bits[0], max_bits[1]);
    return 0;
}
