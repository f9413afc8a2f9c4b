// ht40_joint_plan_check.hip -- a stand-alone program over the host-side planning code of the 40 MHz HT pair's joint coding: tx_ht40_plan_joint
// and ht40_symbols_joint (sora_amd/csrc/kernels.h; sora_ht40_symbols_joint is the latter over 2 x ht40_ndbps).  It walks every MCS 0..31 and every length 0..4100 and
// holds the plan to the format's own statement, written out here once more, and to the bounds the kernels' LDS and output plans rest on.  Meant to be built with the
// host sanitizers and run on its own -- no device is touched:
//   hipcc --offload-arch=gfx950 -std=c++17 -Xarch_host -fsanitize=address,undefined -Isora_amd/csrc tests/cxx/ht40_joint_plan_check.hip -o ht40_joint_plan_check
#include <stdio.h>
#include <stdint.h>
#include "kernels.h"
#include "dev_11n.h"

using namespace sora;

int main()
{
    static const int nbs[7] = { 1, 2, 2, 4, 4, 6, 6 }, crs[7] = { 0, 0, 2, 0, 2, 1, 2 };
    static const uint32_t num[3] = { 1, 2, 3 }, den[3] = { 2, 3, 4 };
    unsigned long checked = 0;
    uint32_t max_bits = 0, max_soft = 0;
    for (uint32_t mcs = 0; mcs < 32; mcs++)
        for (uint32_t len = 0; len <= 4100; len++) {
            TxHt40Plan P{}, Q{};
            const bool ok = tx_ht40_plan_joint(len, mcs, P);
            const bool want = mcs >= 8 && mcs <= 14 && len >= 1 && len <= 3996;
            if (ok != want) { printf("acceptance: mcs %u len %u -> %d\n", mcs, len, (int)ok); return 1; }
            if (ok != tx_ht40_plan(len, mcs, Q)) { printf("the two codings accept different frames: mcs %u len %u\n", mcs, len); return 1; }
            if (!ok) continue;
            const int nb = nbs[mcs - 8], cr = crs[mcs - 8];
            const uint32_t nd = 2u * 108u * (uint32_t)nb * num[cr] / den[cr];
            const uint32_t bits = 16u + 8u * (len + 4u) + 6u, nsym = (bits + nd - 1u) / nd;
            if (P.nb != nb || P.cr != cr || (uint32_t)P.ndbps != nd || P.nsym != nsym || nd != 2u * (uint32_t)Q.ndbps || nd != 2u * ht40_ndbps((uint32_t)nb, (uint32_t)cr)) {
                printf("plan: mcs %u len %u -> nb %d cr %d ndbps %d nsym %u\n", mcs, len, P.nb, P.cr, P.ndbps, P.nsym); return 1; }
            if (ht40_symbols_joint(len + 4u, nd) != nsym || !(nsym * nd >= bits && (nsym - 1u) * nd < bits)) { printf("symbols: mcs %u len %u\n", mcs, len); return 1; }
            if (2u * nsym < Q.nsym || 2u * nsym > Q.nsym + 1u) { printf("joint N_SYM is not half the per-stream one, rounded up: mcs %u len %u\n", mcs, len); return 1; }
            if (nsym * nd > max_bits) max_bits = nsym * nd;
            if (nsym * 216u * (uint32_t)nb > max_soft) max_soft = nsym * 216u * (uint32_t)nb;
            checked++;
        }
    // the bounds k_tx_ht40_joint's LDS plan and the receive handle's buffers assert: 32832 field bits (1026 generator words, 4108 field bytes: MCS 13), 64800 soft bytes
    // in one decoder job (MCS 11; MCS 8 has 64152)
    if (max_bits != 32832u || (max_bits + 31u) / 32u != 1026u || max_soft != 64800u) { printf("bounds: %u bits, %u soft bytes\n", max_bits, max_soft); return 1; }
    printf("ht40_joint_plan_check: %lu plans, largest field %u bits, largest job %u soft bytes: OK\n", checked, max_bits, max_soft);
    return 0;
}
