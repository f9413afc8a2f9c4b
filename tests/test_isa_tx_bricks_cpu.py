"""The transmit kernels keep their budgets now that their bricks are shared pieces (sora_amd/csrc/dev_tx.h): registers, scratch and LDS of every
one, read from the code-object metadata of libsora_hip.so, without a GPU.  The figures are those of the kernels before the pieces were shared
(DESIGN.md f2a): LDS is a layout and must be equal; registers and scratch must not grow (k_tx11a<false> and k_tx11n sit right at an occupancy step)."""
import re

from test_isa_stream11b_cpu import kernel_metadata

#          kernel                vgpr_count, private_segment_fixed_size, group_segment_fixed_size
BUDGET = {"k_tx11aILb0EE":      (64, 20, 17396),
          "k_tx11aILb1EE":      (98, 0, 17396),
          "k_tx_preamble":      (27, 0, 4608),
          "k_tx11n":            (76, 0, 22168),
          "k_tx_ht40_preamble": (33, 0, 2048),
          "k_tx_ht40":          (92, 0, 35632),
          "k_tx11b":            (49, 0, 25704)}


def test_transmit_kernels_keep_their_register_scratch_and_lds_budgets(tmp_path):
    md = kernel_metadata(tmp_path, b"k_tx")
    names = {re.sub(r"^_ZN4sora\d+(k_tx11aILb[01]EE|k_tx\w*?)E.*$", r"\1", k): v for k, v in md.items()}
    for k, (vgpr, scratch, lds) in BUDGET.items():
        assert k in names, "kernel %s missing from libsora_hip.so (found %s)" % (k, sorted(names))
        assert names[k]["group_segment_fixed_size"] == lds, (k, names[k])
        assert names[k]["vgpr_count"] <= vgpr, (k, names[k])
        assert names[k]["private_segment_fixed_size"] <= scratch, (k, names[k])
