"""The kernels MCS 15 adds ship as kernels of their own and fit the budget of the kernels they are modelled on: read from the code-object
metadata of libsora_hip.so, without a GPU.  k_viterbi56_11n (a job table's fourth list) and k_viterbi56_11n_stage (the stage entry point's arrays) exist, have no scratch
and no spills, k_viterbi11n's LDS plus their 16-byte aligned operand table's padding (four workgroups per CU either way), and a VGPR count that allows as many waves
per SIMD; k_tx_ht40_mcs / k_tx_ht40_joint_mcs fit k_tx_ht40_gi / k_tx_ht40_joint_gi the same way (the rule of tests/test_isa_ht40_gi_cpu.py)."""
import re

from test_isa_stream11b_cpu import kernel_metadata

waves = lambda v: 512 // ((v + 7) // 8 * 8)                              # waves per SIMD the VGPR budget allows (gfx950: 512 per lane)


def _kernels(tmp_path, *holds):
    md = {}
    for h in holds:
        md.update(kernel_metadata(tmp_path, h))
    return {re.sub(r"^_ZN4sora\d+(k_[a-z0-9_]+?)E.*$", r"\1", k): v for k, v in md.items()}


def test_rate_56_trellis_kernels_exist_and_fit_the_pair_kernels_budget(tmp_path):
    names = _kernels(tmp_path, b"k_viterbi")
    p = names["k_viterbi11n"]
    for new in ("k_viterbi56_11n", "k_viterbi56_11n_stage"):
        assert new in names, sorted(names)
        n = names[new]
        assert n["private_segment_fixed_size"] == 0 and n.get("vgpr_spill_count", 0) == 0, (new, n)
        assert n["vgpr_count"] <= 128 and waves(n["vgpr_count"]) >= waves(p["vgpr_count"]), (new, n, p)
        # the ring of RingGeom<192, 36> for four waves and their operand tables; 160 KB per CU hold four such workgroups, as they hold four of k_viterbi11n's
        assert n["group_segment_fixed_size"] == 4 * (2 * 33 * 64 * 2 + 64 * 2), (new, n)
        assert n["group_segment_fixed_size"] <= p["group_segment_fixed_size"] + 64 and 4 * n["group_segment_fixed_size"] <= 160 * 1024, (new, n, p)


def test_gated_transmitter_kernels_exist_and_fit_their_parents_budget(tmp_path):
    names = _kernels(tmp_path, b"k_tx_ht40")
    for new, parent in (("k_tx_ht40_mcs", "k_tx_ht40_gi"), ("k_tx_ht40_joint_mcs", "k_tx_ht40_joint_gi")):
        assert new in names and parent in names, sorted(names)
        n, p = names[new], names[parent]
        assert n["private_segment_fixed_size"] == 0 and n.get("vgpr_spill_count", 0) == 0, (new, n)
        assert n["group_segment_fixed_size"] <= p["group_segment_fixed_size"], (new, n, p)
        assert waves(n["vgpr_count"]) >= waves(p["vgpr_count"]), (new, n, p)
