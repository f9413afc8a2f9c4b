"""The guard-aware instantiations ship as kernels of their own and fit the budget of the kernels they are made from: read from the code-object
metadata of libsora_hip.so, without a GPU.  Each exists, has no scratch and no spills, no more LDS than its parent, and a VGPR count that allows at least as many waves
per SIMD (the rule of tests/test_stream11n_cpu.py)."""
import re

from test_isa_stream11b_cpu import kernel_metadata

PAIRS = [("k_tx_ht40_gi", "k_tx_ht40"), ("k_tx_ht40_joint_gi", "k_tx_ht40_joint"),
         ("k_ht40_frame_gi", "k_ht40_frame"), ("k_ht40_frame_joint_gi", "k_ht40_frame_joint"),
         ("k_scan_ht40_gi", "k_scan_ht40"), ("k_scan_ht40_stream_gi", "k_scan_ht40_stream")]


def _kernels(tmp_path):
    md = {}
    for holds in (b"k_tx_ht40", b"k_ht40_frame", b"k_scan_ht40"):
        md.update(kernel_metadata(tmp_path, holds))
    return {re.sub(r"^_ZN4sora\d+(k_[a-z0-9_]+?)E.*$", r"\1", k): v for k, v in md.items()}


def test_guard_aware_kernels_exist_and_fit_their_parents_budget(tmp_path):
    names = _kernels(tmp_path)
    waves = lambda v: 512 // ((v + 7) // 8 * 8)                          # waves per SIMD the VGPR budget allows (gfx950: 512 per lane)
    for new, parent in PAIRS:
        assert new in names and parent in names, "kernel %s / %s missing from libsora_hip.so (found %s)" % (new, parent, sorted(names))
        n, p = names[new], names[parent]
        assert n["private_segment_fixed_size"] == 0 and n.get("vgpr_spill_count", 0) == 0, (new, n)
        assert n["group_segment_fixed_size"] <= p["group_segment_fixed_size"], (new, n, p)
        assert waves(n["vgpr_count"]) >= waves(p["vgpr_count"]), (new, n, p)
