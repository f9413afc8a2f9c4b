"""The stage kernels of the 40 MHz HT modulation graph (sora_amd/csrc/k_mod_ht40.hip) keep everything in registers: no scratch, no spills.  Read from the
code-object metadata of libsora_hip.so, without a GPU."""
from test_isa_stream11b_cpu import kernel_metadata


def test_no_mod_ht40_kernel_uses_scratch_or_spills(tmp_path):
    md = {k: v for k, v in kernel_metadata(tmp_path, b"k_mod_ht40").items() if "k_mod_ht40_" in k}
    assert len(md) >= 9, sorted(md)
    for want in ("parse", "interleave", "interleave_stream", "map", "sig_map", "add_pilot", "ifft", "add_gi", "preamble"):
        assert any("k_mod_ht40_" + want in k for k in md), (want, sorted(md))
    assert any("k_mod_ht40_interleave" in k and "stream" not in k for k in md), sorted(md)
    assert any("k_mod_ht40_map" in k for k in md) and any("k_mod_ht40_sig_map" in k for k in md), sorted(md)
    for name, f in md.items():
        assert f["private_segment_fixed_size"] == 0, (name, f)
        assert f.get("vgpr_spill_count", 0) == 0 and f.get("sgpr_spill_count", 0) == 0, (name, f)
