"""The stage kernels of the 802.11n modulation graphs (sora_amd/csrc/k_mod11n.hip) keep everything in registers: no scratch, no spills.  Read from the
code-object metadata of libsora_hip.so, without a GPU."""
from test_isa_stream11b_cpu import kernel_metadata


def test_no_mod11n_kernel_uses_scratch_or_spills(tmp_path):
    md = {k: v for k, v in kernel_metadata(tmp_path, b"k_mod11n").items() if "k_mod11n_" in k}
    assert len(md) >= 9, sorted(md)
    for want in ("parse", "interleave", "map", "sig_map", "add_pilot", "ifft", "csd", "add_gi", "preamble"):
        assert any("k_mod11n_" + want in k for k in md), (want, sorted(md))
    for name, f in md.items():
        assert f["private_segment_fixed_size"] == 0, (name, f)
        assert f.get("vgpr_spill_count", 0) == 0, (name, f)
