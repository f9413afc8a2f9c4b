"""The stage kernels of the 802.11a modulation graph (sora_amd/csrc/k_mod.hip) keep everything in registers: no scratch, no spills.  Read from the
code-object metadata of libsora_hip.so, without a GPU."""
from test_isa_stream11b_cpu import kernel_metadata


def test_no_mod11a_kernel_uses_scratch_or_spills(tmp_path):
    md = {k: v for k, v in kernel_metadata(tmp_path, b"k_mod_").items() if "k_mod_" in k and "k_mod_ht40" not in k}
    assert len(md) >= 9, sorted(md)
    for want in ("scramble", "encode", "interleave", "map", "add_pilot", "ifftx", "upsample", "pack16to8", "preamble"):
        assert any("k_mod_" + want in k for k in md), (want, sorted(md))
    for nb in (1, 2, 4, 6):                                                      # the instances of the bodies shared with the 802.11n and 40 MHz HT graphs
        assert any("k_mod_interleaveILi%dE" % nb in k for k in md) and any("k_mod_mapILi%dE" % nb in k for k in md), (nb, sorted(md))
    for name, f in md.items():
        assert f["private_segment_fixed_size"] == 0, (name, f)
        assert f.get("vgpr_spill_count", 0) == 0 and f.get("sgpr_spill_count", 0) == 0, (name, f)
