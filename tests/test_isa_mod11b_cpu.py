"""The stage kernels of the 802.11b modulation graph (sora_amd/csrc/k_mod11b.hip) keep everything in registers: no scratch.  One kernel per stage.  Read from the
code-object metadata of libsora_hip.so, without a GPU."""
from test_isa_stream11b_cpu import kernel_metadata

STAGES = ("ppdu", "sc741", "dbpsk", "dqpsk", "cck5", "cck11", "shape")


def test_one_kernel_per_stage_and_none_uses_scratch(tmp_path):
    md = {k: v for k, v in kernel_metadata(tmp_path, b"k_mod11b").items() if "k_mod11b_" in k}
    assert len(md) == len(STAGES), sorted(md)
    for want in STAGES:
        assert sum(("k_mod11b_" + want + "E") in k for k in md) == 1, (want, sorted(md))      # (E: the end of the mangled name -- cck5 is not cck5..)
    for name, f in md.items():
        assert f["private_segment_fixed_size"] == 0, (name, f)
