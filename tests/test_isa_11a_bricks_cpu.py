"""The stage kernels of the 802.11a receive graph's front end (sora_amd/csrc/k_11a.hip) keep everything in registers: no scratch.  One kernel per stage, and the
carrier-sense kernels' register counts as built.  Read from the code-object metadata of libsora_hip.so, without a GPU."""
from test_isa_stream11b_cpu import kernel_metadata

STAGES = ("dc_remove", "dc_estimate", "cca", "carrier_sense", "data_symbol", "viterbi_sig", "plcp_parse")
CARRIER_SENSE_VGPRS = 83
CCA_VGPRS = 114


def test_one_kernel_per_stage_and_none_uses_scratch(tmp_path):
    md = {k: v for k, v in kernel_metadata(tmp_path, b"k_11a_").items() if "k_11a_" in k}
    assert len(md) == len(STAGES), sorted(md)
    for want in STAGES:
        assert sum(("k_11a_" + want + "E") in k for k in md) == 1, (want, sorted(md))      # (E: the end of the mangled name)
    for name, f in md.items():
        assert f["private_segment_fixed_size"] == 0 and f["vgpr_spill_count"] == 0, (name, f)


def test_the_carrier_sense_kernels_register_count(tmp_path):
    md = kernel_metadata(tmp_path, b"k_11a_")
    cs = [v for k, v in md.items() if "k_11a_carrier_senseE" in k][0]; cca = [v for k, v in md.items() if "k_11a_ccaE" in k][0]
    print("k_11a_carrier_sense:", cs, " k_11a_cca:", cca)
    assert cs["vgpr_count"] == CARRIER_SENSE_VGPRS and cca["vgpr_count"] == CCA_VGPRS
    assert cs["group_segment_fixed_size"] == 0 and cca["group_segment_fixed_size"] == 0       # the tile lives in registers: v_readlane hands the walk its burst
