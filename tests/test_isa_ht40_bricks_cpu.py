"""The stage kernels of the 40 MHz HT receiver (sora_amd/csrc/k_ht40_stages.hip) keep everything in registers and LDS: no scratch.  One kernel per stage (the demapper
one per modulation; the de-parser is the 802.11n stage's kernel), with the register and LDS figures as built.  Read from the code-object
metadata of libsora_hip.so, without a GPU."""
from test_isa_stream11b_cpu import kernel_metadata

# kernel -> (VGPRs, LDS bytes) as built
FIGURES = {
    "k_ht40s_data_symbolE": (18, 0), "k_ht40s_mimo_estE": (48, 0), "k_ht40s_mimo_compE": (48, 0), "k_ht40s_pilot_trackE": (34, 0),
    "k_ht40s_demapILi1E": (15, 5632), "k_ht40s_demapILi2E": (15, 5632), "k_ht40s_demapILi4E": (27, 5632), "k_ht40s_demapILi6E": (39, 5632),
    "k_ht40s_deintE": (51, 6480), "k_ht40s_downsampleE": (28, 0), "k_ht40s_noise_varE": (12, 0),
}


def test_one_kernel_per_stage_and_none_uses_scratch(tmp_path):
    md = {k: v for k, v in kernel_metadata(tmp_path, b"k_ht40s_").items() if "k_ht40s_" in k}
    assert len(md) == len(FIGURES), sorted(md)
    for want in FIGURES:
        assert sum(want in k for k in md) == 1, (want, sorted(md))
    for name, f in md.items():
        assert f["private_segment_fixed_size"] == 0 and f["vgpr_spill_count"] == 0, (name, f)


def test_register_and_lds_figures_as_built(tmp_path):
    md = kernel_metadata(tmp_path, b"k_ht40s_")
    got = {want: [(v["vgpr_count"], v["group_segment_fixed_size"]) for k, v in md.items() if want in k][0] for want in FIGURES}
    print(got)
    assert got == FIGURES
    # the de-interleave table and eight symbols' bytes: 648 x 2 + 8 x 648; the demap tables and eight symbols: 6 x 256 + 8 x 512
    assert FIGURES["k_ht40s_deintE"][1] == 648 * 2 + 8 * 648 and FIGURES["k_ht40s_demapILi6E"][1] == 6 * 256 + 8 * 512
