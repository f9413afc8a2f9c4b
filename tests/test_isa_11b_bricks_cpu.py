"""Both forms of the 802.11b receive graph keep their budgets now that they take their bricks from one set of pieces (sora_amd/csrc/dev_11b.h): the
eight whole-capture kernels of the handle (k_rx11b*) and every stage kernel (k_11b_*).  Registers, scratch and LDS are read from the code-object
metadata of libsora_hip.so, without a GPU.  The figures are those of the library before the pieces were shared: LDS is a layout and
must be equal; registers and scratch must not grow (the four CCK kernels sit at 128 VGPRs and already spill)."""
import re

from test_isa_stream11b_cpu import kernel_metadata

#          kernel                    vgpr_count, private_segment_fixed_size, group_segment_fixed_size
BUDGET = {"k_rx11b":                 (90, 0, 27136),
          "k_rx11b_cck":             (128, 40, 35840),
          "k_rx11b_stream":          (86, 0, 27136),
          "k_rx11b_cck_stream":      (128, 104, 35840),
          "k_rx11b_pre":             (88, 0, 27136),
          "k_rx11b_cck_pre":         (128, 28, 35840),
          "k_rx11b_stream_pre":      (85, 0, 27136),
          "k_rx11b_cck_stream_pre":  (128, 108, 35840),
          "k_11b_dc_remove":         (4, 0, 0),
          "k_11b_energy_detect":     (21, 0, 588),
          "k_11b_symtiming":         (42, 0, 7948),
          "k_11b_barker_sync":       (68, 0, 324),
          "k_11b_despread":          (23, 0, 11264),
          "k_11b_sfd_sync":          (18, 0, 300),
          "k_11b_demapILi1EE":       (19, 0, 9216),
          "k_11b_demapILi2EE":       (15, 0, 5120),
          "k_11b_cckILi5EE":         (62, 0, 17408),
          "k_11b_cckILi11EE":        (35, 0, 9216),
          "k_11b_desc741":           (5, 0, 0),
          "k_11b_stream_state":      (8, 0, 0),
          "k_11b_plcp_parse":        (11, 0, 0),
          "k_11b_frame_sink":        (7, 0, 1024)}


def test_both_forms_of_the_11b_graph_keep_their_register_scratch_and_lds_budgets(tmp_path):
    md = {**kernel_metadata(tmp_path, b"k_rx11b"), **kernel_metadata(tmp_path, b"k_11b_")}
    names = {re.sub(r"^_ZN4sora\d+(k_11b_(?:demap|cck)ILi\d+EE|k_\w+?)E.*$", r"\1", k): v for k, v in md.items()}
    stage = sorted(k for k in names if k.startswith("k_11b_"))
    assert stage == sorted(k for k in BUDGET if k.startswith("k_11b_")), "the stage kernels of k_11b.hip and the budget table differ: %s" % stage
    for k, (vgpr, scratch, lds) in BUDGET.items():
        assert k in names, "kernel %s missing from libsora_hip.so (found %s)" % (k, sorted(names))
        assert names[k]["group_segment_fixed_size"] == lds, (k, names[k])
        assert names[k]["vgpr_count"] <= vgpr, (k, names[k])
        assert names[k]["private_segment_fixed_size"] <= scratch, (k, names[k])
