"""The nine stage entry points of the 40 MHz HT receiver, the parts that need no GPU: declared in include/sora_hip.h, exported, bound and typed; each refuses a null
pointer by name and a bad n_bpsc, and accepts a count of 0; optional pointers are optional; the composition sora_amd.rx_ht40_stages over the model's bricks reproduces
oracle/ht40_data_model.py.  (This file fails without the feature: the names do not exist.)"""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SORA_OK, SORA_ERR_INVALID_PARAM, SORA_ERR_NO_DEVICE = 0, -1, -5
P = ctypes.c_void_p(4096)                                                        # a pointer that is not null and is never followed: every check below comes first

# name -> (arguments with every pointer set and counts of 1, the indices of the REQUIRED pointers, the index of the count, the indices of the optional pointers)
STAGES = {
    "sora_hip_data_symbol_ht40":  ([P, P, P, P, P, P, P, 1, 1, None], (0, 1, 2, 3, 4, 5, 6), 7, ()),
    "sora_hip_mimo_est_ht40":     ([P, P, P, P, P, 1, None], (0, 1, 4), 5, (2, 3)),
    "sora_hip_mimo_comp_ht40":    ([P, P, P, P, P, P, 1, None], (0, 2, 3, 4, 5), 6, (1,)),
    "sora_hip_pilot_track_ht40":  ([P, P, P, P, P, P, 1, None], (0, 1, 2, 3, 4), 6, (5,)),
    "sora_hip_demap_ht40":        ([P, P, 2, 1, None], (0, 1), 3, ()),
    "sora_hip_deinterleave_ht40": ([P, P, 4, 1, 1, None], (0, 1), 4, ()),
    "sora_hip_stream_join_ht40":  ([P, P, P, 6, 1, None], (0, 1, 2), 4, ()),
    "sora_hip_downsample_ht40":   ([P, P, P, P, P, P, P, P, 1, 1, None], (0, 1, 2, 3, 4, 5, 6, 7), 8, ()),
    "sora_hip_noise_var_ht40":    ([P, P, P, P, 1, None], (0, 1, 3), 4, (2,)),
}
N_BPSC_ARG = {"sora_hip_demap_ht40": 2, "sora_hip_deinterleave_ht40": 2, "sora_hip_stream_join_ht40": 3}


@pytest.fixture(scope="module")
def lib():
    import sora_amd
    return sora_amd.load()


def test_the_nine_are_declared_exported_bound_and_typed(lib):
    from sora_amd import capi
    assert len(STAGES) == 9
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sora_hip.h")).read(), flags=re.S)
    for name, (args, _, _, _) in STAGES.items():
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in capi.EXPORTS and hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None and len(getattr(lib, name).argtypes) == len(args), name
    assert lib.sora_hip_abi_version() == 4
    import sora_amd.build as b
    assert "k_ht40_stages.hip" in b.SOURCES


def test_python_surface():
    import sora_amd
    for name in ("data_symbol_ht40", "mimo_est_ht40", "mimo_comp_ht40", "pilot_track_ht40", "demap_ht40", "deinterleave_ht40", "stream_join_ht40", "downsample_ht40",
                 "noise_var_ht40", "rx_ht40_stages", "rx_ht40_by_stages", "rx_ht40_front_stages", "rx_ht40_front_by_stages", "ht40_sig_gate"):
        assert callable(getattr(sora_amd, name)), name
    assert "not a fast path" in sora_amd.rx_ht40_by_stages.__doc__ and "not a fast path" in sora_amd.rx_ht40_front_by_stages.__doc__


@pytest.mark.parametrize("name", sorted(STAGES))
def test_a_null_pointer_is_refused_by_name(lib, name):
    args, ptrs, _, _ = STAGES[name]
    for i in ptrs:
        a = list(args); a[i] = None
        assert getattr(lib, name)(*a) == SORA_ERR_INVALID_PARAM, (name, i)
        assert name.encode() in lib.sora_hip_last_error(), (name, i, lib.sora_hip_last_error())


@pytest.mark.parametrize("name", sorted(N_BPSC_ARG))
@pytest.mark.parametrize("nb", [0, 3, 5, 7, 8, -1])
def test_a_bad_n_bpsc_is_refused_even_with_nothing_to_do(lib, name, nb):
    args, _, ncount, _ = STAGES[name]
    for count in (0, 1):
        a = list(args); a[N_BPSC_ARG[name]] = nb; a[ncount] = count
        assert getattr(lib, name)(*a) == SORA_ERR_INVALID_PARAM, (name, nb)
        assert name.encode() in lib.sora_hip_last_error()
    if name == "sora_hip_deinterleave_ht40":
        a = list(args); a[3] = 2
        assert getattr(lib, name)(*a) == SORA_ERR_INVALID_PARAM


@pytest.mark.parametrize("name", sorted(STAGES))
def test_a_count_of_zero_is_accepted_and_nothing_computes_without_a_device(lib, name):
    import sora_amd
    args, _, ncount, optional = STAGES[name]
    a = list(args); a[ncount] = 0
    assert getattr(lib, name)(*a) == SORA_OK, name
    for i in optional:                                                          # an optional pointer may be null: the call gets as far as the device check
        a = list(args); a[i] = None; a[ncount] = 0
        assert getattr(lib, name)(*a) == SORA_OK, (name, i)
    if sora_amd.device_count() <= 0:
        assert getattr(lib, name)(*args) == SORA_ERR_NO_DEVICE, name
        assert b"no HIP device" in lib.sora_hip_last_error()


def test_rx_ht40_stages_over_the_model_ops_reproduces_the_data_model():
    """two frames of different modulation, length and code rate in one call, one zero-forcing and one MMSE, with a described carrier offset"""
    import sora_amd
    from oracle import ht40_data_model as dm
    import ht40_stage_model as sm
    from test_ht40_data_model import send
    rng = np.random.default_rng(40)
    a, psa, _, na = send(rng, 2, 2, (52, 31), 5.0, cfo_step=21.0, lead=6)
    b, psb, _, nb_ = send(rng, 6, 1, (97, 120), 5.0, lead=1)
    iq = np.concatenate([a, b], axis=1)
    descs = [(6, 2, 2, 52, 31, -21, 0.0), (a.shape[1] + 1, 6, 1, 97, 120, 0, 0.39)]
    r = sora_amd.rx_ht40_stages(sm.ModelOps(), iq[0], iq[1], descs)
    assert [x["nsym"] for x in r["rows"]] == [na, na, nb_, nb_] and sora_amd.ht40_frame_symbols(descs[0]) == na
    for f, (d, ps) in enumerate(zip(descs, (psa, psb))):
        want = dm.model(iq, d[0], d[1], d[2], (d[3], d[4]), d[5], np.asarray(r["weights"][f]))
        assert np.array_equal(r["theta"][f], want.theta)
        for s in range(2):
            assert np.array_equal(r["soft"][f][s], want.soft[s])
            row = r["rows"][2 * f + s]
            assert (row["error_code"], row["crc32"], row["mpdu"], row["length"]) == (want.streams[s].error_code, want.streams[s].crc32, want.streams[s].psdu, d[3 + s])
            assert row["error_code"] == 1 and row["mpdu"] == ps[s]
    with pytest.raises(ValueError):
        sora_amd.rx_ht40_stages(sm.ModelOps(), iq[0], iq[1], [(0, 3, 0, 50, 50, 0, 0.0)])
    with pytest.raises(ValueError):
        sora_amd.rx_ht40_stages(sm.ModelOps(), iq[0], iq[1], [(0, 2, 0, 50, 50, 0, 0.0)], coding=1)
    assert sora_amd.rx_ht40_stages(sm.ModelOps(), iq[0], iq[1], [])["rows"] == []
