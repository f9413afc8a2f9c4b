"""The joint coding's entry points (sora_hip_tx_ht40_joint, sora_hip_tx_ht40_joint_samples, sora_ht40_symbols_joint, sora_ht40_set_coding), the parts that need no
GPU: they are exported, typed and declared in include/sora_hip.h; the sample and symbol counts are the model's on both sides of every symbol boundary; frames that
are not accepted count zero samples; the entry points refuse without a device and refuse null handles; the Python wrapper refuses before any launch."""
import ctypes
import os
import re

import pytest

from oracle import py_ht40 as m
import ht40_joint_model as J

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sora_hip.h")
NEW = ("sora_hip_tx_ht40_joint", "sora_hip_tx_ht40_joint_samples", "sora_ht40_symbols_joint", "sora_ht40_set_coding")


@pytest.fixture(scope="module")
def sora():
    import sora_amd
    sora_amd.load()
    return sora_amd


def _step_lengths(mcs, max_nsym=12):
    """lengths (without FCS) on both sides of every step of the joint N_SYM up to max_nsym, as tests/test_tx_ht40_cpu.py picks them for the per-stream coding"""
    nd = J.ndbps(*m.MCS2[mcs])
    out = []
    for n in range(1, max_nsym + 1):
        top = (n * nd - 22) // 8 - 4                                 # the longest MPDU that fits n symbols
        out += [v for v in (top, top + 1) if 1 <= v <= 3996]
    return sorted(set(out))


def test_exports_exist_are_typed_and_declared(sora):
    from sora_amd import capi
    L = sora.load()
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for n in NEW:
        assert n in capi.EXPORTS and hasattr(L, n) and getattr(L, n).argtypes is not None, n
        assert re.search(r"\b%s\s*\(" % n, txt), n
    assert re.search(r"#define\s+SORA_HT40_CODING_PER_STREAM\s+0\b", txt) and re.search(r"#define\s+SORA_HT40_CODING_JOINT\s+1\b", txt)
    assert L.sora_hip_tx_ht40_joint_samples.restype is ctypes.c_size_t and L.sora_hip_tx_ht40_joint_samples.argtypes == [ctypes.c_uint32] * 2
    assert len(L.sora_hip_tx_ht40_joint.argtypes) == 10 and L.sora_hip_tx_ht40_joint.argtypes[5] is ctypes.c_size_t
    assert L.sora_ht40_symbols_joint.restype is ctypes.c_uint32 and L.sora_ht40_symbols_joint.argtypes == [ctypes.c_uint32] * 3
    assert L.sora_ht40_set_coding.argtypes == [ctypes.c_void_p, ctypes.c_int]
    assert callable(sora.tx_ht40_joint) and callable(sora.tx_ht40_joint_samples) and callable(sora.ht40_symbols_joint) and callable(sora.RxHt40.set_coding)
    assert (sora.HT40_CODING_PER_STREAM, sora.HT40_CODING_JOINT) == (0, 1)
    assert L.sora_hip_abi_version() == 4                             # additions only


@pytest.mark.parametrize("mcs", range(8, 15))
def test_sample_and_symbol_counts(sora, mcs):
    nb, cr = m.MCS2[mcs]
    steps = _step_lengths(mcs)
    assert len({J.nsym_for(ln + 4, nb, cr) for ln in steps}) >= 12
    for ln in [1, 2, 3, 37, 1496, 3996] + steps:
        nsym = J.nsym_for(ln + 4, nb, cr)
        assert sora.tx_ht40_joint_samples(ln, mcs) == 1280 + 160 * (2 + nsym), (mcs, ln)
        assert sora.ht40_symbols_joint(ln + 4, nb, cr) == nsym, (mcs, ln)
    assert sora.ht40_symbols_joint(0, nb, cr) == 1


def test_the_extremes(sora):
    assert sora.ht40_symbols_joint(4000, 1, 0) == 297 and sora.tx_ht40_joint_samples(3996, 8) == 1280 + 160 * 299
    assert sora.ht40_symbols_joint(4000, 6, 1) * J.ndbps(6, 1) == 32832


@pytest.mark.parametrize("mcs,ln", [(7, 100), (15, 100), (32, 100), (8, 0), (14, 0), (8, 3997), (14, 3997)])
def test_frames_that_are_not_accepted_give_zero_samples(sora, mcs, ln):
    assert sora.tx_ht40_joint_samples(ln, mcs) == 0


@pytest.mark.parametrize("nb,cr", [(0, 0), (3, 0), (5, 1), (8, 0), (1, 3), (6, 7)])
def test_symbol_count_is_zero_for_bad_arguments(sora, nb, cr):
    assert sora.ht40_symbols_joint(100, nb, cr) == 0


def test_python_wrapper_refuses_before_any_launch(sora):
    for mp, mcs, seeds in (([b"\x01\x02"], [15], None), ([b"\x01\x02"], [7], None), ([b""], [9], None), ([bytes(3997)], [9], None), ([b"\x01"], [9, 10], None),
                           ([b"\x01"], [9], [(1, 2)]), ([b"\x01"], [9], [1, 2])):
        with pytest.raises(sora.SoraError):
            sora.tx_ht40_joint(mp, mcs, seeds)


def test_entry_points_refuse_without_a_device_and_null_arguments(sora):
    L = sora.load()
    p = ctypes.c_void_p(16)
    if sora.device_count() <= 0:
        assert L.sora_hip_tx_ht40_joint(p, p, p, p, None, 1, p, p, p, None) == -5
        assert b"no HIP device" in L.sora_hip_last_error()
        with pytest.raises(sora.SoraError) as e:
            sora.RxHt40(1, 1024)
        assert e.value.code == -5
    else:
        assert L.sora_hip_tx_ht40_joint(None, p, p, p, None, 1, p, p, p, None) == -1
        assert b"sora_hip_tx_ht40_joint: null pointer" in L.sora_hip_last_error()
    for coding in (-1, 0, 1, 2):                                     # a null handle is refused whatever is asked
        assert L.sora_ht40_set_coding(None, coding) == -1
        assert b"sora_ht40_set_coding: null handle" in L.sora_hip_last_error()
