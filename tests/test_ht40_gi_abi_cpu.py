"""The short guard interval's entry points (sora_hip_tx_ht40_gi, sora_hip_tx_ht40_joint_gi, their _samples, sora_ht40_set_guard), the parts that
need no GPU: they are exported, typed and declared in include/sora_hip.h with their constants; the sample counts are 1600 + 144 N_SYM (short) and the existing entry
points' (long) on both sides of every symbol boundary, and 0 for a refused kind, MCS or length; the entry points refuse in the existing ones' order (no device, then
null pointers; a null handle); no struct changed size; the Python wrappers refuse before any launch."""
import ctypes
import os
import re

import pytest

from oracle import py_ht40 as m
import ht40_joint_model as J

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sora_hip.h")
NEW = ("sora_hip_tx_ht40_gi", "sora_hip_tx_ht40_gi_samples", "sora_hip_tx_ht40_joint_gi", "sora_hip_tx_ht40_joint_gi_samples", "sora_ht40_set_guard")


@pytest.fixture(scope="module")
def sora():
    import sora_amd
    sora_amd.load()
    return sora_amd


def test_exports_exist_are_typed_and_declared(sora):
    from sora_amd import capi
    L = sora.load()
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for n in NEW:
        assert n in capi.EXPORTS and hasattr(L, n) and getattr(L, n).argtypes is not None, n
        assert re.search(r"\b%s\s*\(" % n, txt), n
    for name, value in (("SORA_HT40_SHORT_GI", "0x100u"), ("SORA_ROW_SHORT_GI", "4u"), ("SORA_HT40_GUARD_LONG", "0"), ("SORA_HT40_GUARD_SIGNALLED", "1")):
        assert re.search(r"#define\s+%s\s+%s\b" % (name, value), txt), name
    for fn in (L.sora_hip_tx_ht40_gi_samples, L.sora_hip_tx_ht40_joint_gi_samples):
        assert fn.restype is ctypes.c_size_t and fn.argtypes == [ctypes.c_uint32] * 3
    for fn in (L.sora_hip_tx_ht40_gi, L.sora_hip_tx_ht40_joint_gi):                # sora_hip_tx_ht40's arguments in its order, d_gi behind d_seed
        assert len(fn.argtypes) == 11 and fn.argtypes[6] is ctypes.c_size_t
    assert L.sora_ht40_set_guard.argtypes == [ctypes.c_void_p, ctypes.c_int]
    assert all(callable(f) for f in (sora.tx_ht40_gi_samples, sora.tx_ht40_joint_gi_samples, sora.RxHt40.set_guard))
    assert (sora.HT40_SHORT_GI, sora.ROW_SHORT_GI, sora.HT40_GUARD_LONG, sora.HT40_GUARD_SIGNALLED) == (0x100, 4, 0, 1)
    assert sora.ROW_SHORT_GI not in (sora.ROW_TRUNCATED, sora.ROW_SHORT_PREAMBLE) and sora.ROW_SHORT_GI & (sora.ROW_TRUNCATED | sora.ROW_SHORT_PREAMBLE) == 0
    assert L.sora_hip_abi_version() == 4                             # additions only


def test_no_struct_changed_size(sora):
    from sora_amd import capi
    assert ctypes.sizeof(capi.Ht40Found) == 32 and ctypes.sizeof(capi.Ht40Frame) == 40 and ctypes.sizeof(capi.FrameResult) == 36
    txt = open(HEADER).read()
    body = re.search(r"typedef struct \{([^}]*)\} sora_ht40_frame;", txt).group(1)
    assert re.findall(r"\b(\w+)(?:\[2\])?;", re.sub(r"/\*.*?\*/", "", body, flags=re.S)) == ["offset", "n_bpsc", "code_rate", "length", "cfo", "noise_var", "frame_id"]
    body = re.search(r"typedef struct \{([^}]*)\} sora_ht40_found;", txt).group(1)
    assert re.findall(r"\b(\w+)[;,]", re.sub(r"/\*.*?\*/", "", body, flags=re.S)) == ["a20", "mcs", "ht_len", "nsym", "cfo", "noise_var", "end_sample", "error_code"]


def _steps(nd, max_nsym=12):
    out = []
    for n in range(1, max_nsym + 1):
        top = (n * nd - 22) // 8 - 4
        out += [v for v in (top, top + 1) if 1 <= v <= 3996]
    return sorted(set(out))


@pytest.mark.parametrize("mcs", range(8, 15))
def test_sample_counts(sora, mcs):
    nb, cr = m.MCS2[mcs]
    for ln in [1, 2, 37, 1496, 3996] + _steps(m.ndbps(nb, cr)):
        n = m.nsym_for([ln + 4], nb, cr)
        assert sora.tx_ht40_gi_samples(ln, mcs, 1) == 1600 + 144 * n, (mcs, ln)
        assert sora.tx_ht40_gi_samples(ln, mcs, 0) == sora.tx_ht40_samples(ln, mcs) == 1600 + 160 * n, (mcs, ln)
    for ln in [1, 2, 37, 1496, 3996] + _steps(J.ndbps(nb, cr)):
        n = J.nsym_for(ln + 4, nb, cr)
        assert sora.tx_ht40_joint_gi_samples(ln, mcs, 1) == 1600 + 144 * n, (mcs, ln)
        assert sora.tx_ht40_joint_gi_samples(ln, mcs, 0) == sora.tx_ht40_joint_samples(ln, mcs) == 1600 + 160 * n, (mcs, ln)


@pytest.mark.parametrize("mcs,ln,gi", [(9, 100, 2), (9, 100, 3), (9, 100, 255), (9, 100, 0xFFFFFFFF), (7, 100, 1), (15, 100, 1), (8, 0, 1), (14, 3997, 1), (7, 100, 0), (8, 3997, 0)])
def test_refused_inputs_give_zero_samples(sora, mcs, ln, gi):
    assert sora.tx_ht40_gi_samples(ln, mcs, gi) == 0 and sora.tx_ht40_joint_gi_samples(ln, mcs, gi) == 0


def test_the_longest_frames(sora):
    assert sora.tx_ht40_gi_samples(3996, 8, 1) == 1600 + 144 * 593 and sora.tx_ht40_joint_gi_samples(3996, 8, 1) == 1600 + 144 * 297
    assert (1600 + 144 * 593) * 4 % 16 == 0                          # a frame that starts 16-byte aligned ends 16-byte aligned: 144 samples are 576 bytes


def test_python_wrappers_refuse_before_any_launch(sora):
    for gi in ([2], [0, 1], [-1], 7):
        with pytest.raises(sora.SoraError):
            sora.tx_ht40([b"\x01\x02"], [b"\x03\x04"], [9], gi=gi)
        with pytest.raises(sora.SoraError):
            sora.tx_ht40_joint([b"\x01\x02"], [9], gi=gi)
    with pytest.raises(sora.SoraError):
        sora.tx_ht40([b"\x01\x02"], [b"\x03\x04"], [15], gi=[1])


def test_entry_points_refuse_in_the_existing_order(sora):
    L = sora.load()
    p = ctypes.c_void_p(16)
    for fn, name in ((L.sora_hip_tx_ht40_gi, b"sora_hip_tx_ht40_gi"), (L.sora_hip_tx_ht40_joint_gi, b"sora_hip_tx_ht40_joint_gi")):
        if sora.device_count() <= 0:                                 # no device: said first, whatever the pointers are (host_stage.h's order)
            assert fn(None, p, p, p, None, None, 1, p, p, p, None) == -5
            assert b"no HIP device" in L.sora_hip_last_error()
        else:
            for k in (0, 1, 2, 3, 7, 8, 9):                          # d_seed and d_gi may be null; every other pointer may not
                args = [p, p, p, p, None, None, 1, p, p, p, None]; args[k] = None
                assert fn(*args) == -1, (name, k)
                assert name + b": null pointer" in L.sora_hip_last_error()
            assert fn(p, p, p, p, None, None, 0, p, p, p, None) == 0   # no frames: nothing to do
    for mode in (-1, 0, 1, 2):                                       # a null handle is refused whatever is asked
        assert L.sora_ht40_set_guard(None, mode) == -1
        assert b"sora_ht40_set_guard: null handle" in L.sora_hip_last_error()
