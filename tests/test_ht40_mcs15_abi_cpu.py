"""MCS 15 on the 40 MHz HT pair, without a GPU: the new exports are declared, exported and typed by the binding; the sample counts of the gated transmit entry points
follow the closed form on both sides of every symbol step and equal the _gi forms at gate 14; refusals come in the existing order; the gated plans are held to a closed
form over MCS 0..31 x length 0..4100 x gates 13..16 by a stand-alone program built with the host sanitizers (tests/cxx/ht40_mcs15_plan_check.hip); the pure function
sora_ht40_symbols knows rate 5/6 (its joint sibling keeps answering 0); and the ABI version stays 4."""
import ctypes
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sora_hip_viterbi56_11n", "sora_ht40_set_mcs_max", "sora_hip_tx_ht40_mcs", "sora_hip_tx_ht40_mcs_samples", "sora_hip_tx_ht40_joint_mcs",
       "sora_hip_tx_ht40_joint_mcs_samples")


@pytest.fixture(scope="module")
def sora():
    import sora_amd
    sora_amd.load()
    return sora_amd


def test_new_exports_are_declared_exported_and_typed(sora):
    from sora_amd import capi
    L = sora.load()
    hdr = open(os.path.join(ROOT, "include", "sora_hip.h")).read()
    for n in NEW:
        assert n + "(" in hdr and n in capi.EXPORTS and hasattr(L, n) and getattr(L, n).argtypes is not None, n
    assert len(L.sora_hip_tx_ht40_mcs.argtypes) == len(L.sora_hip_tx_ht40_gi.argtypes) + 1 == 12
    assert len(L.sora_hip_tx_ht40_mcs_samples.argtypes) == 4 and L.sora_hip_tx_ht40_mcs_samples.restype is ctypes.c_size_t
    assert "#define SORA_HIP_ABI_VERSION 4" in hdr and L.sora_hip_abi_version() == 4       # this change only adds
    assert "enum { SORA_CR_56 = 3 };" in hdr
    assert callable(sora.RxHt40.set_mcs_max)


def test_sample_counts_on_both_sides_of_every_symbol_step(sora):
    for joint in (False, True):
        nd = 1080 if joint else 540
        gi_form = sora.tx_ht40_joint_gi_samples if joint else sora.tx_ht40_gi_samples
        steps = sorted({(n * nd - 22) // 8 - 4 for n in range(1, 62)} | {1, 2, 3995})
        for ln in [l for s in steps for l in (s, s + 1) if 1 <= l <= 3996]:
            nsym = -(-(16 + 8 * (ln + 4) + 6) // nd)
            for gi in (0, 1):
                assert sora.tx_ht40_samples(ln, 15, 15, gi, joint=joint) == 1600 + (144 if gi else 160) * nsym, (joint, ln, gi)
                assert sora.tx_ht40_samples(ln, 15, 14, gi, joint=joint) == 0
                for mcs in (8, 11, 14):
                    assert sora.tx_ht40_samples(ln, mcs, 15, gi, joint=joint) == sora.tx_ht40_samples(ln, mcs, 14, gi, joint=joint) == gi_form(ln, mcs, gi), (joint, ln, mcs, gi)
        for ln, mcs, gi, gate in ((0, 15, 0, 15), (3997, 15, 0, 15), (100, 16, 0, 15), (100, 7, 0, 15), (100, 15, 2, 15), (100, 15, 0, 13), (100, 15, 0, 16), (100, 9, 0, 16),
                                  (100, 9, 0, 0), (100, 9, 0, -1)):
            assert sora.tx_ht40_samples(ln, mcs, gate, gi, joint=joint) == 0, (joint, ln, mcs, gi, gate)
    assert sora.tx_ht40_samples(3996, 15, 15, 0) == 1600 + 160 * 60 and sora.tx_ht40_samples(3996, 15, 15, 1, joint=True) == 1600 + 144 * 30


def test_pure_symbol_counts_know_rate_56(sora):
    for nb in (1, 2, 4, 6):
        for ln in (4, 5, 64, 65, 700, 4000):
            assert sora.ht40_symbols(ln, ln - 1, nb, 3) == -(-(22 + 8 * ln) // (90 * nb))
            assert sora.ht40_symbols_joint(ln, nb, 3) == 0                      # (pinned at 0 by tests/test_ht40_joint_abi_cpu.py since before the rate existed)
    assert sora.ht40_symbols(100, 100, 6, 4) == 0 and sora.ht40_symbols_joint(100, 6, 4) == 0 and sora.ht40_symbols(100, 100, 3, 3) == 0


def test_entry_points_refuse_in_the_existing_order(sora):
    L = sora.load()
    p = ctypes.c_void_p(16)
    for fn, name in ((L.sora_hip_tx_ht40_mcs, b"sora_hip_tx_ht40_mcs"), (L.sora_hip_tx_ht40_joint_mcs, b"sora_hip_tx_ht40_joint_mcs")):
        for gate in (13, 16, 0, -1):                                      # the gate first: it is this form's own argument
            assert fn(p, p, p, p, p, p, 1, p, p, p, gate, None) == -1 and name + b": mcs_max" in L.sora_hip_last_error()
        if sora.device_count() == 0:
            assert fn(p, p, p, p, p, p, 1, p, p, p, 15, None) == -5       # then a device, as the _gi forms
        else:
            assert fn(None, p, p, p, p, p, 1, p, p, p, 15, None) == -1 and b"null pointer" in L.sora_hip_last_error()
            assert fn(p, p, p, p, p, p, 0, p, p, p, 15, None) == 0
    assert L.sora_ht40_set_mcs_max(None, 15) == -1 and b"sora_ht40_set_mcs_max" in L.sora_hip_last_error()


def test_python_wrappers_refuse_before_any_launch(sora):
    for kw in ({}, {"mcs_max": 14}, {"mcs_max": 13}, {"mcs_max": 16}, {"gi": [1]}):
        with pytest.raises(sora.SoraError):
            sora.tx_ht40([b"\x01\x02"], [b"\x03\x04"], [15], **kw)
        with pytest.raises(sora.SoraError):
            sora.tx_ht40_joint([b"\x01\x02"], [15], **kw)
    with pytest.raises(sora.SoraError):
        sora.tx_ht40([b"\x01\x02"], [b"\x03\x04"], [9], mcs_max=16)      # a bad gate is refused whatever the MCS


def test_gated_plans_against_the_closed_form(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.fail("hipcc not found: the plan check is a program of its own")
    exe = str(tmp_path / "ht40_mcs15_plan_check")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-std=c++17", "-O1", "-Xarch_host", "-fsanitize=address,undefined", "-I", os.path.join(ROOT, "sora_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cxx", "ht40_mcs15_plan_check.hip"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "OK" in r.stdout and not r.stderr.strip(), (r.returncode, r.stdout[-400:], r.stderr[-400:])
