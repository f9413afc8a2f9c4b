"""tests/viterbi56_model.py (tests/cxx/viterbi56_model.c) is the definition k_viterbi56_11n is held to.  It restates oracle/so_rx11a.c::so_viterbi_frame_ex with a
fourth puncture branch and one changed rule inside that branch; here the restatement is held to the oracle byte for byte at rates 0..2 -- on random streams and on the
recorded adversarial streams of tests/golden/trellis_adversarial.npz, under both window schedules -- which shows that it adds the branch and nothing else.  At rate 5/6
it decodes its own encoder's clean codewords at every length the GPU test uses, and the new export is in the header, exported and typed."""
import ctypes
import os

import numpy as np
import pytest

import trellis_streams as ts
import viterbi56_model as vm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("cr", (0, 1, 2))
def test_model_equals_the_oracle_on_random_streams(oracle, cr):
    rng = np.random.default_rng(100 + cr)
    for L in list(range(1, 40)) + [51, 98, 100, 255, 700, 1500]:
        s = rng.integers(0, 8, ts.nsoft_for(L, cr, ts.GB[cr] * (L % 4))).astype(np.uint8)
        for win, look in ts.SCHEDULES.values():
            want = oracle.viterbi_frame_ex(s, cr, L, win, look)
            assert len(want) == L + 2
            assert np.array_equal(vm.viterbi_frame(s, cr, L, win, look), want), (cr, L, win, look)


@pytest.mark.parametrize("cr", (0, 1, 2))
def test_model_equals_the_oracle_on_the_recorded_adversarial_streams(oracle, golden_dir, cr):
    z = np.load(os.path.join(golden_dir, "trellis_adversarial.npz"))
    soft, nsoft, lens = z["soft_%d" % cr], z["nsoft_%d" % cr], z["len_%d" % cr]
    offs = np.concatenate([[0], np.cumsum(nsoft)])
    oo = np.concatenate([[0], np.cumsum(lens + 2)])
    assert len(lens) >= 60
    for name, (win, look) in ts.SCHEDULES.items():
        rec = z["out%s_%d" % (name, cr)]
        for i in range(len(lens)):
            s = soft[offs[i]:offs[i + 1]]
            got = vm.viterbi_frame(s, cr, int(lens[i]), win, look)
            assert np.array_equal(got, rec[oo[i]:oo[i + 1]]), (cr, name, i)                   # what the reference itself made of the stream
            if i % 8 == 0:
                assert np.array_equal(got, oracle.viterbi_frame_ex(s, cr, int(lens[i]), win, look)), (cr, name, i)


def test_rate_56_puncture_pattern():
    """A1 B1 A2 B3 A4 B5: the rate 3/4 pattern's four bits, then A of the fourth step and B of the fifth (against the unpunctured rate 1/2 stream)"""
    bits = np.random.default_rng(1).integers(0, 2, 50).astype(np.uint8)
    half = vm.encode(bits, 0).reshape(-1, 2)                                                  # (A_t, B_t)
    want = np.concatenate([[half[t, 0], half[t, 1], half[t + 1, 0], half[t + 2, 1], half[t + 3, 0], half[t + 4, 1]] for t in range(0, 50, 5)])
    assert np.array_equal(vm.encode(bits, vm.CR_56), want)
    assert np.array_equal(vm.encode(bits[:48], 2), np.concatenate([[half[t, 0], half[t, 1], half[t + 1, 0], half[t + 2, 1]] for t in range(0, 48, 3)]))
    # the encoder is the one the other rates' test streams are made with (tests/trellis_streams.py: 133 / 171)
    x = np.concatenate([np.zeros(6, np.uint8), bits]); d = lambda k: x[6 - k:len(x) - k]
    assert np.array_equal(half[:, 0], d(0) ^ d(2) ^ d(3) ^ d(5) ^ d(6)) and np.array_equal(half[:, 1], d(0) ^ d(1) ^ d(2) ^ d(3) ^ d(6))


@pytest.mark.parametrize("sched", sorted(ts.SCHEDULES))
def test_model_decodes_its_clean_rate_56_codewords(sched):
    win, look = ts.SCHEDULES[sched]
    rng = np.random.default_rng(56)
    for L in list(range(1, 130)) + [700, 1500, 4000]:
        payload = rng.integers(0, 256, L + 2, dtype=np.uint8)
        for extra in (0, 1, 7):
            s = vm.clean_stream(payload.tobytes(), extra_groups=extra)
            assert len(s) % 6 == 0 and len(s) >= vm.nsoft_of(L)
            assert np.array_equal(vm.viterbi_frame(s, vm.CR_56, L, win, look), payload), (L, extra)
    # a few errors per window are corrected (free distance 4 at rate 5/6: isolated single errors, far apart)
    payload = rng.integers(0, 256, 502, dtype=np.uint8)
    s = vm.clean_stream(payload.tobytes())
    s[40::97] = 7 - s[40::97]
    assert np.array_equal(vm.viterbi_frame(s, vm.CR_56, 500), payload)


def test_model_stops_with_its_soft_values():
    """a stream that ends before its frame yields whole windows only; values short of a group are not decoded"""
    rng = np.random.default_rng(3)
    s = rng.integers(0, 8, vm.nsoft_of(100)).astype(np.uint8)
    whole = vm.viterbi_frame(s, vm.CR_56, 100)
    assert len(whole) == 102
    assert len(vm.viterbi_frame(s[:6 * 46], vm.CR_56, 100)) == 0                              # 230 steps: no window yet
    cut = vm.viterbi_frame(s[:6 * 47 + 5], vm.CR_56, 100)                                     # 235 steps and five values more
    assert len(cut) == 24 and np.array_equal(cut, vm.viterbi_frame(s[:6 * 47], vm.CR_56, 100))
    assert len(vm.viterbi_frame(s[:5], vm.CR_56, 100)) == 0


def test_stage_export_is_declared_exported_and_typed():
    import sora_amd
    from sora_amd import capi
    lib = sora_amd.load()
    hdr = open(os.path.join(ROOT, "include", "sora_hip.h")).read()
    assert "enum { SORA_CR_56 = 3 };" in hdr and capi.CR_56 == 3 == vm.CR_56 and sora_amd.CR_56 == 3
    assert "int sora_hip_viterbi56_11n(" in hdr and "sora_hip_viterbi56_11n" in capi.EXPORTS
    assert len(lib.sora_hip_viterbi56_11n.argtypes) == 9 and callable(sora_amd.viterbi56_11n)
    assert lib.sora_hip_abi_version() == 4                                                    # additive
    p = ctypes.c_void_p(256)
    assert lib.sora_hip_viterbi56_11n(None, 64, p, p, p, p, p, 1, None) == -1                 # SORA_ERR_INVALID_PARAM, by name
    assert b"sora_hip_viterbi56_11n" in lib.sora_hip_last_error()
    assert lib.sora_hip_viterbi56_11n(p, 64, p, p, p, p, p, 0, None) == 0                     # nothing to launch: true with or without a device
    if sora_amd.device_count() == 0:
        assert lib.sora_hip_viterbi56_11n(p, 64, p, p, p, p, p, 1, None) == -5                # no CPU path
