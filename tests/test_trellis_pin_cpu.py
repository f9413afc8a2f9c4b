"""The oracle's trellis schedules pinned to the reference on adversarial soft streams (tests/trellis_streams.py), at every code rate:
Oracle.viterbi_frame (T11aViterbi<..,256,24>, the 802.11a graph's decoder) against Reference.viterbi_frame, and Oracle.viterbi_frame_ex(.., 192, 36)
(T11aViterbi<..,312,192,36>, the 802.11n graph's, fb11ndemod_config.hpp:199) against Reference.viterbi_frame_ex -- the reference's own TViterbiCore
driven with the same schedule (oracle/ref_shim.cpp).  The live comparisons run where oracle/_ref is built; tests/golden/trellis_adversarial.npz holds
a recorded subset with the reference's outputs, so the pin stands where the reference tree is absent.  The unit plan restated in
trellis_streams.py (where the GPU test puts its bursts) is checked against dev_winplan.h itself."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import trellis_streams as ts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATES = (0, 1, 2)


def _families(cr, sched):
    jobs = ts.ties(cr) + ts.wrap(cr)
    for njobs in (1, 64, 4096):
        jobs += ts.bursts(cr, sched, njobs, 8)[0]
    jobs += ts.lengths(cr, sched)[:132] + ts.batch(cr, 65)
    return jobs


def _both(oracle, reference, sched):
    if sched == "11a":
        return (lambda s, cr, L: oracle.viterbi_frame(s, cr, L)), (lambda s, cr, L: reference.viterbi_frame(s, cr, L))
    win, look = ts.SCHEDULES[sched]
    return (lambda s, cr, L: oracle.viterbi_frame_ex(s, cr, L, win, look)), (lambda s, cr, L: reference.viterbi_frame_ex(s, cr, L, win, look))


@pytest.mark.parametrize("sched", ["11a", "11n"])
@pytest.mark.parametrize("cr", RATES)
def test_oracle_equals_reference_on_adversarial_streams(oracle, reference, cr, sched):
    mine, ref = _both(oracle, reference, sched)
    for i, (s, L) in enumerate(_families(cr, sched)):
        want = ref(s, cr, L)
        assert len(want) == L + 2, (sched, cr, i, L)
        assert np.array_equal(mine(s, cr, L), want), (sched, cr, i, L)


def test_reference_schedule_ex_is_the_plain_one_at_256_24(reference):
    rng = np.random.default_rng(7)
    for cr in RATES:
        for L in (1, 33, 500):
            s = rng.integers(0, 8, ts.nsoft_for(L, cr, 48)).astype(np.uint8)
            assert np.array_equal(reference.viterbi_frame_ex(s, cr, L, 256, 24), reference.viterbi_frame(s, cr, L))


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "trellis_adversarial.npz"))


@pytest.mark.parametrize("cr", RATES)
def test_oracle_equals_recorded_reference(oracle, golden, cr):
    soft, nsoft, lens = golden["soft_%d" % cr], golden["nsoft_%d" % cr], golden["len_%d" % cr]
    assert len(lens) >= 60 and soft.max() == 7 and soft.min() == 0
    offs = np.concatenate([[0], np.cumsum(nsoft)])
    oo = np.concatenate([[0], np.cumsum(lens + 2)])
    assert offs[-1] == len(soft)
    for name, (win, look) in ts.SCHEDULES.items():
        out = golden["out%s_%d" % (name, cr)]
        assert oo[-1] == len(out)
        for i, L in enumerate(lens):
            s = soft[offs[i]:offs[i + 1]]
            got = oracle.viterbi_frame(s, cr, int(L)) if name == "11a" else oracle.viterbi_frame_ex(s, cr, int(L), win, look)
            assert np.array_equal(got, out[oo[i]:oo[i + 1]]), (name, cr, i, int(L))


def test_recorded_subset_is_what_the_generator_makes(golden):
    """the fixture's inputs are tests/golden/make_golden.py's trellis_subset(): the families have not drifted from what was recorded"""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    from make_golden import trellis_subset
    for cr in RATES:
        jobs = trellis_subset(cr)
        assert np.array_equal(np.concatenate([s for s, _ in jobs]), golden["soft_%d" % cr])
        assert [L for _, L in jobs] == list(golden["len_%d" % cr])


WINPLAN = r"""
#define __host__
#define __device__
#include "dev_winplan.h"
extern "C" {
unsigned w_events(unsigned length, unsigned cr, unsigned win, unsigned look) { return sora::win_events(length, cr, win, look); }
unsigned w_units_per_frame(unsigned n, unsigned target) { return sora::win_units_per_frame(n, target); }
unsigned w_per_unit(unsigned nev, unsigned q) { return sora::win_per_unit(nev, q); }
}
"""


def test_unit_plan_restatement_is_dev_winplan(tmp_path):
    src = tmp_path / "wp.cpp"; src.write_text(WINPLAN)
    so = tmp_path / "libwp.so"
    subprocess.check_call(["g++", "-O1", "-shared", "-fPIC", "-I", os.path.join(ROOT, "sora_amd", "csrc"), str(src), "-o", str(so)])
    L = ctypes.CDLL(str(so))
    for f in ("w_events", "w_units_per_frame", "w_per_unit"):
        getattr(L, f).restype = ctypes.c_uint
    for win, look in ts.SCHEDULES.values():
        for cr in RATES:
            for n in list(range(1, 400)) + list(range(900, 1100)) + list(range(2200, 2400)) + list(range(4000, 4096)):
                assert ts.win_events(n, cr, win, look) == L.w_events(n, cr, win, look), (win, cr, n)
    for n in (1, 2, 7, 64, 65, 204, 205, 4095, 4096, 8192, 16384, 16385, 100000):
        q = ts.units_per_frame(n)
        assert q == L.w_units_per_frame(n, ts.TARGET)
        for nev in range(1, 140):
            assert ts.win_per_unit(nev, q) == L.w_per_unit(nev, q)
    assert ts.verify_points(1000, 0, 64, "11a")[:3] == [240, 504, 768]      # floor24(256 k): units of one window
    assert ts.verify_points(1000, 0, 4096, "11a") == [2304, 4608, 6912]     # 4096 jobs: four units of nine windows


def test_every_family_is_well_formed():
    for cr in RATES:
        for sched in ts.SCHEDULES:
            for s, L in _families(cr, sched):
                assert s.dtype == np.uint8 and s.max() <= 7 and len(s) % ts.GB[cr] == 0
                assert len(s) // ts.GB[cr] * ts.GS[cr] >= 8 * L + 22
