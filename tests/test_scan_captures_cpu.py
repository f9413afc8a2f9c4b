"""The capture families of tests/scan_captures.py on the CPU: the restatement (oracle/so_rx11a.c) reports on every one of them exactly what the compiled
reference graph reports, so it is a valid yardstick for k_scan there (tests/test_gpu_scan_sense.py); and together the families reach every branch class of
carrier sense that the restatement counts (so_oracle.h: SO_CS_*), the two rare ones included:
  * a true carrier test between E_CS_TIMEOUT being raised and the end of its source call (k_scan.hip: the `K` limit behind a raise, `to_pending`),
  * a lock dropped on the burst at which dc_update_cnt == 0 (k_scan.hip: the DC update inside the locked phase).
The totals are the restatement's own, pinned: a change to a generator or to the restatement's carrier sense shows here first."""
import numpy as np
import pytest

import scan_captures as sc
from gpu_util import same_as_reference_graph
from oracle.pyoracle import CS_COUNTERS, CS_RECORD_MAGIC, ReferenceGraph

FLOOR = 8                       # every class at least this often

TOTALS = {"true_test": 36039, "est_lock": 8522, "est_no_lock": 10022, "est_lock_late_peak": 7358, "lock_dropped": 4073, "lock_dropped_dc_update": 88,
          "frame_detected": 4448, "peak_raised": 5391, "dc_update": 75295, "timeout_raised": 31518, "true_test_timeout_pending": 86}

COUNTS = {"dc_steps": 1120, "sts_fragments": 528, "blip_gap_frame": 1200, "lead_sweep": 896, "gap_sweep": 448, "many_frames": 5, "loud_noise": 36,
          "composite_stream": 1}


def test_the_families_are_what_the_issue_describes(oracle):
    fam = sc.families(oracle)
    assert {k: len(v) for k, v in fam.items()} == COUNTS
    for name, caps in fam.items():
        for c in caps:
            assert c.dtype == np.int16 and c.ndim == 2 and c.shape[1] == 2 and len(c) % 28 == 0, name
    assert len(sc.frame(oracle)) == 960
    assert len(fam["composite_stream"][0]) == 18200
    # seeded: a second generation gives the same samples
    again = sc.lead_sweep(oracle)
    assert all(np.array_equal(a, b) for a, b in zip(again, fam["lead_sweep"]))


def test_the_counters_are_inert_unless_asked_for(oracle):
    cap = sc.families(oracle)["blip_gap_frame"][7]
    oracle.cs_counters(False)
    before = oracle.rx_capture(cap, 40)
    assert set(oracle.cs_counters_read().values()) == {0}
    oracle.cs_counters(True)
    assert oracle.rx_capture(cap, 40) == before
    c = oracle.cs_counters_read()
    assert tuple(c) == CS_COUNTERS and c["true_test"] >= 4 and c["frame_detected"] == 1 and c["dc_update"] > 0
    oracle.cs_counters(False)
    assert set(oracle.cs_counters_read().values()) == {0}
    assert oracle.rx_capture(cap, 40) == before and set(oracle.cs_counters_read().values()) == {0}


def test_the_families_reach_every_class_of_carrier_sense(oracle):
    fam = sc.families(oracle)
    oracle.cs_counters(True)
    try:
        for caps in fam.values():
            for c in caps:
                oracle.rx_capture(c, 40, max_frames=80)
        got = oracle.cs_counters_read()
    finally:
        oracle.cs_counters(False)
    print("carrier-sense classes over %d captures: %s" % (sum(COUNTS.values()), got))
    assert all(got[k] >= FLOOR for k in CS_COUNTERS), got
    assert got == TOTALS


def test_many_frames_all_decode(oracle):
    for nf, cap in zip(sc.MANY_FRAMES, sc.families(oracle)["many_frames"]):
        rows = oracle.rx_capture(cap, 40, max_frames=80)
        assert len(rows) == nf and all(r["error_code"] == 1 for r in rows)
        assert [r["rate_kbps"] for r in rows] == [(54000, 48000, 24000)[i % 3] for i in range(nf)]


def test_the_state_trace_of_the_composite_stream(oracle):
    """cs_trace: resume points lie on the source-call grid (the resampler's period at 44), in increasing order, the first at 0 in the reset state, the
    last at the stream's end; the 20 MHz form of the stream gives the same records but for the position word; the record counts the events in front."""
    x = sc.families(oracle)["composite_stream"][0]
    rows = oracle.rx_capture(x, 40)
    p40, r40 = oracle.cs_trace(x, 40)
    p20, r20 = oracle.cs_trace(x[::2].copy(), 20)
    p44, r44 = oracle.cs_trace(x, 44)
    assert oracle.rx_capture(x, 40) == rows                                    # tracing leaves nothing behind
    for p, r, grid in ((p40, r40, 14), (p20, r20, 14), (p44, r44, 140)):
        assert len(p) >= 40 and p[0] == 0 and p[-1] == len(x) // 2 and np.all(np.diff(p.astype(np.int64)) > 0) and np.all(p % grid == 0)
        assert np.all(r[:, 41] == CS_RECORD_MAGIC) and not r[:, 43:].any()
        assert not r[0, :35].any() and r[0, 35] == 8 and not r[0, 36:41].any() and r[0, 42] == 0
    assert np.array_equal(p40, p20) and np.array_equal(r40[:, 40], 2 * p40) and np.array_equal(r20[:, 40], p20) and np.array_equal(r44[:, 40], 2 * p44)
    keep = [w for w in range(64) if w != 40]
    assert np.array_equal(r40[:, keep], r20[:, keep])
    for p, r in zip(p40, r40):
        assert r[42] == sum(e["end_sample"] <= p for e in rows)
    assert r40[-1, 42] == len(rows) and len(rows) >= 5
    # the state moves: the DC estimate, the sums and the counters take several values over the stream, and some records hold the stale
    # high_count / peak_corr / peak_index of a lock that was dropped
    for w in (16, 28, 30, 35, 36, 38, 39):
        assert len(set(r40[:, w].tolist())) >= 4, w
    assert (r40[:, 33] != 0).sum() >= 4 and (r44[:, 33] != 0).sum() >= 2 and (r40[:, 32] != 0).any() and (r40[:, 34] != 0).any()
    assert len(set(r40[:, 31].tolist())) >= 3                                  # (sense_count at a resume point is a multiple of 28 below 84)
    assert len(set(r44[:, 38].tolist())) >= 4


@pytest.fixture(scope="module")
def graph():
    g = ReferenceGraph()
    if not g.available():
        pytest.skip("oracle/_ref/libsora_refgraph.so not built (needs the reference tree)")
    return g


@pytest.mark.parametrize("name", [n for n, _ in sc.FAMILIES])
def test_the_restatement_equals_the_reference_graph(oracle, graph, name):
    caps = sc.families(oracle)[name]
    nev = 0
    for i, cap in enumerate(caps):
        ev = graph.rx11a(cap, max_frames=80)
        ok, why = same_as_reference_graph(oracle.rx_capture(cap, 40, max_frames=80), ev)
        assert ok, "%s capture %d: %s" % (name, i, why)
        nev += len(ev)
    assert nev > 0 or name == "loud_noise"
