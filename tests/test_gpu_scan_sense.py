"""k_scan's carrier sense against the restated reference graph, bit for bit, on the capture families of tests/scan_captures.py -- the branches that frames
behind a quiet lead never reach (tests/test_scan_captures_cpu.py counts them and holds the restatement to the compiled reference graph on every capture):

  * ROWS: every family through sora.Rx as 40 MHz input, as 20 MHz input (the even samples) and under sample_rate_mhz = 44, with the automatic kernel choice
    and with the three-kernel chain (set_front(3): the only chain k_scan fills slot_row for); every row and MPDU byte equals oracle.rx_capture's.
  * STATE: in stream mode k_scan stores the whole carrier-sense state at every resume point (k_scan.hip: cont_store).  sora_rx_stream_record_of reads it,
    and every word is held to the restatement's state at that point (Oracle.cs_trace) -- for every prefix of one composite stream, at 40 MHz (where stream
    mode cuts a pass at seven bursts), at 20 MHz and in 44 MHz mode (resume points 140 samples apart: passes of up to sixteen bursts with their state
    visible).  No word is excluded: 0-40 and 42 are state, 41 the magic, 43-63 zero.  Every family capture's last record is checked the same way.
  * CONTINUATION: a stream cut twice; the second call starts from the first one's record.  Its record equals the uncut stream's state there, and the rows of
    both calls are the uncut stream's.

What these tests cannot hold, because nothing observable depends on it: the outcome of a carrier test BETWEEN a time-out being raised and the end of its source
call (k_scan.hip: the passes under to_pending).  That window is at most three bursts; establish_sync needs four true tests in a row and auto_count is 0 at the
raise (21 false tests led to it); the DC estimator is fed either way; and the reset at the window's end clears auto_count and sense_count.  A true test IN
FRONT of the raise (it moves the raise into the middle of a source call) is held: the blip_gap_frame family is built for it."""
import ctypes

import numpy as np
import pytest

import scan_captures as sc
from gpu_util import batch, make_capture, same_results
from oracle.pyoracle import CS_RECORD_MAGIC

pytestmark = pytest.mark.gpu

RATES = (40, 20, 44)
_memo = {}


@pytest.fixture(scope="module")
def sora():
    import sora_amd
    sora_amd.load()
    assert sora_amd.device_count() > 0
    return sora_amd


def _at_rate(cap, rate):
    """the capture as the handle of that rate takes it: 20 = the even samples (whole 14-sample source calls again, as the raw capture is whole 28s);
    44 = the same 40 MHz samples, read as the resampled stream"""
    return np.ascontiguousarray(cap[::2]) if rate == 20 else cap


def _family_captures(oracle, rate):
    """[(family, index, capture)] of every family but many_frames, and the restatement's rows for them: computed once, left unchanged"""
    key = ("fam", rate)
    if key not in _memo:
        items = [(name, i, _at_rate(c, rate)) for name, caps in sc.families(oracle).items() if name != "many_frames" for i, c in enumerate(caps)]
        want = []
        for k, (_, _, c) in enumerate(items):
            for r in oracle.rx_capture(c, rate, max_frames=8):
                r = dict(r); r["capture_id"] = k; want.append(r)
        _memo[key] = (items, want)
    return _memo[key]


def _run(sora, caps, rate, front, max_frames):
    import torch
    iq, descs = batch(caps)
    rx = sora.Rx(len(caps), len(iq), sample_rate_mhz=rate, max_frames_per_capture=max_frames)
    if front:
        rx.set_front(front)
    t = rx.process_dev(torch.from_numpy(iq).cuda(), descs)
    got = rx.results(ticket=t)
    used_front = rx.call_front(t)
    rx.close()
    return got, used_front


def _first_difference(items, got, want):
    """-> a message naming the family and capture of the first row that differs"""
    for g, w in zip(got, want):
        ok, why = same_results([g], [w])
        if not ok:
            k = min(g["capture_id"], w["capture_id"])
            return "%s capture %d: %s" % (items[k][0], items[k][1], why)
    return "row count %d != %d" % (len(got), len(want))


@pytest.mark.parametrize("front", [0, 3])
@pytest.mark.parametrize("rate", RATES)
def test_rows_of_every_family(sora, oracle, rate, front):
    items, want = _family_captures(oracle, rate)
    assert len(items) > 4000 and len(want) > 3000
    got, used_front = _run(sora, [c for _, _, c in items], rate, front, 8)
    if front:
        assert used_front == front
    assert not any(r["flags"] for r in got)                                    # no capture holds more than eight events
    ok, _ = same_results(got, want)
    assert ok, "%d MHz, front %d: %s" % (rate, front, _first_difference(items, got, want))
    kinds = {r["error_code"] for r in got}
    assert {0x1, 0x80000005, 0x80000006} <= kinds


@pytest.mark.parametrize("front", [0, 3])
@pytest.mark.parametrize("rate", RATES)
def test_many_frames_in_one_call_with_small_captures(sora, oracle, rate, front):
    """16, 63, 64, 65 and 70 frames in a capture (k_scan queues a capture's decode jobs in its 64 lanes and hands them over when they are used up), in one
    call with small captures of other rates: every frame comes back E_FRAME_OK and equal to the restatement's."""
    small = [make_capture(oracle, kbps, n, seed=40 + i, rate_mhz=40, sigma=30, lead=100 + 30 * i)[0] for i, (kbps, n) in enumerate(((6000, 60), (36000, 90), (12000, 33), (9000, 70)))]
    caps = [_at_rate(c, rate) for c in small[:2] + sc.families(oracle)["many_frames"] + small[2:]]
    want = []
    for k, c in enumerate(caps):
        for r in oracle.rx_capture(c, rate, max_frames=80):
            r = dict(r); r["capture_id"] = k; want.append(r)
    per_capture = [sum(r["capture_id"] == k for r in want) for k in range(len(caps))]
    assert per_capture == [1, 1] + list(sc.MANY_FRAMES) + [1, 1]
    assert all(r["error_code"] == 1 for r in want)
    got, used_front = _run(sora, caps, rate, front, 80)
    if front:
        assert used_front == front
    assert [r["error_code"] for r in got] == [1] * len(want) and not any(r["flags"] for r in got)
    ok, why = same_results(got, want)
    assert ok, "%d MHz, front %d: %s" % (rate, front, why)
    assert {r["rate_kbps"] for r in got} == {6000, 9000, 12000, 24000, 36000, 48000, 54000}


# ---- the state records

def _trace(oracle, rate):
    """the composite stream at that rate, its resume points (20 MHz-rate positions), their records, and the restatement's rows of the whole stream"""
    key = ("trace", rate)
    if key not in _memo:
        x = _at_rate(sc.families(oracle)["composite_stream"][0], rate)
        p, r = oracle.cs_trace(x, rate)
        _memo[key] = (x, p.astype(np.int64), r, oracle.rx_capture(x, rate))
    return _memo[key]


def _open_stream(sora, ncaps, total, rate):
    rx = sora.Rx(ncaps, total, sample_rate_mhz=rate, max_frames_per_capture=8)
    assert rx.set_stream_mode(1) == 0
    return rx


def _rows_of(rows, k, shift=0):
    out = []
    for r in rows:
        if r["capture_id"] == k:
            r = dict(r); r["capture_id"] = 0; r["start_sample"] += shift; r["end_sample"] += shift; out.append(r)
    return out


def _rows_in_front(rows, pos20):
    out = []
    for r in rows:
        if r["end_sample"] <= pos20:
            r = dict(r); r["capture_id"] = 0; out.append(r)
    return out


@pytest.mark.parametrize("rate", RATES)
def test_state_record_at_the_last_resume_point_of_every_prefix(sora, oracle, rate):
    """Capture k of ONE call of a fresh stream-mode handle is the first k source bursts of the composite stream (56 raw samples at 40 MHz, 28 at 20 MHz; one
    resampler period of 280 in 44 MHz mode).  Per capture: stream_consumed is the restatement's last resume point in the prefix, the record is its state
    there, word for word, and the rows are the whole stream's events in front of that point."""
    import torch
    x, p, rec, rows = _trace(oracle, rate)
    per20 = 1 if rate == 20 else 2                                           # input samples per 20 MHz-rate sample
    step = {40: 56, 20: 28, 44: 280}[rate]
    K = len(x) // step
    assert K * step == len(x) and K == {40: 325, 20: 325, 44: 65}[rate]
    iq, descs = batch([x[:step * k] for k in range(1, K + 1)])
    rx = _open_stream(sora, K, len(iq), rate)
    t = rx.process_dev(torch.from_numpy(iq).cuda(), descs)
    got_rows = rx.results(ticket=t)
    used = rx.stream_consumed(t, K)
    points = set()
    for k in range(1, K + 1):
        i = int(np.searchsorted(p, step * k // per20, side="right")) - 1     # the last resume point at or in front of the prefix's end
        assert i >= 0
        points.add(i)
        assert int(used[k - 1]) == p[i] * per20, "prefix %d: consumed %d, the restatement's last resume point is %d" % (k, used[k - 1], p[i] * per20)
        got = rx.stream_record_of(t, k - 1)
        assert len(got) == 64 and got[41] == CS_RECORD_MAGIC and not got[43:].any()
        bad = np.nonzero(got != rec[i])[0]
        assert len(bad) == 0, "prefix %d (resume point %d): words %s are %s, the restatement has %s" % (k, p[i], bad.tolist(), got[bad].tolist(), rec[i][bad].tolist())
        ok, why = same_results(_rows_of(got_rows, k - 1), _rows_in_front(rows, p[i]))
        assert ok, "prefix %d: %s" % (k, why)
    rx.close()
    # the prefixes stop at many different points, some of them with the stale peak of a dropped lock in the record, some inside the DC step
    # (resume points are at least one prefix step apart: every one but the stream's start is some prefix's last)
    assert points == set(range(1, len(p))) and len(p) >= (45 if rate == 44 else 200)
    assert (rec[:, 33] != 0).sum() >= 2 and len(set(rec[:, 38].tolist())) >= 4 and len(set(rec[:, 42].tolist())) >= 3


@pytest.mark.parametrize("rate", RATES)
def test_state_record_at_the_end_of_every_family_capture(sora, oracle, rate):
    """The composite stream holds no true carrier test behind a raised time-out and one lock dropped on a DC update; the families hold them by the dozen
    (tests/test_scan_captures_cpu.py).  So every family capture also goes through a stream-mode handle, whole: its resume point, its record and its rows
    are the restatement's at the capture's last resume point.  What a rare branch does to the DC estimate or a window shows in the record even where no
    row moves."""
    import torch
    items, want = _family_captures(oracle, rate)
    key = ("last", rate)
    if key not in _memo:
        last = []
        for _, _, c in items:
            p, r = oracle.cs_trace(c, rate)
            last.append((int(p[-1]), r[-1].copy()))
        _memo[key] = last
    last = _memo[key]
    per20 = 1 if rate == 20 else 2
    iq, descs = batch([c for _, _, c in items])
    rx = _open_stream(sora, len(items), len(iq), rate)
    t = rx.process_dev(torch.from_numpy(iq).cuda(), descs)
    got_rows = rx.results(ticket=t)
    used = rx.stream_consumed(t, len(items))
    by_capture = {}
    for r in want:
        by_capture.setdefault(r["capture_id"], []).append(r)
    got_by_capture = {}
    for r in got_rows:
        got_by_capture.setdefault(r["capture_id"], []).append(r)
    for k, (name, i, _) in enumerate(items):
        pos, rec = last[k]
        assert int(used[k]) == pos * per20, "%s capture %d: consumed %d, the restatement's last resume point is %d" % (name, i, used[k], pos * per20)
        got = rx.stream_record_of(t, k)
        bad = np.nonzero(got != rec)[0]
        assert len(bad) == 0, "%s capture %d (resume point %d): words %s are %s, the restatement has %s" % (name, i, pos, bad.tolist(), got[bad].tolist(), rec[bad].tolist())
        ok, why = same_results(got_by_capture.get(k, []), [r for r in by_capture.get(k, []) if r["end_sample"] <= pos])
        assert ok, "%s capture %d: %s" % (name, i, why)
    rx.close()
    assert len({int(rec[38]) for _, rec in last}) >= 100                     # the captures end with many different DC estimates


@pytest.mark.parametrize("rate", RATES)
def test_a_continued_capture_ends_in_the_state_of_the_uncut_stream(sora, oracle, rate):
    """Forty pairs of cuts (c1, c2), one stream per pair: call 1 holds the stream up to c1, call 2 what call 1 left unconsumed, up to c2.  The record after
    call 2 is the uncut stream's state at the last resume point in front of c2 (its position and frame count relative to call 2's capture), and the rows
    of both calls are the uncut stream's events in front of that point."""
    import torch
    x, p, rec, rows = _trace(oracle, rate)
    per20 = 1 if rate == 20 else 2
    q = 14 if rate == 20 else 28                                             # captures are whole source calls
    n = len(x) // q
    rng = np.random.default_rng(20261109 + rate)
    pairs = []
    while len(pairs) < 40:
        a = int(rng.integers(1, n - 1))
        b = min(n, a + int(rng.integers(1, int(rng.choice([3, 12, 60, n])) + 1)))                # call 2 adds a little, or a lot
        pairs.append((a * q, b * q))
    np_ = len(pairs)
    iq1, d1 = batch([x[:c1] for c1, _ in pairs])
    rx = _open_stream(sora, np_, 2 * len(x) * np_, rate)
    t1 = rx.process_dev(torch.from_numpy(iq1).cuda(), d1)
    rows1 = rx.results(ticket=t1)
    used1 = [int(u) for u in rx.stream_consumed(t1, np_)]
    iq2, d2 = batch([x[u:c2] for u, (_, c2) in zip(used1, pairs)])
    t2 = rx.process_dev(torch.from_numpy(iq2).cuda(), d2)
    rows2 = rx.results(ticket=t2)
    used2 = [int(u) for u in rx.stream_consumed(t2, np_)]
    moved = 0
    for j, (c1, c2) in enumerate(pairs):
        i1 = int(np.searchsorted(p, c1 // per20, side="right")) - 1
        i2 = int(np.searchsorted(p, c2 // per20, side="right")) - 1
        assert used1[j] == p[i1] * per20, "pair %d (%d, %d): call 1 consumed %d, not %d" % (j, c1, c2, used1[j], p[i1] * per20)
        assert used1[j] + used2[j] == p[i2] * per20, "pair %d (%d, %d): call 2 consumed %d, not %d" % (j, c1, c2, used2[j], p[i2] * per20 - used1[j])
        want = rec[i2].copy()
        want[40] = p[i2] * per20 - used1[j]
        want[42] = rec[i2][42] - rec[i1][42]
        got = rx.stream_record_of(t2, j)
        bad = np.nonzero(got != want)[0]
        assert len(bad) == 0, "pair %d (%d, %d): words %s are %s, the uncut stream has %s" % (j, c1, c2, bad.tolist(), got[bad].tolist(), want[bad].tolist())
        both = _rows_of(rows1, j) + _rows_of(rows2, j, shift=used1[j] // per20)
        ok, why = same_results(both, _rows_in_front(rows, p[i2]))
        assert ok, "pair %d (%d, %d): %s" % (j, c1, c2, why)
        moved += i2 > i1
    rx.close()
    assert moved >= 20


def test_record_read_out_refuses_what_it_cannot_answer(sora, oracle):
    import torch
    x = sc.families(oracle)["composite_stream"][0][:56 * 20]
    d = torch.from_numpy(x).cuda()
    rx = sora.Rx(2, 2 * len(x), sample_rate_mhz=40, max_frames_per_capture=2)
    t = rx.process_dev(d, [(0, len(x), 0)])
    out = np.zeros(64, np.uint32); n = ctypes.c_size_t(7)
    L = rx._L
    assert L.sora_rx_stream_record_of(rx._h, t, 0, out.ctypes.data, 64, ctypes.byref(n)) == -1 and n.value == 0       # stream mode is off
    assert b"sora_rx_stream_record_of" in L.sora_hip_last_error()
    rx.set_stream_mode(1)
    t = rx.process_dev(d, [(0, len(x), 0)])
    assert L.sora_rx_stream_record_of(rx._h, t, 1, out.ctypes.data, 64, ctypes.byref(n)) == -1                        # the call had one capture
    assert L.sora_rx_stream_record_of(rx._h, t + 1, 0, out.ctypes.data, 64, ctypes.byref(n)) == -1                    # no such call
    assert L.sora_rx_stream_record_of(rx._h, t, 0, out.ctypes.data, 63, ctypes.byref(n)) == -6 and n.value == 64 and not out.any()
    assert L.sora_rx_stream_record_of(rx._h, t, 0, out.ctypes.data, 64, ctypes.byref(n)) == 0 and n.value == 64 and out[41] == CS_RECORD_MAGIC
    first = out.copy()
    assert np.array_equal(rx.stream_record_of(t, 0), first)                                                             # reading changes nothing
    pos, want = oracle.cs_trace(x, 40)
    assert int(rx.stream_consumed(t, 1)[0]) == first[40] == 2 * pos[-1] and np.array_equal(first, want[-1])
    rx.close()
