"""Stream continuation of the 802.11n 2x2 receive graph (sora_rx11n_set_stream_mode, include/sora_hip.h): two-chain 40 MHz streams handed to
the library in pieces cut at random source calls must yield exactly the events RxThread reports on the UNCUT stream -- the live-source case,
where a Sora host binds CreateDemodGraph11n to TRxStream and the graph's carrier-sense state (MimoAutoCorr rings, running sums, delayed
energies, TCCA11n counters) carries over from read to read.  The reference is the compiled reference graph where oracle/_ref is built (the
GPU handle with stream mode off is held to it as well); without it, the GPU modulator makes the frames and the mode-off handle over the
uncut stream is the reference.  Every stream ends in a quiet tail, so the uncut stream's own end-of-capture flush raises nothing."""
import numpy as np
import pytest

from gpu_util import capture_11n, same_events_11n

pytestmark = pytest.mark.gpu
QUIET = 28 * 150                      # near-silent samples behind every stream


@pytest.fixture(scope="module")
def sora():
    import sora_amd
    sora_amd.load()
    assert sora_amd.device_count() > 0
    return sora_amd


class _GpuModulator:
    """ReferenceGraph.tx11n's shape over sora_amd.tx11n (the GPU transmitter, bit-exact to the reference's modulator)"""

    def __init__(self, sora):
        self.sora = sora

    def tx11n(self, mpdu, mcs):
        o0, o1, _ = self.sora.tx11n([bytes(mpdu)], [mcs])
        return o0.cpu().numpy(), o1.cpu().numpy()


@pytest.fixture(scope="module")
def graph(sora):
    from oracle.pyoracle import ReferenceGraph
    g = ReferenceGraph()
    return g if g.available() else None


def _modulator(sora, graph):
    return graph if graph is not None else _GpuModulator(sora)


def _quiet(rng, n=QUIET):
    return np.rint(rng.normal(0, 3, (n, 2))).astype(np.int16)


def _frame(mod, rng, mcs, ln):
    return mod.tx11n(rng.integers(0, 256, ln).astype(np.uint8).tobytes(), mcs)


def _stream(segments, rng):
    """two-chain stream from capture_11n segments, a quiet lead and a quiet tail; a whole number of 28-sample source calls"""
    a = np.concatenate([_quiet(rng, 28 * 10)] + [s[0] for s in segments] + [_quiet(rng)])
    b = np.concatenate([_quiet(rng, 28 * 10)] + [s[1] for s in segments] + [_quiet(rng)])
    n = len(a) // 28 * 28
    return np.ascontiguousarray(a[:n]), np.ascontiguousarray(b[:n])


def _random_stream(mod, rng, pool):
    """2-5 segments of 1-2 frames: MCS 8-10 (decoded), 11-14 (refused by the SIG parser), noise up to FCS failures, gain / phase /
    cross-talk / CFO, some multipath, now and then a frame cut short in the middle of the stream"""
    segs = []
    for _ in range(int(rng.integers(2, 6))):
        fr = [pool[int(i)] for i in rng.integers(0, len(pool), size=int(rng.integers(1, 3)))]
        sigma = float(rng.choice([3, 20, 60, 200, 600, 1500]))
        segs.append(capture_11n(rng, fr, sigma=sigma, cut=float(rng.uniform(0.1, 0.9)) if rng.random() < 0.15 else None, multipath_p=0.3))
    return _stream(segs, rng)


def _pool(mod, rng):
    out = []
    for k in range(14):
        mcs = [8, 9, 10, 8, 9, 10, 10, 11, 12, 13, 14, 8, 9, 10][k]
        ln = int(rng.integers(1, 700)) if k % 3 else int(rng.integers(1, 60))
        out.append(_frame(mod, rng, mcs, ln))
    return out


def _mode_off(sora, stream, max_frames=64):
    """the GPU handle, stream mode off, over the uncut stream as one capture: events in ReferenceGraph.rx11n's form"""
    import torch
    a, b = stream
    rx = sora.Rx11n(1, len(a), max_frames_per_capture=max_frames)
    rx.process_dev(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), [(0, len(a), 0)])
    rows = rx.results(); rx.close()
    return [dict(r, sample_index=r["end_sample"]) for r in rows]


def _all_events(run):
    """run(max_frames) -> events; the cap grows until the events no longer fill it"""
    cap = 64
    while True:
        ev = run(cap)
        if len(ev) < cap:
            return ev
        cap *= 4


def _reference(sora, graph, stream):
    off = _all_events(lambda cap: _mode_off(sora, stream, cap))
    if graph is None:
        return off
    want = _all_events(lambda cap: graph.rx11n(stream[0], stream[1], max_frames=cap))
    ok, why = same_events_11n(off, want, position="sample_index")
    assert ok, "stream mode off, uncut stream, against the reference graph: " + why
    return want


def _run_in_pieces(sora, streams, rng, step=(1, 200), max_frames=32, trellis=0, depth=1, host_input=False, hold=None):
    """One capture per stream and call: from the stream's resume point to what has 'arrived' (grows by a random number of 28-sample
    source calls per call; the host tail grows while the stream does not move).  hold(call, k) -> True gives stream k a zero-length
    capture in that call.  -> absolute rows per stream, (descriptors, resume points, rows) per call, final resume points."""
    import torch
    ns = len(streams)
    rx = sora.Rx11n(ns, sum(len(s[0]) for s in streams) + 28 * ns, max_frames_per_capture=max_frames)
    rx.set_trellis(trellis)
    rx.set_depth(depth)
    assert rx.set_stream_mode(1) == 0 and rx.set_stream_mode(-1) == 1
    base, arrived, done = [0] * ns, [0] * ns, [False] * ns
    events = [[] for _ in range(ns)]
    history = []
    call = 0
    while not all(done):
        s0, s1, descs, off, last = [], [], [], 0, [False] * ns
        for k, (a, b) in enumerate(streams):
            n = 0
            if not done[k] and not (hold and hold(call, k)):
                arrived[k] = min(len(a), max(arrived[k], base[k]) + 28 * int(rng.integers(*step)))
                n = (arrived[k] - base[k]) // 28 * 28
                last[k] = base[k] + n + 28 > len(a)                      # everything has arrived
            s0.append(a[base[k]:base[k] + n]); s1.append(b[base[k]:base[k] + n]); descs.append((off, n, k)); off += n
        if off:
            iq0, iq1 = np.ascontiguousarray(np.concatenate(s0)), np.ascontiguousarray(np.concatenate(s1))
        else:
            iq0 = iq1 = np.zeros((28, 2), np.int16)
        if host_input and call % 2:
            rx.process(iq0, iq1, descs); t = rx.ticket()
        else:
            t = rx.process_dev(torch.from_numpy(iq0).cuda(), torch.from_numpy(iq1).cuda(), descs)
        rows = rx.results(ticket=t)
        used = rx.stream_consumed(t, ns)
        for r in rows:
            k = r["capture_id"]
            assert r["end_sample"] <= used[k], (r["end_sample"], used[k])   # every reported row lies in front of the resume point
            assert not r["flags"], r                                          # no row stands for lost events
            events[k].append(dict(r, end_sample=r["end_sample"] + base[k]))
        for k in range(ns):
            assert used[k] % 28 == 0 and used[k] <= descs[k][1], (used[k], descs[k])
            base[k] += int(used[k])
            done[k] = done[k] or (last[k] and (used[k] == 0 or len(streams[k][0]) - base[k] < 28))
        history.append((list(descs), [int(u) for u in used], rows))
        call += 1
        assert call < 3000
    rx.close()
    return events, history, base


def _check(got, want, final, what):
    assert all(e["sample_index"] <= final for e in want), (what, "an event lies behind the final resume point", final)
    ok, why = same_events_11n(got, want, position="sample_index")
    assert ok, what + ": " + why


@pytest.fixture(scope="module")
def random_sets(sora, graph):
    """three sets of random streams (1, 4 and 9 streams) with the reference's events on each uncut stream"""
    mod = _modulator(sora, graph)
    rng = np.random.default_rng(20261016)
    pool = _pool(mod, rng)
    sets = []
    for ns in (1, 4, 9):
        streams = [_random_stream(mod, rng, pool) for _ in range(ns)]
        sets.append((streams, [_reference(sora, graph, s) for s in streams]))
    return sets


@pytest.mark.parametrize("depth", [1, 4])
@pytest.mark.parametrize("trellis", [0, 16, 64, 1])
def test_pieces_report_what_the_uncut_stream_reports(sora, random_sets, trellis, depth):
    """Random two-chain streams, 1 to 9 per call, cut at random source calls beyond each resume point: the rows of all calls equal the
    reference graph's events on each uncut stream, under every trellis choice (automatic, 16, 64, windowed) and at depth 1 and 4."""
    rng = np.random.default_rng(7 * trellis + depth)
    nev = 0; kinds = set(); mcs = set()
    for i, (streams, want) in enumerate(random_sets):
        got, history, final = _run_in_pieces(sora, streams, rng, step=(1, 120), trellis=trellis, depth=depth)
        for k in range(len(streams)):
            _check(got[k], want[k], final[k], "trellis %d depth %d set %d stream %d (%d calls)" % (trellis, depth, i, k, len(history)))
            nev += len(want[k]); kinds.update(e["error_code"] for e in want[k]); mcs.update(e["rate_kbps"] for e in want[k] if e["error_code"] == 1)
    assert nev > 30 and {0x1, 0x80000005, 0x80000006} <= kinds and {8, 9, 10} <= mcs, (nev, kinds, mcs)


def test_a_long_frame_straddling_many_pieces_is_reported_once(sora, graph):
    """A 1500-byte MCS 8 frame (1496 bytes and the FCS, the longest the SIG parser takes; about 37 k samples per chain) fed 28 x 20 samples at a time: the resume point stays put while it runs, the
    host's tail grows, and the frame is reported once, when a piece finally holds all of its symbols."""
    mod = _modulator(sora, graph)
    rng = np.random.default_rng(11)
    stream = _stream([capture_11n(rng, [_frame(mod, rng, 8, 1496)], sigma=20.0)], rng)
    want = _reference(sora, graph, stream)
    assert [e["error_code"] for e in want] == [1]
    got, history, final = _run_in_pieces(sora, [stream], rng, step=(20, 21))
    _check(got[0], want, final[0], "long frame")
    start = next(i for i, (d, u, r) in enumerate(history) if u[0] < d[0][1])
    report = next(i for i, (d, u, r) in enumerate(history) if r)
    assert report - start > 50, (start, report)
    pos = [sum(h[1][0] for h in history[:i + 1]) for i in range(len(history))]
    assert len(set(pos[start:report])) == 1 and pos[start] < want[0]["sample_index"] - 36000


def _one_frame(sora, graph, mcs, ln, seed):
    """a stream holding one frame at a known position: (stream, first sample of the frame, reference events)"""
    mod = _modulator(sora, graph)
    rng = np.random.default_rng(seed)
    s0, s1 = _frame(mod, rng, mcs, ln)
    lead = 28 * 40
    seg = (np.concatenate([np.zeros((lead, 2), np.int16), s0.astype(np.int16)]), np.concatenate([np.zeros((lead, 2), np.int16), s1.astype(np.int16)]))
    a, b = seg[0].copy(), seg[1].copy()
    a += np.rint(rng.normal(0, 20, a.shape)).astype(np.int16); b += np.rint(rng.normal(0, 20, b.shape)).astype(np.int16)
    stream = _stream([(a, b)], rng)
    f0 = 28 * 10 + lead
    return stream, f0, _reference(sora, graph, stream)


def _two_calls(sora, stream, cut):
    """stream mode: the stream up to `cut`, then the rest from the resume point -> (rows 1, resume point 1, rows 2 shifted to the stream)"""
    import torch
    a, b = stream
    rx = sora.Rx11n(1, len(a), max_frames_per_capture=4)
    rx.set_stream_mode(1)
    t = rx.process_dev(torch.from_numpy(a[:cut].copy()).cuda(), torch.from_numpy(b[:cut].copy()).cuda(), [(0, cut, 0)])
    r1 = rx.results(ticket=t); u1 = int(rx.stream_consumed(t, 1)[0])
    n = (len(a) - u1) // 28 * 28
    t = rx.process_dev(torch.from_numpy(a[u1:u1 + n].copy()).cuda(), torch.from_numpy(b[u1:u1 + n].copy()).cuda(), [(0, n, 0)])
    r2 = rx.results(ticket=t)
    rx.close()
    return r1, u1, [dict(r, end_sample=r["end_sample"] + u1) for r in r2]


# 40 MHz offsets from the frame's first sample: L-STF 0..320, L-LTF 320..640, L-SIG / HT-SIG1 / HT-SIG2 640..1120, HT-STF 1120..1280,
# HT-LTF 1280..1600, then the data symbols (160 each)
CUTS = {"plateau": 200, "l_ltf": 480, "l_sig": 720, "ht_sig1": 880, "ht_sig2": 1040, "ht_stf": 1200, "ht_ltf": 1440, "data": None,
        "last_burst": -56, "call_before_event": -28}


@pytest.mark.parametrize("where", sorted(CUTS))
def test_a_cut_inside_the_frame_withholds_it_until_the_next_call(sora, graph, where):
    """The first capture ends inside the detection plateau, the L-LTF, each SIG symbol, the HT-STF / HT-LTF, the data field, the last
    312-value Viterbi burst, or one call in front of the event: no row, a resume point in front of the frame's L-LTF (and of the cut), and
    the next call reports the frame once with the reference's fields."""
    stream, f0, want = _one_frame(sora, graph, 9, 400, 3)
    assert [e["error_code"] for e in want] == [1]
    e = want[0]["sample_index"]
    off = CUTS[where]
    cut = f0 + off if off is not None and off > 0 else (f0 + e) // 2 if off is None else e + off
    cut = cut // 28 * 28
    assert f0 < cut < e
    r1, u1, r2 = _two_calls(sora, stream, cut)
    assert r1 == [] and u1 <= min(cut, f0 + 400), (where, cut, u1)
    ok, why = same_events_11n(r2, want, position="sample_index")
    assert ok, (where, why)


def test_a_cut_at_the_event_reports_it_in_that_call(sora, graph):
    """The first capture ends exactly at the call boundary the event is reported at: all of the frame lies inside it, so the row comes with
    that call (no flush needed) and the resume point is the event's position; the rest of the stream adds nothing."""
    stream, f0, want = _one_frame(sora, graph, 10, 900, 4)
    assert [e["error_code"] for e in want] == [1]
    e = want[0]["sample_index"]
    r1, u1, r2 = _two_calls(sora, stream, e)
    assert u1 == e and r2 == []
    ok, why = same_events_11n(r1, want, position="sample_index")
    assert ok, why


def test_a_header_failure_cut_in_its_sig_field_is_withheld(sora, graph):
    """MCS 12: the SIG parser refuses the frame, an event at the end of the third SIG symbol.  Cut inside HT-SIG2, the capture does not
    hold that symbol: no zero-padded SIG decode, no event, until the next call."""
    stream, f0, want = _one_frame(sora, graph, 12, 100, 5)
    assert [e["error_code"] for e in want] == [0x80000005]
    cut = (f0 + 1040) // 28 * 28
    r1, u1, r2 = _two_calls(sora, stream, cut)
    assert r1 == [] and u1 <= f0 + 400
    ok, why = same_events_11n(r2, want, position="sample_index")
    assert ok, why


@pytest.mark.parametrize("max_frames", [1, 2])
def test_no_event_is_lost_to_max_frames_per_capture(sora, graph, max_frames):
    """One or two row slots per capture, several short frames per piece: each call reports at most max_frames rows and stops its resume point
    in front of the first event without a slot; over the calls every event is reported once."""
    mod = _modulator(sora, graph)
    rng = np.random.default_rng(2 + max_frames)
    pool = [_frame(mod, rng, int(rng.choice([8, 9, 10, 11])), int(rng.integers(1, 80))) for _ in range(6)]
    streams = [_stream([capture_11n(rng, [pool[int(i)] for i in rng.integers(0, 6, size=4)], sigma=20.0) for _ in range(3)], rng) for _ in range(2)]
    want = [_reference(sora, graph, s) for s in streams]
    per_frame = np.mean([len(s[0]) for s in streams]) / 12
    step = int(4 * per_frame / 28)
    got, history, final = _run_in_pieces(sora, streams, rng, step=(step, step + 1), max_frames=max_frames)
    for k in range(2):
        _check(got[k], want[k], final[k], "stream %d" % k)
        assert len(want[k]) >= 10
    per_call = [max(sum(r["capture_id"] == k for r in h[2]) for k in range(2)) for h in history]
    assert max(per_call) == max_frames, per_call


def test_zero_length_captures_host_input_mode_switch_and_api_errors(sora, graph, random_sets):
    """A zero-length capture between non-empty ones leaves its stream as it was (consumed 0); host-buffer process alternates with
    process_dev; switching the mode starts the streams afresh; the resume points exist for the most recent call only, for no more captures
    than it had, and not without stream mode."""
    import torch
    streams, want = random_sets[1]
    rng = np.random.default_rng(9)
    got, history, final = _run_in_pieces(sora, streams, rng, step=(20, 150), host_input=True, hold=lambda call, k: k == 0 and call in (2, 3, 5))
    for k in range(len(streams)):
        _check(got[k], want[k], final[k], "stream %d" % k)
    assert history[2][0][0][1] == 0 and history[2][1][0] == 0 and history[3][1][0] == 0 and history[5][1][0] == 0

    rx = sora.Rx11n(2, 28 * 64)
    assert rx.set_stream_mode(-1) == 0 and rx.set_stream_mode(-1) == 0
    z = torch.zeros((28 * 8, 2), dtype=torch.int16, device="cuda")
    t = rx.process_dev(z, z, [(0, 28 * 4, 0), (28 * 4, 28 * 4, 1)])
    with pytest.raises(sora.SoraError):
        rx.stream_consumed(t, 2)                                         # not in stream mode
    assert rx.set_stream_mode(1) == 0
    t1 = rx.process_dev(z, z, [(0, 28 * 4, 0), (28 * 4, 28 * 4, 1)])
    assert list(rx.stream_consumed(t1, 2)) == [28 * 4, 28 * 4]
    t2 = rx.process_dev(z, z, [(0, 28 * 8, 0)])
    with pytest.raises(sora.SoraError):
        rx.stream_consumed(t1, 1)                                        # a stale ticket
    with pytest.raises(sora.SoraError):
        rx.stream_consumed(t2, 2)                                        # more captures than the call had
    assert list(rx.stream_consumed(t2, 1)) == [28 * 8]
    assert rx.set_stream_mode(0) == 1 and rx.set_stream_mode(-1) == 0
    rx.close()

    # a switch restarts the stream: the tail of a frame cut in the previous call is then a stream of its own (mode on -> on again)
    stream, f0, one = _one_frame(sora, graph, 9, 400, 3)
    a, b = stream
    cut = (f0 + 1440) // 28 * 28
    rx = sora.Rx11n(1, len(a), max_frames_per_capture=4)
    rx.set_stream_mode(1)
    t = rx.process_dev(torch.from_numpy(a[:cut].copy()).cuda(), torch.from_numpy(b[:cut].copy()).cuda(), [(0, cut, 0)])
    u1 = int(rx.stream_consumed(t, 1)[0])
    assert rx.results(ticket=t) == [] and u1 < f0 + 400
    assert rx.set_stream_mode(1) == 1                                   # starts every stream afresh
    n = (len(a) - cut) // 28 * 28
    t = rx.process_dev(torch.from_numpy(a[cut:cut + n].copy()).cuda(), torch.from_numpy(b[cut:cut + n].copy()).cuda(), [(0, n, 0)])
    fresh = rx.results(ticket=t)
    rx.close()
    ref = _mode_off(sora, (np.ascontiguousarray(a[cut:cut + n]), np.ascontiguousarray(b[cut:cut + n])))
    ok, why = same_events_11n(fresh, ref, position="sample_index")
    assert ok, why
