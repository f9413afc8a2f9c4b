"""Stream continuation of the 802.11b receive graph (sora_rx11b_set_stream_mode, include/sora_hip.h): 44 MHz streams handed to the library
in pieces cut at random source calls must yield exactly the events MAC11b_Receive reports on the UNCUT stream -- the live-source case,
where a Sora host binds CreateDemodGraph11b to TRxStream and the graph's DC estimate, energy detector, facades and output buffer carry
over from read to read.  The reference is the compiled reference graph where oracle/_ref is built (the GPU handle with stream mode off is
held to it as well); without it, the GPU modulator makes the frames and the mode-off handle over the uncut stream is the reference."""
import numpy as np
import pytest

from gpu_util import random_capture_11b, same_as_reference_11b

pytestmark = pytest.mark.gpu
QUIET = 28 * 120                      # low noise behind every stream: its last frame and the Seek behind it end inside the stream


@pytest.fixture(scope="module")
def sora():
    import sora_amd
    sora_amd.load()
    assert sora_amd.device_count() > 0
    return sora_amd


class _GpuModulator:
    """ReferenceGraph.tx11b's shape over sora_amd.tx11b (the GPU transmitter, bit-exact to the reference's modulator)"""

    def __init__(self, sora):
        self.sora = sora

    def tx11b(self, mpdu, rate_kbps):
        out, _ = self.sora.tx11b([bytes(mpdu)], [rate_kbps])
        return out.cpu().numpy()


@pytest.fixture(scope="module")
def graph(sora):
    from oracle.pyoracle import ReferenceGraph
    g = ReferenceGraph()
    return g if g.available() else None


def _modulator(sora, graph):
    return graph if graph is not None else _GpuModulator(sora)


def _quiet(rng, n=QUIET):
    return np.rint(rng.normal(0, 30, (n, 2))).astype(np.int16)


def _frames(mod, rng, spec, gap=(600, 3000)):
    """frames [(rate_kbps, mpdu_len)], back to back with random gaps, low noise"""
    parts = [_quiet(rng, 28 * 20)]
    for rate, ln in spec:
        s8 = mod.tx11b(rng.integers(0, 256, ln).astype(np.uint8).tobytes(), rate)
        x = np.zeros((len(s8) + int(rng.integers(*gap)), 2), np.int16)
        x[:len(s8)] = s8.astype(np.int16) << 8
        parts.append(x + _quiet(rng, len(x)))
    x = np.concatenate(parts + [_quiet(rng)])
    return np.ascontiguousarray(x[:len(x) // 28 * 28])


def _mode_off(sora, stream, max_frames=256):
    """the GPU handle, stream mode off, over the uncut stream as one capture: events in ReferenceGraph.rx11b's form"""
    import torch
    rx = sora.Rx11b(1, len(stream), max_frames_per_capture=max_frames)
    rx.process_dev(torch.from_numpy(stream).cuda(), [(0, len(stream), 0)])
    rows = rx.results(); rx.close()
    return [dict(r, sample_index=r["end_sample"]) for r in rows]


def _all_events(run):
    """run(max_frames) -> events; the cap grows until the events no longer fill it (bare noise can raise an event every few hundred samples)"""
    cap = 256
    while True:
        ev = run(cap)
        if len(ev) < cap:
            return ev
        cap *= 4


def _reference(sora, graph, stream):
    off = _all_events(lambda cap: _mode_off(sora, stream, cap))
    if graph is None:
        return off
    want = _all_events(lambda cap: graph.rx11b(stream, max_frames=cap))
    ok, why = same_as_reference_11b(off, want)
    assert ok, "stream mode off, uncut stream, against the reference graph: " + why
    return want


def _run_in_pieces(sora, streams, rng, step=(1, 3000), max_frames=32, plan=2, host_input=False, hold=None):
    """One capture per stream and call: from the stream's resume point to what has 'arrived' (grows by a random number of 28-sample
    source calls per call; the host tail grows while the stream does not move).  hold(call, k) -> True gives stream k a zero-length
    capture in that call.  -> absolute rows per stream, resume points per call, calls."""
    import torch
    ns = len(streams)
    rx = sora.Rx11b(ns, sum(len(s) for s in streams) + 28 * ns, max_frames_per_capture=max_frames)
    rx.set_single_pass(plan)
    assert rx.set_stream_mode(1) == 0 and rx.set_stream_mode(-1) == 1
    base, arrived, done = [0] * ns, [0] * ns, [False] * ns
    events = [[] for _ in range(ns)]
    history = []
    call = 0
    while not all(done):
        segs, descs, off, last = [], [], 0, [False] * ns
        for k, s in enumerate(streams):
            n = 0
            if not done[k] and not (hold and hold(call, k)):
                arrived[k] = min(len(s), max(arrived[k], base[k]) + 28 * int(rng.integers(*step)))
                n = (arrived[k] - base[k]) // 28 * 28
                last[k] = base[k] + n + 28 > len(s)                     # everything has arrived
            segs.append(s[base[k]:base[k] + n]); descs.append((off, n, k)); off += n
        iq = np.ascontiguousarray(np.concatenate(segs)) if off else np.zeros((28, 2), np.int16)
        if host_input and call % 2:
            rx.process(iq, descs); t = rx.ticket()
        else:
            t = rx.process_dev(torch.from_numpy(iq).cuda(), descs)
        rows = rx.results(ticket=t)
        used = rx.stream_consumed(t, ns)
        for r in rows:
            k = r["capture_id"]
            assert r["end_sample"] <= used[k], (r["end_sample"], used[k])   # every reported row lies in front of the resume point
            assert not r["flags"], r                                          # no row stands for lost events
            events[k].append(dict(r, end_sample=r["end_sample"] + base[k]))
        for k in range(ns):
            assert used[k] % 4 == 0 and used[k] <= descs[k][1], (used[k], descs[k])
            base[k] += int(used[k])
            # done once everything has arrived and a call no longer moves the stream (withheld rows move it on in later calls)
            done[k] = done[k] or (last[k] and (used[k] == 0 or len(streams[k]) - base[k] < 28))
        history.append((list(descs), [int(u) for u in used], rows))
        call += 1
        assert call < 2000
    rx.close()
    return events, history, base


def _check(got, want, final, what):
    assert all(e["sample_index"] <= final for e in want), (what, "an event lies behind the final resume point", final)
    ok, why = same_as_reference_11b(got, want)
    assert ok, what + ": " + why


@pytest.mark.parametrize("plan", [0, 1, 2])
def test_pieces_report_what_the_uncut_stream_reports(sora, graph, plan):
    """Streams of random captures (all four rates, gaps, DC / gain / carrier offsets, noise, truncated frames, bare noise), 1 to 9 per call,
    cut at random source calls: the rows of all calls equal the reference graph's events on each uncut stream, under every pass plan."""
    mod = _modulator(sora, graph)
    rng = np.random.default_rng(20261016 + plan)
    nev = 0; kinds = set(); rates = set()
    for trial in range(5):
        ns = [1, 3, 9, 5, 2][trial]
        streams = []
        for _ in range(ns):
            x = np.concatenate([random_capture_11b(mod, rng) for _ in range(int(rng.integers(2, 6)))] + [_quiet(rng)])
            streams.append(np.ascontiguousarray(x[:len(x) // 28 * 28]))
        want = [_reference(sora, graph, s) for s in streams]
        got, history, final = _run_in_pieces(sora, streams, rng, plan=plan)
        for k in range(ns):
            _check(got[k], want[k], final[k], "plan %d trial %d stream %d (%d calls)" % (plan, trial, k, len(history)))
            nev += len(want[k]); kinds.update(e["error_code"] for e in want[k]); rates.update(e["rate_kbps"] for e in want[k] if e["error_code"] == 1)
    assert nev > 40 and 0x1 in kinds and len(kinds) >= 3 and {1000, 2000, 5500, 11000} <= rates, (nev, kinds, rates)


def test_a_long_frame_straddling_many_pieces_is_reported_once(sora, graph):
    """A 1 Mbps frame of 300 bytes (about 110 k samples) fed 28 x 100 samples at a time: the resume point stays put while it runs, the host's
    tail grows, and the frame is reported once, when a piece finally holds its end and the Seek behind it."""
    mod = _modulator(sora, graph)
    rng = np.random.default_rng(11)
    stream = _frames(mod, rng, [(1000, 300)])
    want = _reference(sora, graph, stream)
    assert [e["error_code"] for e in want] == [1]
    got, history, final = _run_in_pieces(sora, [stream], rng, step=(100, 101))
    _check(got[0], want, final[0], "long frame")
    assert len(history) > 30
    # from the call whose capture reaches into the frame until the one that reports it, every resume point is the one in front of the frame
    start = next(i for i, (d, u, r) in enumerate(history) if u[0] < d[0][1])
    report = next(i for i, (d, u, r) in enumerate(history) if r)
    assert report - start > 25
    pos = [sum(h[1][0] for h in history[:i + 1]) for i in range(len(history))]
    assert len(set(pos[start:report])) == 1 and pos[start] < want[0]["sample_index"] - 100000


def test_a_short_frame_after_a_cut_reads_the_stale_bytes_of_the_long_one(sora, graph):
    """A long frame, a cut, then a shorter frame: the short frame's last MPDU byte and its FCS word's top byte are what the long frame left
    in the harness's output buffer -- one call earlier.  Without the buffer in the continuation record they come out as zeros."""
    mod = _modulator(sora, graph)
    rng = np.random.default_rng(5)
    stream = _frames(mod, rng, [(2000, 200), (11000, 30)], gap=(8000, 8001))
    want = _reference(sora, graph, stream)
    assert [e["error_code"] for e in want] == [1, 1] and want[1]["mpdu"][-1] != 0
    cut = (want[0]["sample_index"] + 352 + 28 * 20) // 28 * 28           # behind the first frame and its Seek, in front of the second
    assert cut < want[1]["sample_index"] - 12000
    import torch
    rx = sora.Rx11b(1, len(stream), max_frames_per_capture=4)
    rx.set_stream_mode(1)
    t = rx.process_dev(torch.from_numpy(stream[:cut].copy()).cuda(), [(0, cut, 0)])
    r1 = rx.results(ticket=t); u1 = int(rx.stream_consumed(t, 1)[0])
    assert len(r1) == 1 and r1[0]["end_sample"] <= u1
    rest = np.ascontiguousarray(stream[u1:u1 + (len(stream) - u1) // 28 * 28])
    t = rx.process_dev(torch.from_numpy(rest).cuda(), [(0, len(rest), 0)])
    r2 = rx.results(ticket=t)
    rx.close()
    got = r1 + [dict(r, end_sample=r["end_sample"] + u1) for r in r2]
    ok, why = same_as_reference_11b(got, want)
    assert ok, why
    assert r2[0]["mpdu"][-1] == want[1]["mpdu"][-1] != 0


@pytest.mark.parametrize("behind", [0, 28, 28 * 6])
def test_a_cut_inside_the_seek_withholds_the_row_until_the_next_call(sora, graph, behind):
    """The capture ends at the frame's event (behind = 0) or inside the 352-sample Seek behind it: the kernel clips that Seek, the uncut
    stream does not, so the row lies behind the resume point -- withheld, then reported once by the next call."""
    import torch
    mod = _modulator(sora, graph)
    rng = np.random.default_rng(3)
    stream = _frames(mod, rng, [(1000, 20), (1000, 14)])
    want = _reference(sora, graph, stream)
    assert [e["error_code"] for e in want] == [1, 1]
    e0 = want[0]["sample_index"]
    assert e0 % 28 == 0                                                  # the first frame's calls are aligned to the stream's start
    cut = e0 + behind
    rx = sora.Rx11b(1, len(stream), max_frames_per_capture=4)
    rx.set_stream_mode(1)
    t = rx.process_dev(torch.from_numpy(stream[:cut].copy()).cuda(), [(0, cut, 0)])
    r1 = rx.results(ticket=t); u1 = int(rx.stream_consumed(t, 1)[0])
    assert r1 == [] and u1 < e0 - 10000
    rest = np.ascontiguousarray(stream[u1:u1 + (len(stream) - u1) // 28 * 28])
    t = rx.process_dev(torch.from_numpy(rest).cuda(), [(0, len(rest), 0)])
    r2 = rx.results(ticket=t)
    rx.close()
    ok, why = same_as_reference_11b([dict(r, end_sample=r["end_sample"] + u1) for r in r2], want)
    assert ok, why


def test_no_event_is_lost_to_max_frames_per_capture(sora, graph):
    """Two row slots per capture, about five frames per piece: each call reports at most two rows and stops its resume point in front of the
    first event without a slot; over the calls every event is reported once."""
    mod = _modulator(sora, graph)
    rng = np.random.default_rng(2)
    spec = [(int(rng.choice([5500, 11000])), int(rng.choice([1, 14, 30]))) for _ in range(16)]
    streams = [_frames(mod, rng, spec, gap=(400, 900)) for _ in range(2)]
    want = [_reference(sora, graph, s) for s in streams]
    per_frame = np.mean([len(s) for s in streams]) / 16
    got, history, final = _run_in_pieces(sora, streams, rng, step=(int(5 * per_frame / 28), int(5 * per_frame / 28) + 1), max_frames=2)
    for k in range(2):
        _check(got[k], want[k], final[k], "stream %d" % k)
        assert sum(e["error_code"] == 1 for e in want[k]) >= 15
    per_call = [max(sum(r["capture_id"] == k for r in h[2]) for k in range(2)) for h in history]
    assert max(per_call) == 2 and len(history) >= 8, per_call


def test_zero_length_capture_host_input_and_api_errors(sora, graph):
    """A zero-length capture in the middle calls leaves its stream's record as it was (consumed 0); host input works in stream mode; the
    resume points exist for the most recent call only, for no more captures than it had, and not without stream mode."""
    import torch
    mod = _modulator(sora, graph)
    rng = np.random.default_rng(9)
    streams = [_frames(mod, rng, [(1000, 30), (2000, 60), (11000, 100)]) for _ in range(2)]
    want = [_reference(sora, graph, s) for s in streams]
    got, history, final = _run_in_pieces(sora, streams, rng, step=(200, 700), host_input=True, hold=lambda call, k: k == 0 and call in (2, 3))
    for k in range(2):
        _check(got[k], want[k], final[k], "stream %d" % k)
    assert history[2][0][0][1] == 0 and history[2][1][0] == 0 and history[3][1][0] == 0
    rx = sora.Rx11b(2, 28 * 64)
    assert rx.set_stream_mode(-1) == 0 and rx.set_stream_mode(-1) == 0
    iq = torch.zeros((28 * 8, 2), dtype=torch.int16, device="cuda")
    t = rx.process_dev(iq, [(0, 28 * 4, 0), (28 * 4, 28 * 4, 1)])
    with pytest.raises(sora.SoraError):
        rx.stream_consumed(t, 2)                                         # not in stream mode
    assert rx.set_stream_mode(1) == 0
    t1 = rx.process_dev(iq, [(0, 28 * 4, 0), (28 * 4, 28 * 4, 1)])
    assert list(rx.stream_consumed(t1, 2)) == [28 * 4, 28 * 4]
    t2 = rx.process_dev(iq, [(0, 28 * 8, 0)])
    with pytest.raises(sora.SoraError):
        rx.stream_consumed(t1, 1)                                        # a stale ticket
    with pytest.raises(sora.SoraError):
        rx.stream_consumed(t2, 2)                                        # more captures than the call had
    assert list(rx.stream_consumed(t2, 1)) == [28 * 8]
    assert rx.set_stream_mode(0) == 1 and rx.set_stream_mode(-1) == 0
    rx.close()
