"""Stream continuation of the 40 MHz HT receive handle (sora_ht40_set_stream_mode, include/sora_hip.h): two-chain 40 MHz streams handed to
sora_ht40_process_captures_dev in pieces cut at random source calls must yield exactly the rows the handle reports, with the mode off, on the
UNCUT stream.  HT40 parity is unpinned, so the yardsticks are that mode-off handle (one capture per stream) and the PSDUs that were sent
(oracle/py_ht40.py makes the frames).  Every stream ends in more than 800 samples of noise only, so that the mode-off kernel's end-of-capture
padding plays no part in the yardstick."""
import numpy as np
import pytest

from oracle import py_ht40 as m

pytestmark = pytest.mark.gpu

FRAME_OK, PLCP_FAIL = 0x1, 0x80000005
TAIL = 28 * 32                        # noise-only samples behind the last frame of a stream (896)
KEY = ("error_code", "rate_kbps", "stream", "length", "crc32", "end_sample", "mpdu")


@pytest.fixture(scope="module")
def env():
    import torch
    import sora_amd
    sora_amd.load()
    assert sora_amd.device_count() > 0
    return torch, sora_amd


def _stream(rng, frames, sigma=8.0, cfo=0.0):
    """frames: [(mcs, length, spoil)] -> (iq [2, n, 2] int16 with n a whole number of 28-sample source calls, truth [(mcs, psdus, spoil, first sample)]).
    As tests/test_gpu_ht40.py::_raw_captures builds a capture: per frame a lead of 300-900 samples, a 2x2 channel with cross-talk, then noise over all."""
    segs, truth, pos = [], [], 0
    for mcs, ln, spoil in frames:
        ps = [m.add_fcs(rng.integers(0, 256, ln - 4, dtype=np.uint8).tobytes()) for _ in range(2)]
        x, nsym, pre = m.tx_frame(ps, mcs)
        if spoil == "sig":                                               # garbage where L-SIG / HT-SIG should be: the header must fail
            x[:, 640:1120] = x[:, 640:1120][:, ::-1] * 1j
        ph = rng.uniform(0, 2 * np.pi, 4)
        H = np.array([[1.0 * np.exp(1j * ph[0]), 0.3 * np.exp(1j * ph[1])], [0.25 * np.exp(1j * ph[2]), 0.9 * np.exp(1j * ph[3])]])
        lead = int(rng.integers(300, 900))
        y = m.channel(x, H, 0.0, rng, cfo_step=cfo, lead=lead)
        segs.append(y); truth.append((mcs, ps, spoil, pos + lead)); pos += y.shape[1]
    y = np.concatenate(segs + [np.zeros((2, TAIL + 27, 2), np.int16)], axis=1).astype(np.float64)
    y += rng.normal(0, sigma, y.shape)
    y = np.clip(np.rint(y), -32768, 32767).astype(np.int16)
    n = y.shape[1] // 28 * 28
    return np.ascontiguousarray(y[:, :n]), truth


def _key(r):
    return tuple(r[f] for f in KEY)


def _mode_off(env, streams, max_frames=8, rx=None):
    """the yardstick: the handle with stream mode off, one capture per uncut stream -> rows per stream"""
    torch, sora = env
    own = rx is None
    if own:
        rx = sora.RxHt40(64, 1 << 22)
    iq = np.concatenate(streams, axis=1)
    descs, pos = [], 0
    for k, s in enumerate(streams):
        descs.append((pos, s.shape[1], k)); pos += s.shape[1]
    t = rx.process_captures_dev(torch.from_numpy(iq[0].copy()).cuda(), torch.from_numpy(iq[1].copy()).cuda(), descs, max_frames_per_capture=max_frames)
    rows = rx.results(ticket=t)
    if own:
        rx.close()
    per = [[] for _ in streams]
    for r in rows:
        assert not r["flags"], r
        per[r["capture_id"]].append(r)
    return per


def _check_yardstick(rows, truth, n):
    """on the yardstick's own rows: every frame that was sent with a sound header is decoded (two FRAME_OK rows, the PSDUs that were sent), every spoiled
    header is a PLCP row, nothing else is reported as a frame, and the last row lies at least 400 samples in front of the stream's end"""
    ok = [r for r in rows if r["error_code"] == FRAME_OK]
    want = [(mcs, s, ps[s]) for mcs, ps, spoil, _ in truth if not spoil for s in range(2)]
    assert [(r["rate_kbps"], r["stream"], r["mpdu"]) for r in ok] == want, [(hex(r["error_code"]), r["rate_kbps"], r["stream"], r["length"]) for r in rows]
    assert all(r["error_code"] in (FRAME_OK, PLCP_FAIL) for r in rows), [hex(r["error_code"]) for r in rows]
    assert sum(r["error_code"] == PLCP_FAIL for r in rows) >= sum(1 for t in truth if t[2])
    ends = [r["end_sample"] for r in rows]
    assert ends == sorted(ends) and ends[-1] + 400 <= n, (ends, n)


def _cuts(rng, n, pieces):
    """`pieces` arrival points of a stream of n samples: random multiples of 28, the last one its end"""
    inner = rng.choice(np.arange(1, n // 28), size=pieces - 1, replace=False)
    return sorted(int(c) * 28 for c in inner) + [n]


def _run_in_pieces(env, streams, arrivals, rng, per_call=(1, 3), max_frames=8, trellis=None):
    """Stream mode.  arrivals[k]: the sample counts of stream k that have 'arrived' at its successive turns.  Each call takes one to three streams that
    still have a turn left and gives every other stream a zero-length capture; capture k runs from stream k's resume point to its arrival point.
    -> (rows per stream with end_sample shifted to the stream, final resume points, [(descs, resume points, rows)] per call)."""
    torch, sora = env
    ns = len(streams)
    rx = sora.RxHt40(64, 1 << 22)
    if trellis is not None:
        rx.set_trellis(trellis)
    assert rx.set_stream_mode(1) == 0 and rx.set_stream_mode(-1) == 1
    base, turn = [0] * ns, [0] * ns
    got = [[] for _ in range(ns)]
    history = []
    while any(turn[k] < len(arrivals[k]) for k in range(ns)):
        left = [k for k in range(ns) if turn[k] < len(arrivals[k])]
        active = set(int(k) for k in rng.choice(left, size=min(len(left), int(rng.integers(per_call[0], per_call[1] + 1))), replace=False))
        parts, descs, off = [], [], 0
        for k in range(ns):
            n = 0
            if k in active:
                n = arrivals[k][turn[k]] - base[k]; turn[k] += 1
                assert n > 0 and n % 28 == 0
                parts.append(streams[k][:, base[k]:base[k] + n])
            descs.append((off, n, k)); off += n
        iq = np.concatenate(parts, axis=1)
        t = rx.process_captures_dev(torch.from_numpy(iq[0].copy()).cuda(), torch.from_numpy(iq[1].copy()).cuda(), descs, max_frames_per_capture=max_frames)
        rows = rx.results(ticket=t)
        used = [int(u) for u in rx.stream_consumed(t, ns)]
        for r in rows:
            k = r["capture_id"]
            assert r["end_sample"] <= used[k], (r["end_sample"], used[k])   # every reported row lies in front of the resume point
            assert not r["flags"], r                                          # no row stands for lost events
            got[k].append(dict(r, end_sample=r["end_sample"] + base[k]))
        for k in range(ns):
            assert used[k] % 28 == 0 and used[k] <= descs[k][1], (k, used[k], descs[k])
            base[k] += used[k]
        history.append((descs, used, rows))
        assert len(history) < 2000
    rx.close()
    return got, base, history


def _same(got, want, final, what):
    assert [_key(r) for r in got] == [_key(r) for r in want], (what, [(hex(r["error_code"]), r["rate_kbps"], r["stream"], r["end_sample"]) for r in got],
                                                                [(hex(r["error_code"]), r["rate_kbps"], r["stream"], r["end_sample"]) for r in want])
    assert not want or final >= want[-1]["end_sample"], (what, "the final resume point lies in front of the last row", final)


@pytest.fixture(scope="module")
def cut_set(env):
    """eight streams of three to six frames (MCS 8-14, 40-600 bytes, a carrier offset on every other one, one spoiled SIG field each) with the
    yardstick's rows on each uncut stream: computed once, shared, left unchanged"""
    rng = np.random.default_rng(20261018)
    streams, truths = [], []
    for k in range(8):
        nf = int(rng.integers(3, 7))
        frames = [(8 + int(rng.integers(0, 7)), int(rng.integers(40, 601)), None) for _ in range(nf)]
        sp = int(rng.integers(0, nf))
        frames[sp] = (frames[sp][0], frames[sp][1], "sig")
        s, tr = _stream(rng, frames, sigma=8.0, cfo=21.0 if k % 2 else 0.0)
        streams.append(s); truths.append(tr)
    want = _mode_off(env, streams)
    for k in range(8):
        _check_yardstick(want[k], truths[k], streams[k].shape[1])
    assert {r["rate_kbps"] for w in want for r in w if r["error_code"] == FRAME_OK} == set(range(8, 15))
    return streams, truths, want


def test_cut_streams_equal_the_uncut_stream(env, cut_set):
    """Eight streams, each cut at random multiples of 28 samples into 3-12 pieces, one to three streams per call: the rows of all calls, shifted by
    each capture's place in its stream, are the mode-off handle's rows on the uncut stream, exactly and in order (error code, MCS, spatial stream,
    length, FCS, position, MPDU bytes); every FRAME_OK row carries the PSDU that was sent; every row lies in front of its call's resume point."""
    streams, truths, want = cut_set
    rng = np.random.default_rng(1)
    arrivals = [_cuts(rng, s.shape[1], int(rng.integers(3, 13))) for s in streams]
    got, final, history = _run_in_pieces(env, streams, arrivals, rng)
    assert len(history) >= 12
    for k in range(len(streams)):
        _same(got[k], want[k], final[k], "stream %d" % k)
        sent = [ps[s] for _, ps, spoil, _ in truths[k] if not spoil for s in range(2)]
        assert [r["mpdu"] for r in got[k] if r["error_code"] == FRAME_OK] == sent, k
    # some frame did straddle two calls (its call's resume point stood in front of it)
    assert any(u < d[1] - 28 * 40 for descs, used, _ in history for d, u in zip(descs, used) if d[1])


def test_a_frame_longer_than_many_pieces_is_reported_once(env):
    """One 1500-byte MCS 8 frame (223 data symbols, about 37 k samples) fed 2800 samples at a time: while it runs the resume point stays in front of
    its detection and the host's tail grows; it is reported once, when a piece finally holds all of its symbols, with both PSDUs right."""
    rng = np.random.default_rng(2)
    s, truth = _stream(rng, [(8, 1500, None)])
    want = _mode_off(env, [s])[0]
    _check_yardstick(want, truth, s.shape[1])
    assert [r["error_code"] for r in want] == [FRAME_OK, FRAME_OK] and m.nsym_for([1500, 1500], *m.MCS2[8]) == 223
    n = s.shape[1]
    arrivals = [list(range(2800, n, 2800)) + [n]]
    got, final, history = _run_in_pieces(env, [s], arrivals, rng, per_call=(1, 1))
    _same(got[0], want, final[0], "long frame")
    assert [r["mpdu"] for r in got[0]] == truth[0][1]
    f0 = truth[0][3]
    pos = np.cumsum([h[1][0] for h in history])                           # the stream's resume point after each call
    report = next(i for i, h in enumerate(history) if h[2])
    start = next(i for i, (d, u, r) in enumerate(history) if u[0] < d[0][1] - 28)
    assert report - start >= 10, (start, report)
    # (the detection lies in front of the L-LTF's end, 640 samples into the frame)
    assert len(set(pos[start:report])) == 1 and pos[start] <= f0 + 640, (pos, f0)
    assert sum(bool(h[2]) for h in history) == 1


def test_no_event_is_lost_to_max_frames_per_capture(env):
    """Five short frames in one piece and two row slots per capture: each call reports two events at most and stops its resume point in front of the
    first event that found no slot; over three calls all five frames come out, once each."""
    rng = np.random.default_rng(3)
    s, truth = _stream(rng, [(8 + k, 60 + 10 * k, None) for k in range(5)])
    want = _mode_off(env, [s])[0]
    _check_yardstick(want, truth, s.shape[1])
    assert len(want) == 10
    n = s.shape[1]
    got, final, history = _run_in_pieces(env, [s], [[n, n, n]], rng, per_call=(1, 1), max_frames=2)
    _same(got[0], want, final[0], "row slots")
    assert [len(h[2]) for h in history] == [4, 4, 2]
    pos = np.cumsum([h[1][0] for h in history])
    for call, third in ((0, 2), (1, 4)):
        # behind the last event that found a slot, in front of the detection (hence of the L-LTF's end) of the first one that found none
        assert got[0][2 * third - 1]["end_sample"] <= pos[call] <= truth[third][3] + 640, (call, pos, truth[third][3])


def test_back_to_back_calls_are_serialised_and_collected_by_ticket(env, cut_set):
    """Eight stream-mode calls issued without a wait in between (the library runs them one after the other: each needs the records its predecessor
    leaves), call j bringing all of stream j as capture j and nothing for the other streams; each call is collected by its own ticket afterwards and
    holds the yardstick's rows of its stream.  The resume points exist for the last call only."""
    torch, sora = env
    streams, truths, want = cut_set
    ns = len(streams)
    rx = sora.RxHt40(64, 1 << 22)
    assert rx.calls_in_flight() >= ns
    rx.set_stream_mode(1)
    dev = [(torch.from_numpy(s[0].copy()).cuda(), torch.from_numpy(s[1].copy()).cuda()) for s in streams]
    tickets = []
    for j in range(ns):
        descs = [(0, streams[j].shape[1] if k == j else 0, k) for k in range(ns)]
        tickets.append(rx.process_captures_dev(dev[j][0], dev[j][1], descs, max_frames_per_capture=8))
    used = rx.stream_consumed(tickets[-1], ns)
    assert list(used[:-1]) == [0] * (ns - 1) and used[-1] % 28 == 0 and want[-1][-1]["end_sample"] <= used[-1] <= streams[-1].shape[1]
    with pytest.raises(sora.SoraError):
        rx.stream_consumed(tickets[0], ns)
    for j, t in enumerate(tickets):
        rows = rx.results(ticket=t)
        assert all(r["capture_id"] == j for r in rows)
        assert [_key(r) for r in rows] == [_key(r) for r in want[j]], j
    rx.close()


def test_the_modes_edges(env, cut_set):
    """A zero-length capture leaves its stream as it was; switching the mode off and on restarts the streams; a handle switched on and off again reports
    what it reported before; the resume points exist only in stream mode, for the latest ticket and for no more captures than its call had; a
    stream-mode call takes at most max_frames captures."""
    torch, sora = env
    streams, truths, want = cut_set
    s, tr = streams[0], truths[0]
    n = s.shape[1]
    a, b = torch.from_numpy(s[0].copy()).cuda(), torch.from_numpy(s[1].copy()).cuda()
    z = torch.zeros((28 * 9, 2), dtype=torch.int16, device="cuda")
    # a cut inside the data field of the first frame with a sound header
    f = next(t for t in tr if not t[2])
    cut = (f[3] + 1600 + 80) // 28 * 28                                  # (HT-LTF 2 ends 1600 samples into the frame: the middle of data symbol 0)

    rx = sora.RxHt40(8, 1 << 22)
    before = _mode_off(env, [s], rx=rx)[0]
    assert [_key(r) for r in before] == [_key(r) for r in want[0]]
    t = rx.process_captures_dev(a, b, [(0, n, 0)], max_frames_per_capture=8)
    with pytest.raises(sora.SoraError):
        rx.stream_consumed(t, 1)                                         # not in stream mode
    assert rx.set_stream_mode(-1) == 0 and rx.set_stream_mode(1) == 0 and rx.set_stream_mode(-1) == 1

    # ---- zero-length capture between two pieces
    t1 = rx.process_captures_dev(a, b, [(0, cut, 0)], max_frames_per_capture=8)
    r1 = rx.results(ticket=t1); u1 = int(rx.stream_consumed(t1, 1)[0])
    assert u1 % 28 == 0 and u1 <= f[3] + 640 and all(r["end_sample"] <= u1 for r in r1)
    t2 = rx.process_captures_dev(z, z, [(0, 0, 0)], max_frames_per_capture=8)
    assert rx.results(ticket=t2) == [] and list(rx.stream_consumed(t2, 1)) == [0]
    with pytest.raises(sora.SoraError):
        rx.stream_consumed(t1, 1)                                        # a stale ticket
    with pytest.raises(sora.SoraError):
        rx.stream_consumed(t2, 2)                                        # more captures than the call had
    t3 = rx.process_captures_dev(a[u1:], b[u1:], [(0, n - u1, 0)], max_frames_per_capture=8)
    r3 = [dict(r, end_sample=r["end_sample"] + u1) for r in rx.results(ticket=t3)]
    assert [_key(r) for r in r1 + r3] == [_key(r) for r in want[0]]

    # ---- a stream-mode call with more captures than max_frames is refused before anything runs
    t_before = rx.ticket()
    with pytest.raises(sora.SoraError) as e:
        rx.process_captures_dev(z, z, [(28 * k, 28, k) for k in range(9)], max_frames_per_capture=8)
    assert e.value.code == -1 and rx.ticket() == t_before               # SORA_ERR_INVALID_PARAM

    # ---- off and on: the streams start afresh, so the frame cut before the switch is not found from its second half
    assert rx.set_stream_mode(1) == 1
    t4 = rx.process_captures_dev(a, b, [(0, cut, 0)], max_frames_per_capture=8)
    r4 = rx.results(ticket=t4); u4 = int(rx.stream_consumed(t4, 1)[0])
    assert [_key(r) for r in r4] == [_key(r) for r in r1] and u4 == u1
    assert rx.set_stream_mode(0) == 1 and rx.set_stream_mode(1) == 0
    t5 = rx.process_captures_dev(a[cut:], b[cut:], [(0, n - cut, 0)], max_frames_per_capture=8)
    r5 = [dict(r, end_sample=r["end_sample"] + cut) for r in rx.results(ticket=t5)]
    cut_frame = [r for r in want[0] if r["error_code"] == FRAME_OK][:2]
    assert all(r["mpdu"] == p for r, p in zip(cut_frame, f[1]))
    assert not any(r["error_code"] == FRAME_OK and r["mpdu"] in f[1] for r in r5)
    # ... while the frames behind it are found as ever
    later = [_key(r) for r in want[0] if r["end_sample"] > cut_frame[-1]["end_sample"] and r["error_code"] == FRAME_OK]
    found = [_key(r) for r in r5 if r["error_code"] == FRAME_OK]
    assert found and all(k in later for k in found)

    # ---- on and then off: a mode-off call gives the rows it gave before
    assert rx.set_stream_mode(0) == 1 and rx.set_stream_mode(-1) == 0
    after = _mode_off(env, [s], rx=rx)[0]
    assert [_key(r) for r in after] == [_key(r) for r in before]
    rx.close()


def test_both_trellis_choices_give_the_same_rows(env, cut_set):
    """set_trellis(16) and set_trellis(64) on one stream cut the same way: identical rows, and the yardstick's."""
    streams, truths, want = cut_set
    k = max(range(len(streams)), key=lambda i: len(want[i]))
    out = {}
    for lanes in (16, 64):
        rng = np.random.default_rng(6)
        arrivals = [_cuts(rng, streams[k].shape[1], 7)]
        got, final, history = _run_in_pieces(env, [streams[k]], arrivals, rng, per_call=(1, 1), trellis=lanes)
        _same(got[0], want[k], final[0], "trellis %d" % lanes)
        out[lanes] = [_key(r) for r in got[0]]
    assert out[16] == out[64]
