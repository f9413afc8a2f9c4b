"""The receive handles at full-scale, DC-shifted and near-silent levels: every capture of tests/level_captures.py through the C ABI, every row against the
events the compiled reference graphs reported for it (tests/golden/refgraph_levels.npz).  What distinguishes a faithful port from a nearly faithful one --
saturating against wrapping arithmetic in k_scan's DC removal, energies, correlators and divisions, in the 802.11b scan and in the 802.11n carrier sense --
only shows at these levels, and those front ends have no stage entry point: whole captures are the only way in.  The live graphs, where oracle/_ref is
built, are a second check only; nothing here needs them."""
import numpy as np
import pytest

import level_captures as lc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sora():
    import sora_amd
    sora_amd.load()
    assert sora_amd.device_count() > 0
    return sora_amd


_SETS = {}


def _set(chain, oracle):
    """(captures, recorded reference events) of a chain, built once"""
    if chain not in _SETS:
        caps = lc.chain(chain, oracle)
        _SETS[chain] = (caps, lc.recorded(chain, caps))
    return _SETS[chain]


def _per_capture(rows, n):
    per = [[] for _ in range(n)]
    for r in rows:
        per[r["capture_id"]].append(r)
    return per


def _check(chain, caps, per, want, what):
    """rows per capture against the recorded events: every capture compared, all differences counted, the first shown"""
    bad = []
    for c, rows, w in zip(caps, per, want):
        assert not any(r["flags"] for r in rows), (what, c.name, "a row stands for lost events")
        got = lc.row_events(chain, rows)
        if got != w:
            bad.append("%s: got %r, reference %r" % (c.name, got, w))
    assert not bad, "%s: %d of %d captures differ; first: %s" % (what, len(bad), len(caps), bad[0])


def _live_second_check(chain, caps, want):
    from oracle.pyoracle import ReferenceGraph
    g = ReferenceGraph()
    if g.available():
        for c, w in zip(caps, want):
            assert lc.run_reference(g, chain, c) == w, (chain, c.name, "the recorded events are not what oracle/_ref reports now")


# ------------------------------------------------------------------ 802.11a: sora_rx
def _run_rx(sora, iqs, mhz, front=None, trellis=None, max_frames=lc.MAX_EVENTS["11a"]):
    import torch
    from gpu_util import batch
    iq, descs = batch(iqs)
    rx = sora.Rx(len(iqs), len(iq), sample_rate_mhz=mhz, max_frames_per_capture=max_frames)
    if front is not None:
        rx.set_front(front)
    if trellis is not None:
        rx.set_trellis(trellis)
    t = rx.process_dev(torch.from_numpy(iq).cuda(), descs)
    rows, used = rx.results(ticket=t), (rx.call_front(t), rx.trellis())
    rx.close()
    return _per_capture(rows, len(iqs)), used


@pytest.mark.parametrize("front,trellis", [(0, None), (3, None), (1, None), (None, 64), (None, 16), (None, 1)])
def test_rx_at_40_mhz(sora, oracle, front, trellis):
    """every front-end form that takes a whole batch (0: the library's choice, 3: k_sym_front -> k_track_lds -> k_sym_back, 1: k_frame) and every trellis
    (64, 16, 1: window-parallel)"""
    caps, want = _set("11a", oracle)
    per, used = _run_rx(sora, [c.iq for c in caps], 40, front, trellis)
    assert front in (None, 0) or used[0] == front
    assert trellis is None or used[1] == trellis
    _check("11a", caps, per, want, "front %s trellis %s" % (front, trellis))
    if front == 0:
        _live_second_check("11a", caps, want)


def _one_by_one_through_k_pipe(sora, caps, todo):
    """-> the rows of the captures of `todo` that a k_pipe launch decoded on its own, and the captures it did not: those whose call ran as another form, or
    whose data field the finishing kernel made again with k_frame's code because a wait inside the launch gave up (sora_rx_pipe_stats counts them).  After
    such a call the handle keeps to the three-kernel chain for its next 64 calls, so the captures after it go to a fresh handle."""
    import torch
    rows, left, rx = {}, [], None
    for i in todo:
        if rx is None:
            rx = sora.Rx(1, max(len(c.iq) for c in caps), sample_rate_mhz=40, max_frames_per_capture=lc.MAX_EVENTS["11a"])
            rx.set_depth(1); rx.set_front(4)
            assert rx.front() == 4
        t = rx.process_dev(torch.from_numpy(caps[i].iq).cuda(), [(0, len(caps[i].iq), 0)])
        r = rx.results(ticket=t)
        if rx.call_front(t) == 4 and rx.pipe_stats() == {"calls_made_again": 0, "backoffs": 0}:
            rows[i] = r
        else:
            left.append(i); rx.close(); rx = None
    if rx is not None:
        rx.close()
    return rows, left


def test_rx_at_40_mhz_through_k_pipe(sora, oracle):
    """front 4 -- the symbol chain and the window-parallel trellis as one launch -- takes what fits the chip at once (every workgroup of every call in flight
    resident together): one capture per call, one call in flight.  Every capture must have been decoded by k_pipe alone: a call that was made again, or that
    ran as another form, gets one more turn on a fresh handle, and whatever is left after that fails the test."""
    caps, want = _set("11a", oracle)
    rows, again = _one_by_one_through_k_pipe(sora, caps, range(len(caps)))
    more, left = _one_by_one_through_k_pipe(sora, caps, again)
    print("k_pipe: %d of %d captures decoded by the launch alone at once, %d at the second turn" % (len(rows), len(caps), len(more)))
    assert not left, ("%d of %d captures never went through a k_pipe launch alone in two turns (first: %s): a wait inside the launch gave up both times, "
                      "which is interference from other work on the chip and no statement about the rows" % (len(left), len(caps), caps[left[0]].name))
    rows.update(more)
    assert sorted(rows) == list(range(len(caps)))
    _check("11a", caps, [rows[i] for i in range(len(caps))], want, "front 4")


def test_rx_at_20_mhz_equals_the_oracle(sora, oracle):
    """the 20 MHz entry (every second sample) has no compiled reference graph: the restatement, which equals the graph on these captures at 40 MHz, is its reference"""
    from gpu_util import oracle_results, same_results
    caps, _ = _set("11a", oracle)
    iqs = [np.ascontiguousarray(c.iq[::2]) for c in caps]
    per, _ = _run_rx(sora, iqs, 20)
    want = _per_capture(oracle_results(oracle, iqs, 20), len(iqs))
    nev = 0
    for c, g, w in zip(caps, per, want):
        assert len(w) < lc.MAX_EVENTS["11a"]
        ok, why = same_results(g, w)
        assert ok, (c.name, why)
        nev += len(w)
    assert nev > 150, nev


def test_rx_behind_the_44_mhz_ingest(sora, oracle):
    """sora_hip_ingest(44 -> 40) in front of sora_rx with sample_rate_mhz = 44, against CreateDemodGraph11a_44M's recorded events"""
    import torch
    caps, want = _set("11a44", oracle)
    parts, descs, pos = [], [], 0
    for i, c in enumerate(caps):
        x = sora.ingest(torch.from_numpy(c.iq).cuda(), sora.INGEST_44TO40)
        n = x.shape[0] // 28 * 28
        parts.append(x[:n]); descs.append((pos, n, i)); pos += n
    iq = torch.cat(parts)
    rx = sora.Rx(len(caps), iq.shape[0], sample_rate_mhz=44, max_frames_per_capture=lc.MAX_EVENTS["11a44"])
    rx.process_dev(iq, descs)
    per = _per_capture(rx.results(), len(caps)); rx.close()
    _check("11a44", caps, per, want, "44 MHz ingest")
    _live_second_check("11a44", caps, want)


def _stream_of(chain, oracle):
    caps, want = _set(chain, oracle)
    i = next(i for i, c in enumerate(caps) if c.family == "stream")
    return caps[i], want[i]


def test_rx_stream_mode_cut_at_arbitrary_bursts(sora, oracle):
    """the stream capture (captures of every family back to back) handed over in 17 pieces: the rows of all calls are the uncut capture's recorded events"""
    import torch
    from test_gpu_stream import _run_in_pieces
    cap, want = _stream_of("11a", oracle)
    rng = np.random.default_rng(11)
    cuts = sorted(int(c) * 28 for c in rng.choice(np.arange(1, len(cap.iq) // 28), size=16, replace=False)) + [len(cap.iq)]
    got, calls = _run_in_pieces(sora, torch, [cap.iq], [cuts], max_frames=lc.MAX_EVENTS["11a"])
    assert calls == 17 and len(want) >= 8
    _check("11a", [cap], got, [want], "stream mode")


# ------------------------------------------------------------------ 802.11b: sora_rx11b
@pytest.mark.parametrize("plan", [0, 1, 2])
def test_rx11b_under_every_pass_plan(sora, oracle, plan):
    """0: two passes (Barker scan, then the CCK-capable kernel where needed), 1: every capture straight through the CCK-capable kernel, 2: automatic"""
    import torch
    caps, want = _set("11b", oracle)
    descs, pos = [], 0
    for i, c in enumerate(caps):
        descs.append((pos, len(c.iq), i)); pos += len(c.iq)
    rx = sora.Rx11b(len(caps), pos, max_frames_per_capture=lc.MAX_EVENTS["11b"])
    rx.set_single_pass(plan)
    assert rx.set_single_pass(-1) == plan
    rx.process_dev(torch.from_numpy(np.concatenate([c.iq for c in caps])).cuda(), descs)
    per = _per_capture(rx.results(), len(caps)); rx.close()
    _check("11b", caps, per, want, "pass plan %d" % plan)
    if plan == 2:
        _live_second_check("11b", caps, want)


def test_rx11b_stream_mode_cut_at_arbitrary_bursts(sora, oracle):
    from test_gpu_stream11b import _run_in_pieces
    cap, want = _stream_of("11b", oracle)
    got, history, final = _run_in_pieces(sora, [cap.iq], np.random.default_rng(12), step=(1, 1500), max_frames=lc.MAX_EVENTS["11b"])
    assert len(history) > 8 and len(want) >= 8 and all(e[1] <= final[0] for e in want)
    _check("11b", [cap], got, [want], "stream mode")


# ------------------------------------------------------------------ 802.11n 2x2: sora_rx11n
def _run_11n(sora, caps, trellis=None, mcs_max=None):
    import torch
    descs, pos = [], 0
    for i, c in enumerate(caps):
        descs.append((pos, len(c.iq[0]), i)); pos += len(c.iq[0])
    rx = sora.Rx11n(len(caps), pos, max_frames_per_capture=lc.MAX_EVENTS["11n"])
    if trellis is not None:
        rx.set_trellis(trellis)
        assert rx.trellis() == trellis
    if mcs_max is not None:
        rx.set_mcs_max(mcs_max)
        assert rx.set_mcs_max(-1) == mcs_max
    rx.process_dev(torch.from_numpy(np.concatenate([c.iq[0] for c in caps])).cuda(), torch.from_numpy(np.concatenate([c.iq[1] for c in caps])).cuda(), descs)
    per = _per_capture(rx.results(), len(caps)); rx.close()
    return per


@pytest.mark.parametrize("trellis", [None, 64, 16, 1])
def test_rx11n_under_every_trellis(sora, oracle, trellis):
    """the reference's gate (MCS 8..10): None the library's choice, 64 k_viterbi11n, 16 k_viterbi16_11n, 1 window-parallel"""
    caps, want = _set("11n", oracle)
    _check("11n", caps, _run_11n(sora, caps, trellis=trellis, mcs_max=10), want, "trellis %s" % trellis)
    if trellis is None:
        _live_second_check("11n", caps, want)


def test_rx11n_with_the_gate_at_14_equals_the_extension_model(sora, oracle):
    """sora_rx11n_set_mcs_max(14): no compiled reference decodes MCS 11..14, so tests/rx11n_ext_model.py -- the reference's graph with the one comparison
    moved, built from the reference-pinned stage functions -- is the reference (tests/test_oracle_levels.py holds it to the recorded events of these
    captures with the gate at 10)."""
    import rx11n_ext_model as model
    caps, _ = _set("11n", oracle)
    lim = lc.MAX_EVENTS["11n"]
    at14 = [lc.row_events("11n", model.rx11n(c.iq[0], c.iq[1], mcs_max=14, max_frames=lim)) for c in caps]
    assert all(len(w) < lim for w in at14) and model.parser_disagreements() == 0
    new = {e[2] for w in at14 for e in w if e[0] == lc.E_OK and e[2] > 10}
    assert new == {11, 12, 13, 14}, new                                      # the gate at 14 decodes all four, overdriven and offset ones among them
    _check("11n", caps, _run_11n(sora, caps, mcs_max=14), at14, "gate at 14")


def test_rx11n_stream_mode_cut_at_arbitrary_bursts(sora, oracle):
    from test_gpu_stream11n import _run_in_pieces
    cap, want = _stream_of("11n", oracle)
    got, history, final = _run_in_pieces(sora, [cap.iq], np.random.default_rng(13), step=(1, 120), max_frames=lc.MAX_EVENTS["11n"])
    assert len(history) > 8 and len(want) >= 8 and all(e[1] <= final[0] for e in want)
    _check("11n", [cap], got, [want], "stream mode")
