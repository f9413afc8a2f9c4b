"""Stream continuation of the 44 MHz 802.11a graph (sora_rx_set_stream_mode with sample_rate_mhz = 44, include/sora_hip.h): a 44 MHz stream
handed to the library in pieces, each ingested on its own (sora_hip_ingest(SORA_INGEST_44TO40), or inside sora_rx_process_dump), must yield
exactly the events CreateDemodGraph11a_44M reports on the UNCUT stream.  The host resubmits the 44 MHz source from used * 11 / 10, a
multiple of 308 samples, where TDownSample44_40 holds nothing (tests/test_stream44_cpu.py checks that premise)."""
import numpy as np
import pytest

from gpu_util import make_capture, random_capture, same_as_reference_graph, source_position_44, upsample_40_to_44

pytestmark = pytest.mark.gpu

TAIL44 = 308 * 210           # quiet behind every test stream: longer than what is left of any frame random_capture truncates, so every event is followed by a resume point


@pytest.fixture(scope="module")
def sora():
    import sora_amd
    sora_amd.load()
    assert sora_amd.device_count() > 0
    return sora_amd


def _close(x, tail=TAIL44):
    """whole RX_BLOCKs, then `tail` quiet samples, up to a whole resampler period"""
    n = len(x) // 28 * 28 + tail
    n += (-n) % 308
    out = np.zeros((n, 2), np.int16); out[:len(x) // 28 * 28] = x[:len(x) // 28 * 28]
    return out


def _stream(oracle, rng, ncaps):
    """random 40 MHz captures (frames of all rates and lengths, gaps, DC and gain steps, carrier offsets, noise, bare noise) at 44 MHz, back to back"""
    return _close(np.concatenate([upsample_40_to_44(random_capture(oracle, rng, 40)) for _ in range(ncaps)]))


def _reference_events(oracle, stream44):
    from oracle.pyoracle import ReferenceGraph
    g = ReferenceGraph()
    if g.available():
        return g.rx11a_44(stream44, max_frames=256), "reference"
    ev = []
    for r in oracle.rx_capture(oracle.down44to40(stream44), 44, max_frames=256):   # the restatement, pinned to that graph in test_oracle_vs_refgraph.py
        e = dict(r); e["sample_index"] = source_position_44(r["end_sample"]); ev.append(e)
    return ev, "port"


def _open(sora, ns, total, front=None, depth=None, max_frames=32):
    rx = sora.Rx(ns, total + 64 * ns, sample_rate_mhz=44, max_frames_per_capture=max_frames)
    if front is not None:
        rx.set_front(front)
    if depth is not None:
        rx.set_depth(depth)
    assert rx.set_stream_mode(1) == 0 and rx.set_stream_mode(-1) == 1
    return rx


def _call(sora, torch, rx, pieces, dump=False):
    """One call, capture k = pieces[k] (44 MHz samples, whole RX_BLOCKs).  dump=False: each piece ingested on its own on the device, then
    process_dev.  dump=True: one RX_BLOCK dump through process_dump, every piece starting a multiple of 11 blocks in (zero blocks between),
    capture offset (first block / 11) * 280, length ingest_count(piece bytes).  -> (ticket, capture lengths)"""
    if dump:
        from test_oracle_ingest import make_dump
        flags = sora.INGEST_RXBLOCK | sora.INGEST_44TO40
        blocks, descs, nb = [], [], 0
        for k, p in enumerate(pieces):
            d = make_dump(p, raw14=False, seed=k).reshape(-1, 128) if len(p) else np.zeros((0, 128), np.uint8)
            descs.append((nb // 11 * 280, sora.ingest_count(len(d) * 128, flags), k))
            pad = (-len(d)) % 11
            blocks += [d, np.zeros((pad, 128), np.uint8)]
            nb += len(d) + pad
        if nb == 0:
            blocks.append(np.zeros((11, 128), np.uint8))                 # (a call of empty pieces still hands over a dump)
        raw = np.ascontiguousarray(np.concatenate(blocks).reshape(-1))
        return rx.process_dump(raw, flags, descs), [d[1] for d in descs]
    parts, descs, off = [], [], 0
    for k, p in enumerate(pieces):
        n = sora.ingest_count(len(p) * 4, sora.INGEST_44TO40)
        if n:
            x = sora.ingest(torch.from_numpy(np.ascontiguousarray(p)).cuda(), sora.INGEST_44TO40)
            assert x.shape[0] == n
            parts.append(x)
        descs.append((off, n, k)); off += n                              # (n is a multiple of 28: offsets stay 4-aligned)
    iq = torch.cat(parts) if parts else torch.zeros((4, 2), dtype=torch.int16, device="cuda")
    return rx.process_dev(iq, descs), [d[1] for d in descs]


def _run_in_pieces(sora, torch, streams, cuts, front=None, depth=None, dump=False, max_frames=32, rx=None):
    """streams: 44 MHz int16 [n, 2]; cuts[k]: increasing RX_BLOCK boundaries (multiples of 28, not necessarily of 308) at which the samples
    that have arrived of stream k end, call by call.  Every call carries one capture per stream: from where the call before left it to the cut."""
    ns = len(streams)
    own = rx is None
    if own:
        rx = _open(sora, ns, sum(len(s) for s in streams), front, depth, max_frames)
    base = [0] * ns                                                      # 44 MHz source position of each capture's first sample
    events = [[] for _ in range(ns)]
    calls = 0
    useds = []
    for i in range(len(cuts[0])):
        pieces = [streams[k][base[k]:max(base[k], cuts[k][i])] for k in range(ns)]
        t, lens = _call(sora, torch, rx, pieces, dump)
        rows = rx.results(ticket=t)
        used = rx.stream_consumed(t, ns)
        calls += 1
        for k in range(ns):
            assert used[k] % 280 == 0 and used[k] <= lens[k], (used[k], lens[k])
            for r in rows:                                               # a reported frame lies in front of the resume point
                if r["capture_id"] == k:
                    assert source_position_44(r["end_sample"]) <= used[k] * 11 // 10, (r["end_sample"], used[k])
        for r in rows:
            k = r["capture_id"]
            r = dict(r); r["start_sample"] += base[k] * 10 // 22; r["end_sample"] += base[k] * 10 // 22    # base / 308 periods of 140
            events[k].append(r)
        for k in range(ns):
            base[k] += int(used[k]) * 11 // 10
        useds.append([int(u) for u in used])
    if own:
        rx.close()
    return events, calls, useds


def _random_cuts(rng, n, npieces):
    return sorted(int(c) * 28 for c in rng.integers(1, n // 28, size=npieces - 1)) + [n]


def test_pieces_cut_at_arbitrary_rx_blocks_report_what_the_uncut_stream_reports(sora, oracle):
    """Random streams, 1-3 per call, cut at random RX_BLOCK boundaries; every front-end choice at depth 1 and 3; some calls through process_dump."""
    import torch
    rng = np.random.default_rng(20261016)
    total_events = 0; kinds = set()
    plans = [(None, None, False), (1, 1, False), (3, 3, False), (4, 1, False), (None, 3, True), (1, 3, True), (3, 1, False), (4, 3, True)]
    for trial in range(16):
        front, depth, dump = plans[trial % len(plans)]
        ns = 1 + trial % 3
        streams = [_stream(oracle, rng, int(rng.integers(3, 8))) for _ in range(ns)]
        want = [_reference_events(oracle, s) for s in streams]
        npieces = int(rng.integers(2, 14))
        cuts = [_random_cuts(rng, len(s), npieces) for s in streams]
        got, calls, _ = _run_in_pieces(sora, torch, streams, cuts, front=front, depth=depth, dump=dump)
        for k in range(ns):
            ok, why = same_as_reference_graph(got[k], want[k][0], position=source_position_44)
            assert ok, "trial %d stream %d (%d pieces, front %s, depth %s, dump %s, against the %s): %s" % (trial, k, npieces, front, depth, dump, want[k][1], why)
            total_events += len(want[k][0]); kinds.update(e["error_code"] for e in want[k][0])
    assert total_events > 60 and {0x1, 0x80000005} <= kinds, (total_events, kinds)


def test_a_frame_over_many_short_pieces_is_reported_once(sora, oracle):
    """A 1500-byte 6 Mbps frame (about 89 k samples at 44 MHz) over pieces of 3,360 samples: nothing is consumed while it runs, and it is
    reported once.  The same pieces with the mode off lose it."""
    import torch
    rng = np.random.default_rng(7)
    cap = make_capture(oracle, 6000, 1500, seed=3, rate_mhz=40, sigma=40, lead=56 * 9, tail=560)[0]
    noise = np.rint(rng.normal(0, 30, (28 * 40, 2))).astype(np.int16)
    stream = _close(upsample_40_to_44(np.concatenate([noise, cap, noise])), tail=308 * 4)
    want, kind = _reference_events(oracle, stream)
    assert len(want) == 1 and want[0]["error_code"] == 1
    cuts = list(range(28 * 120, len(stream), 28 * 120)) + [len(stream)]
    got, calls, useds = _run_in_pieces(sora, torch, [stream], [cuts], max_frames=4)
    ok, why = same_as_reference_graph(got[0], want, position=source_position_44)
    assert ok, why
    assert calls >= 25
    assert sum(u[0] == 0 for u in useds) >= 20                          # the calls inside the frame consume nothing
    rx = sora.Rx(1, len(stream), sample_rate_mhz=44, max_frames_per_capture=4)
    lost = 0
    for a, b in zip([0] + cuts[:-1], cuts):
        x = sora.ingest(torch.from_numpy(np.ascontiguousarray(stream[a:b])).cuda(), sora.INGEST_44TO40)
        rx.process_dev(x, [(0, x.shape[0], 0)])
        lost += len(rx.results())
    assert lost == 0
    rx.close()


def _queued_after(ev):
    """20 MHz-rate samples left in front of TDownSample2 when the graph resets after an event at the end of burst ev: the source call that
    delivers that burst ends at ce, the whole bursts up to it are still taken (consumed_to), the rest waits.  Bursts are 4, calls 14 here,
    so that is 0 or 2; with 2 the walk goes on at ce - 2 where the 40 MHz graph (which flushes) goes on at ce."""
    ce = -(-ev // 14) * 14
    return (ce - ev) % 4


def _two_frames(oracle):
    """A frame that leaves samples in TDownSample2's queue when the graph resets, and a second one close behind it, with the resampler's
    period boundaries just after the first frame's event and in the gap."""
    for seed in range(40):
        a = make_capture(oracle, 24000, 100 + seed, seed=11 + seed, rate_mhz=40, sigma=30, lead=280, tail=0)[0]
        b = make_capture(oracle, 12000, 60, seed=91 + seed, rate_mhz=40, sigma=30, lead=600, tail=400)[0]
        s44 = _close(upsample_40_to_44(np.concatenate([a, b])), tail=308 * 3)
        port = oracle.rx_capture(oracle.down44to40(s44), 44)
        if len(port) == 2 and all(r["error_code"] == 1 for r in port) and _queued_after(port[0]["end_sample"]) == 2:
            return s44, port
    raise AssertionError("no two-frame stream with a queued tail behind the first frame")


def test_the_queue_a_frame_leaves_holds_across_a_cut(sora, oracle):
    """TDownSample44_40 has no Reset/Flush: after a frame the samples in front of TDownSample2 are processed (keep_queue).  Cut just after the
    first frame, at the first resume point behind it, and one period later: the second frame is found as on the uncut stream."""
    import torch
    s44, port = _two_frames(oracle)
    want, kind = _reference_events(oracle, s44)
    assert len(want) == 2
    assert _queued_after(port[0]["end_sample"]) == 2                     # the first frame leaves two samples queued
    ev1 = want[0]["sample_index"]
    rp = -(-ev1 // 308) * 308
    for cut in (ev1, ev1 + 28, rp, rp + 308, rp + 28):
        got, calls, useds = _run_in_pieces(sora, torch, [s44], [[cut, len(s44)]])
        ok, why = same_as_reference_graph(got[0], want, position=source_position_44)
        assert ok, "cut at %d (first event at %d, %s): %s" % (cut, ev1, kind, why)
        if cut >= rp:                                                   # the first frame is final there, and reported by the first call
            assert useds[0][0] * 11 // 10 >= rp, (cut, useds)
        else:                                                           # nothing behind the first frame's last resume point is final yet: it is withheld
            assert useds[0][0] * 11 // 10 < ev1, (cut, useds)


def test_a_withheld_frame_leaves_a_bound_mpdu_array_alone(sora, oracle):
    """A capture that ends between a frame's event and the resume point behind it withholds the frame: no row, and (sora_rx_bind_mpdu) no byte
    of the caller's array written.  The next call reports it with its MPDU."""
    import torch
    s44, port = _two_frames(oracle)
    want, _ = _reference_events(oracle, s44)
    ev1 = want[0]["sample_index"]
    x = sora.ingest(torch.from_numpy(np.ascontiguousarray(s44[:ev1])).cuda(), sora.INGEST_44TO40)
    descs = [(0, x.shape[0], 0)]
    probe = sora.Rx(1, x.shape[0], sample_rate_mhz=44, max_frames_per_capture=4)
    t = probe.process_dev(x, descs)
    nbytes = probe.mpdu_bytes(t)
    assert len(probe.results(ticket=t)) == 1                           # with the mode off the piece holds the frame's event
    probe.close()
    rx = _open(sora, 1, len(s44), max_frames=4)
    buf = sora.HostResults(4, nbytes)
    buf.mpdu[:] = 0xEE
    rx.bind_mpdu(buf)
    t = rx.process_dev(x, descs); rx.deliver_async(t, buf); rx.wait(t)
    used44 = int(rx.stream_consumed(t, 1)[0]) * 11 // 10
    assert int(buf.nrows[0]) == 0 and used44 < ev1, (int(buf.nrows[0]), used44, ev1)
    assert np.all(buf.mpdu == 0xEE)
    x2 = sora.ingest(torch.from_numpy(np.ascontiguousarray(s44[used44:])).cuda(), sora.INGEST_44TO40)
    t = rx.process_dev(x2, [(0, x2.shape[0], 0)])
    rows = [dict(r) for r in rx.results(ticket=t)]
    for r in rows:
        r["end_sample"] += used44 * 10 // 22
    ok, why = same_as_reference_graph(rows, want, position=source_position_44)
    assert ok, why
    buf.close(); rx.close()


def test_a_carrier_sense_timeout_cut_in_the_middle(sora, oracle):
    """Loud noise trips carrier sense again and again (E_CS_TIMEOUT resets it at the end of a source call); pieces cut inside it, a frame
    behind it."""
    import torch
    rng = np.random.default_rng(31)
    quiet = np.rint(rng.normal(0, 30, (28 * 20, 2))).astype(np.int16)
    loud = np.rint(rng.normal(0, 3000, (28 * 150, 2))).astype(np.int16)
    cap = make_capture(oracle, 36000, 300, seed=5, rate_mhz=40, sigma=60, lead=200, tail=400)[0]
    stream = _close(upsample_40_to_44(np.concatenate([quiet, loud, cap])), tail=308 * 3)
    want, kind = _reference_events(oracle, stream)
    assert any(e["error_code"] == 1 for e in want)
    for first in range(28 * 22, 28 * 22 + 308 * 6, 28 * 5):
        cuts = [first, first + 28 * 13, first + 308 * 4 + 56, len(stream)]
        got, calls, useds = _run_in_pieces(sora, torch, [stream], [cuts])
        ok, why = same_as_reference_graph(got[0], want, position=source_position_44)
        assert ok, "cuts %s: %s" % (cuts, why)


def test_reset_mode_switch_zero_length_and_short_pieces(sora, oracle):
    import torch
    rng = np.random.default_rng(99)
    stream = _stream(oracle, rng, 4)
    want, _ = _reference_events(oracle, stream)
    assert want
    rx = _open(sora, 2, 2 * len(stream))
    # a piece shorter than one period consumes nothing; a zero-length capture neither; the stream goes on unharmed
    t, lens = _call(sora, torch, rx, [stream[:28 * 10], stream[:0]])
    assert list(rx.stream_consumed(t, 2)) == [0, 0] and lens[1] == 0
    t, lens = _call(sora, torch, rx, [stream[:28 * 10], stream[:28 * 10]])
    assert list(rx.stream_consumed(t, 2)) == [0, 0]
    got, _, _ = _run_in_pieces(sora, torch, [stream, stream], [_random_cuts(rng, len(stream), 6)] * 2, rx=rx)
    for k in range(2):
        ok, why = same_as_reference_graph(got[k], want, position=source_position_44)
        assert ok, "after short pieces, stream %d: %s" % (k, why)
    # sora_rx_reset and a mode switch start every stream afresh: the same stream from its start gives the same events again
    for restart in ("reset", "switch"):
        if restart == "reset":
            rx.reset()
        else:
            assert rx.set_stream_mode(0) == 1 and rx.set_stream_mode(1) == 0
        got, _, _ = _run_in_pieces(sora, torch, [stream, stream], [_random_cuts(rng, len(stream), 5)] * 2, rx=rx)
        for k in range(2):
            ok, why = same_as_reference_graph(got[k], want, position=source_position_44)
            assert ok, "after %s, stream %d: %s" % (restart, k, why)
    # with the mode off the call does what it always did: the uncut stream as one capture
    rx.set_stream_mode(0)
    t, _ = _call(sora, torch, rx, [stream, stream[:0]])
    ok, why = same_as_reference_graph(rx.results(ticket=t), want, position=source_position_44)
    assert ok, "mode off: " + why
    rx.close()
