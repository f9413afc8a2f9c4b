"""sora_rx11n_set_mcs_max on the GPU: with the SIG parser's gate raised, the 802.11n 2x2 receive handle decodes MCS 11..14 (16-QAM, 64-QAM; code rates
1/2, 3/4, 2/3, 3/4).  No compiled reference decodes such a frame, so the rows and MPDU bytes are held to tests/rx11n_ext_model.py -- the reference's graph
with the one comparison moved, built from the reference-pinned stage functions (tests/test_rx11n_mcs_cpu.py pins it to the oracle and the compiled graph
at the default gate) -- and, for truth, to the bytes that went into the GPU modulator (sample-exact to the reference's, tests/test_gpu_tx11n.py).
Frames come from the GPU modulator, so nothing here needs oracle/_ref."""
import numpy as np
import pytest

import rx11n_ext_model as model
from gpu_util import capture_11n

pytestmark = pytest.mark.gpu
E_OK, E_PLCP, E_CRC = 0x1, 0x80000005, 0x80000006
KEY = lambda e: (e["end_sample"], e["error_code"]) + ((e["rate_kbps"], e["length"], e["crc32"], e["mpdu"]) if e["error_code"] != E_PLCP else ())


@pytest.fixture(scope="module")
def sora():
    import sora_amd
    sora_amd.load()
    assert sora_amd.device_count() > 0
    return sora_amd


def modulate(sora, mpdus, mcs):
    """[(s0, s1)] int16 [n,2] per frame from the GPU modulator, one launch"""
    o0, o1, off = sora.tx11n([bytes(m) for m in mpdus], list(mcs))
    a, b = o0.cpu().numpy(), o1.cpu().numpy()
    return [(a[off[i]:off[i + 1]].copy(), b[off[i]:off[i + 1]].copy()) for i in range(len(mpdus))]


def layout(caps):
    iq0 = np.ascontiguousarray(np.concatenate([a for a, _ in caps])); iq1 = np.ascontiguousarray(np.concatenate([b for _, b in caps]))
    descs = []; off = 0
    for i, (a, _) in enumerate(caps):
        descs.append((off, len(a), i)); off += len(a)
    return iq0, iq1, descs


def per_capture(rows, n):
    per = [[] for _ in range(n)]
    for r in rows:
        per[r["capture_id"]].append(r)
    return per


def run_batch(sora, caps, mcs_max=None, trellis=None, max_frames=8):
    import torch
    iq0, iq1, descs = layout(caps)
    rx = sora.Rx11n(len(caps), len(iq0), max_frames_per_capture=max_frames)
    if trellis is not None:
        rx.set_trellis(trellis)
    if mcs_max is not None:
        assert rx.set_mcs_max(mcs_max) == 10
    rx.process_dev(torch.from_numpy(iq0).cuda(), torch.from_numpy(iq1).cuda(), descs)
    rows = rx.results(); rx.close()
    return per_capture(rows, len(caps))


# ---- random captures against the model
NCAPS = 420


@pytest.fixture(scope="module")
def random_set(sora):
    """420 two-chain captures: 1-3 frames of MCS 8..14 (six lengths each: short ones and up to 1496 bytes), capture_11n's gaps, gains, phases, cross-talk and CFO,
    three in ten through a 2x2 multipath channel, sigma 3..1500, every third capture cut inside its last frame -- and the model's events with the gate at 14"""
    rng = np.random.default_rng(20261019)
    mcs = [8 + k % 7 for k in range(42)]
    lens = [int(rng.integers(1, 1497)) if (k // 7) % 3 else int(rng.integers(1, 80)) for k in range(42)]
    pool = modulate(sora, [rng.integers(0, 256, n).astype(np.uint8).tobytes() for n in lens], mcs)
    caps = []
    for t in range(NCAPS):
        fr = [pool[int(i)] for i in rng.integers(0, len(pool), size=int(rng.integers(1, 4)))]
        caps.append(capture_11n(rng, fr, sigma=float(rng.choice([3, 20, 60, 200, 600, 1500])), cut=float(rng.uniform(0.05, 1.0)) if t % 3 == 2 else None, multipath_p=0.3))
    want = [model.rx11n(a, b, mcs_max=14) for a, b in caps]
    assert model.parser_disagreements() == 0
    return caps, want


def test_the_random_set_holds_decoded_and_crc_failed_frames_of_every_new_rate(random_set):
    """Floors set by the design of the set, not by what a receiver makes of it: two thirds of the captures are whole, four sevenths of their ~2 frames are
    MCS 11..14, and a third of the noise levels (sigma 3, 20) decodes them all -- some 100 decoded frames at the least; sigma 60 and 200 break the FCS of many
    of the long 64-QAM frames while leaving the header (BPSK, rate 1/2) intact."""
    caps, want = random_set
    ok = {m: 0 for m in range(8, 15)}; crc = dict(ok); plcp = 0
    for ev in want:
        for e in ev:
            if e["error_code"] == E_OK: ok[e["rate_kbps"]] += 1
            elif e["error_code"] == E_CRC: crc[e["rate_kbps"]] += 1
            else: plcp += 1
    print("FRAME_OK per MCS", ok, "CRC_FAIL per MCS", crc, "PLCP_HEADER_FAIL", plcp)
    assert sum(ok[m] for m in (11, 12, 13, 14)) >= 100 and all(ok[m] >= 10 for m in range(8, 15)), ok
    assert sum(crc[m] for m in (11, 12, 13, 14)) >= 40 and all(crc[m] >= 3 for m in (11, 12, 13, 14)), crc
    assert plcp >= 20


@pytest.mark.parametrize("depth", [1, 4])
@pytest.mark.parametrize("trellis", [0, 64, 16, 1])
def test_gpu_equals_the_model_with_the_gate_at_14(sora, random_set, trellis, depth):
    """Rows (position, code, MCS, length, FCS) and MPDU bytes, CRC-failed ones included, of every event of every capture: each trellis form (0 automatic, 64
    k_viterbi11n, 16 k_viterbi16_11n, 1 window-parallel with its proof), one call or four in flight, read by sora_rx11n_results_of and through
    sora_rx11n_deliver_async."""
    import torch
    caps, want = random_set
    parts = [list(range(NCAPS))] if depth == 1 else [list(range(k, NCAPS, 4)) for k in range(4)]
    batches = []
    for idx in parts:
        iq0, iq1, descs = layout([caps[i] for i in idx])
        batches.append((idx, torch.from_numpy(iq0).cuda(), torch.from_numpy(iq1).cuda(), descs))
    rx = sora.Rx11n(max(len(p) for p in parts), max(len(b[1]) for b in batches), max_frames_per_capture=8)
    rx.set_trellis(trellis)
    assert rx.set_depth(depth) == 1
    assert rx.set_mcs_max(14) == 10 and rx.set_mcs_max() == 14
    bufs = [sora.HostResults(len(p) * 8, len(p) * 8 * 1504) for p in parts]
    tickets = []
    for (idx, d0, d1, descs), buf in zip(batches, bufs):
        t = rx.process_dev(d0, d1, descs); rx.deliver_async(t, buf); tickets.append(t)
    nev = 0
    for (idx, _, _, _), buf, t in zip(batches, bufs, tickets):
        rx.wait(t)
        by_ticket = rx.results(ticket=t)
        delivered = buf.results()
        full = lambda r: (r["capture_id"],) + KEY(r)
        assert [full(r) for r in delivered] == [full(r) for r in by_ticket]
        per = per_capture(by_ticket, len(idx))
        for j, i in enumerate(idx):
            assert [KEY(e) for e in per[j]] == [KEY(e) for e in want[i]], (trellis, depth, i, [KEY(e)[:4] for e in per[j]], [KEY(e)[:4] for e in want[i]])
            nev += len(want[i])
    assert nev > NCAPS
    for b in bufs:
        b.close()
    rx.close()


# ---- truth: what went into the modulator comes out
def clean_set(sora, seed=20261020):
    rng = np.random.default_rng(seed)
    mcs = []; mpdus = []
    for m in (11, 12, 13, 14):
        for ln in (1, 2, 40, 1495, 1496, int(rng.integers(1, 1497)), int(rng.integers(1, 1497)), int(rng.integers(1, 1497))):
            mcs.append(m); mpdus.append(rng.integers(0, 256, ln).astype(np.uint8).tobytes())
    frames = modulate(sora, mpdus, mcs)
    caps = [model.clean_channel(rng, s0, s1, sigma=float(rng.uniform(10, 20))) for s0, s1 in frames]
    return mcs, mpdus, caps


def test_loop_back_of_gpu_modulated_frames_and_the_default_gate(sora):
    """GPU-modulated MCS 11..14 frames of 1, 2, 40, 1495, 1496 and random lengths through the clean channel (unit gain, random phases, cross-talk 0 or 0.1, CFO
    up to 2e-4, sigma 10..20): with the gate at 14 every one comes back FRAME_OK with the transmitted bytes and their FCS, under every trellis form; a handle
    left at the default reports each as the PLCP header failure it is today (the oracle's rows)."""
    from oracle.pyoracle import Oracle
    mcs, mpdus, caps = clean_set(sora)
    for trellis in (0, 64, 16, 1):
        got = run_batch(sora, caps, mcs_max=14, trellis=trellis, max_frames=4)
        for i, (m, mp) in enumerate(zip(mcs, mpdus)):
            assert [(e["error_code"], e["rate_kbps"], e["length"]) for e in got[i]] == [(E_OK, m, len(mp) + 4)], (trellis, i, m, len(mp), got[i])
            assert got[i][0]["mpdu"] == mp + model.fcs(mp) and got[i][0]["crc32"] == int.from_bytes(model.fcs(mp), "little"), (trellis, i)
            assert KEY(got[i][0]) == KEY(model.rx11n(*caps[i], mcs_max=14)[0])
    o = Oracle()
    default = run_batch(sora, caps, max_frames=4)
    explicit = run_batch(sora, caps, mcs_max=10, max_frames=4)
    for i in range(len(caps)):
        want = o.rx11n_capture(*caps[i])
        assert [e["error_code"] for e in want] == [E_PLCP]
        for got in (default[i], explicit[i]):
            assert [(e["end_sample"], e["error_code"], e["rate_kbps"], e["length"], e["crc32"], e["mpdu"]) for e in got] == [(want[0]["end_sample"], E_PLCP, 0, 0, 0, b"")], i


def test_switching_the_gate_on_one_handle(sora, random_set):
    """10 -> 14 -> 12 -> 10 on one handle, the same batch each time: each setting's rows are the model's at that gate; the return value is the previous gate;
    values outside 10..14 are refused and change nothing; at 10 the rows are the oracle's."""
    import torch
    from oracle.pyoracle import Oracle
    caps = random_set[0][:80]
    iq0, iq1, descs = layout(caps)
    d0, d1 = torch.from_numpy(iq0).cuda(), torch.from_numpy(iq1).cuda()
    rx = sora.Rx11n(len(caps), len(iq0), max_frames_per_capture=8)
    rx.set_depth(2)
    assert rx.set_mcs_max() == 10 and rx.set_mcs_max(0) == 10
    prev = 10
    o = Oracle()
    for gate in (10, 14, 12, 10, 11, 13, 10):
        assert rx.set_mcs_max(gate) == prev and rx.set_mcs_max() == gate
        prev = gate
        for bad in (9, 15, 7, 100):
            with pytest.raises(sora.SoraError):
                rx.set_mcs_max(bad)
        assert rx.set_mcs_max() == gate
        t = rx.process_dev(d0, d1, descs)
        per = per_capture(rx.results(ticket=t), len(caps))
        for i, (a, b) in enumerate(caps):
            want = model.rx11n(a, b, mcs_max=gate)
            assert [KEY(e) for e in per[i]] == [KEY(e) for e in want], (gate, i)
            if gate == 10:
                assert want == o.rx11n_capture(a, b)
    rx.close()


# ---- stream continuation with the gate raised
def test_streams_cut_at_random_source_calls_give_the_models_events_on_the_uncut_stream(sora):
    """sora_rx11n_set_stream_mode with the gate at 14: nine two-chain streams of MCS 8..14 frames handed over in pieces cut at random source calls, every
    trellis form: the rows of all calls are the model's events on each uncut stream (the gate is handle state: it outlives every call and resume point)."""
    import torch
    rng = np.random.default_rng(20261021)
    mcs = [8 + k % 7 for k in range(21)]
    pool = modulate(sora, [rng.integers(0, 256, int(rng.integers(1, 700)) if k % 3 else int(rng.integers(1, 60))).astype(np.uint8).tobytes() for k in range(21)], mcs)
    quiet = lambda n: np.rint(rng.normal(0, 3, (n, 2))).astype(np.int16)
    streams = []
    for _ in range(9):
        segs = [capture_11n(rng, [pool[int(i)] for i in rng.integers(0, len(pool), size=int(rng.integers(1, 3)))], sigma=float(rng.choice([3, 20, 60, 200, 600])),
                            cut=float(rng.uniform(0.1, 0.9)) if rng.random() < 0.15 else None, multipath_p=0.3) for _ in range(int(rng.integers(3, 8)))]
        a = np.concatenate([quiet(280)] + [s[0] for s in segs] + [quiet(28 * 150)]); b = np.concatenate([quiet(280)] + [s[1] for s in segs] + [quiet(28 * 150)])
        n = len(a) // 28 * 28
        streams.append((np.ascontiguousarray(a[:n]), np.ascontiguousarray(b[:n])))
    want = [model.rx11n(a, b, mcs_max=14, max_frames=256) for a, b in streams]
    seen = {e["rate_kbps"] for w in want for e in w if e["error_code"] == E_OK}
    assert {11, 12, 13, 14} <= seen and sum(len(w) for w in want) > 20, seen
    ns = len(streams)
    for trellis in (0, 64, 16, 1):
        rx = sora.Rx11n(ns, sum(len(s[0]) for s in streams) + 28 * ns, max_frames_per_capture=32)
        rx.set_trellis(trellis)
        assert rx.set_stream_mode(1) == 0 and rx.set_mcs_max(14) == 10
        base, arrived, done = [0] * ns, [0] * ns, [False] * ns
        events = [[] for _ in range(ns)]
        calls = 0
        while not all(done):
            s0, s1, descs, off, last = [], [], [], 0, [False] * ns
            for k, (a, b) in enumerate(streams):
                n = 0
                if not done[k]:
                    arrived[k] = min(len(a), max(arrived[k], base[k]) + 28 * int(rng.integers(1, 160)))
                    n = (arrived[k] - base[k]) // 28 * 28
                    last[k] = base[k] + n + 28 > len(a)
                s0.append(a[base[k]:base[k] + n]); s1.append(b[base[k]:base[k] + n]); descs.append((off, n, k)); off += n
            iq0 = np.ascontiguousarray(np.concatenate(s0)) if off else np.zeros((28, 2), np.int16)
            iq1 = np.ascontiguousarray(np.concatenate(s1)) if off else np.zeros((28, 2), np.int16)
            t = rx.process_dev(torch.from_numpy(iq0).cuda(), torch.from_numpy(iq1).cuda(), descs)
            rows = rx.results(ticket=t); used = rx.stream_consumed(t, ns)
            for r in rows:
                assert r["end_sample"] <= used[r["capture_id"]] and not r["flags"], r
                events[r["capture_id"]].append(dict(r, end_sample=r["end_sample"] + base[r["capture_id"]]))
            for k in range(ns):
                assert used[k] % 28 == 0 and used[k] <= descs[k][1]
                base[k] += int(used[k])
                done[k] = done[k] or (last[k] and (used[k] == 0 or len(streams[k][0]) - base[k] < 28))
            calls += 1
            assert calls < 3000
        assert rx.set_mcs_max() == 14
        rx.close()
        for k in range(ns):
            assert [KEY(e) for e in events[k]] == [KEY(e) for e in want[k]], (trellis, k, calls)


def test_window_parallel_proof_runs_on_a_lone_mcs_14_capture(sora):
    """A handle of one capture chooses the window-parallel trellis; a lone 1496-byte MCS 14 frame (26 symbols of 624 soft values, rate 3/4) is cut into units,
    every boundary is compared, and the row is the model's."""
    import torch
    rng = np.random.default_rng(14)
    mp = rng.integers(0, 256, 1496).astype(np.uint8).tobytes()
    (s0, s1), = modulate(sora, [mp], [14])
    a, b = model.clean_channel(rng, s0, s1, sigma=15.0)
    rx = sora.Rx11n(1, len(a), max_frames_per_capture=4)
    assert rx.trellis() == sora.TRELLIS_WINDOWED and rx.set_mcs_max(14) == 10
    rx.process_dev(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), [(0, len(a), 0)])
    rows = rx.results(); st = rx.window_stats(); rx.close()
    assert [KEY(e) for e in rows] == [KEY(e) for e in model.rx11n(a, b, mcs_max=14)]
    assert [(e["error_code"], e["rate_kbps"], e["mpdu"]) for e in rows] == [(E_OK, 14, mp + model.fcs(mp))]
    assert st["units"] > 1 and st["boundaries"] > 0, st
