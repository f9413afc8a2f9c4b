"""The front end of the 40 MHz HT receiver on raw captures (k_scan_ht40 / k_scan_ht40_stream, k_ht40_plan, the host's event collection) held to the integer model
tests/ht40_front_model.py -- the reference's 802.11n scan on the oracle's bricks with the library's stated own definitions -- record for record
(sora_ht40_found_of): a20, mcs, ht_len, nsym, cfo, end_sample, error_code and the event count, no tolerance; noise_var within the rounding of its single-precision
sum.  The plan is held by equivalence: the records, translated by the stated rule (ht40_front_model.descriptor), fed to the descriptor call on the same buffers
must give the raw-capture call's rows and PSDU bytes, and that descriptor call is held to oracle/ht40_data_model.py bit for bit (tests/ht40_soft_check.py).  The
model itself is held to the reference-pinned receiver, to the generator and to a census of this case set in tests/test_ht40_front_model_cpu.py."""
import ctypes
import functools

import numpy as np
import pytest

import ht40_front_captures as fc
import ht40_front_model as fm
import ht40_soft_check as sc

pytestmark = pytest.mark.gpu
E_PLCP = 0x80000005
ROW_TRUNCATED = 1
FIELDS = ("a20", "mcs", "ht_len", "nsym", "cfo", "end_sample", "error_code")


@pytest.fixture(scope="module")
def env():
    import torch
    import sora_amd
    if sora_amd.device_count() <= 0:
        pytest.skip("no HIP device")
    assert sora_amd.ROW_TRUNCATED == ROW_TRUNCATED
    return torch, sora_amd


@functools.lru_cache(maxsize=None)
def case_set(joint):
    """-> (captures, iq [2, N, 2], descriptors, the model's events per capture)"""
    caps = fc.build(joint)
    iq, descs = fc.layout(caps)
    assert all(d[0] % 4 == 0 and d[0] % 8 and d[0] % 28 for d in descs)
    want = [fm.front(c.iq[0], c.iq[1], flags=fm.OWN | (fm.JOINT if joint else 0)) for c in caps]
    return caps, iq, descs, want


def dev(env, iq):
    torch, _ = env
    return torch.from_numpy(iq[0].copy()).cuda(), torch.from_numpy(iq[1].copy()).cuda()


def noise_var_differences(got, want):
    """|noise_var - S / 416| <= 2^-19 S / 416 (at most 16 roundings of 2^-24 each on any path through a sum of non-negative terms and one multiply, doubled),
    exactly 0.0 where S = 0 -> the violations"""
    bad = []
    for i, (g, w) in enumerate(zip(got, want)):
        exact = fm.noise_var_of(w["S"]); nv = float(g["noise_var"])
        if (w["S"] == 0 and nv != 0.0) or abs(nv - exact) > 2.0 ** -19 * exact:
            bad.append((i, nv, exact))
    return bad


def record_differences(names, got, want, mf):
    """got / want: per capture the library's records and the model's events -> [(capture, what)]"""
    diffs = []
    for name, g, w in zip(names, got, want):
        if len(g) != min(len(w), mf):
            diffs.append((name, "%d records, the model has %d events (row slots: %d)" % (len(g), len(w), mf)))
        for i, (a, b) in enumerate(zip(g, w)):
            d = [(f, a[f], b[f]) for f in FIELDS if a[f] != b[f]]
            if d:
                diffs.append((name, "event %d: (field, library, model) %r" % (i, d)))
        for i, nv, exact in noise_var_differences(g, w):
            diffs.append((name, "event %d: noise_var %r, S / 416 = %r" % (i, nv, exact)))
    return diffs


def check_records(names, got, want, mf, what):
    diffs = record_differences(names, got, want, mf)
    assert not diffs, "%s: %d of %d captures differ from the model; the first: %r" % (what, len({d[0] for d in diffs}), len(names), diffs[0])


def raw_call(env, f0, f1, descs, mf, joint=False, max_frames=256, max_soft=1 << 21, rx=None):
    """-> (rx, ticket, records per capture)"""
    _, sora = env
    if rx is None:
        rx = sora.RxHt40(max_frames, max_soft)
        if joint:
            rx.set_coding(sora.HT40_CODING_JOINT)
    t = rx.process_captures_dev(f0, f1, descs, max_frames_per_capture=mf)
    rx.wait(t)
    return rx, t, [rx.found(c, ticket=t) for c in range(len(descs))]


def expected_rows(descs, want, mf, joint):
    """the rows a raw-capture call reports, as far as the front end decides them: (capture_id, stream, end_sample, error_code or None for a recorded frame's
    verdict, rate_kbps = MCS, nsym, flags) in (capture, time) order"""
    rows = []
    for d, ev in zip(descs, want):
        for i, e in enumerate(ev[:mf]):
            flag = ROW_TRUNCATED if (i + 1 == mf and len(ev) > mf) else 0
            if e["error_code"]:
                rows.append((d[2], 0, e["end_sample"], E_PLCP, 0, 0, flag))
            else:
                rows += [(d[2], s, e["end_sample"], None, e["mcs"], e["nsym"], flag) for s in range(1 if joint else 2)]
    return rows


def check_rows_against_the_front_model(rows, descs, want, mf, joint, what):
    exp = expected_rows(descs, want, mf, joint)
    assert len(rows) == len(exp), (what, len(rows), len(exp))
    for r, e in zip(rows, exp):
        got = (r["capture_id"], r["stream"], r["end_sample"], None if e[3] is None else r["error_code"], r["rate_kbps"], r["nsym"], r["flags"])
        assert got == e, (what, got, e)
        if e[3] is not None:
            assert (r["length"], r["crc32"], r["mpdu"]) == (0, 0, b""), (what, got)
        else:
            assert r["error_code"] in (0x1, 0x80000006), (what, got, hex(r["error_code"]))


# ------------------------------------------------------------------ 1. the records
def test_records_of_every_capture_equal_the_model(env):
    caps, iq, descs, want = case_set(False)
    f0, f1 = dev(env, iq)
    rx, t, got = raw_call(env, f0, f1, descs, fc.MAX_EVENTS)
    rx.close()
    check_records([c.name for c in caps], got, want, fc.MAX_EVENTS, "every family")
    assert sum(len(g) for g in got) > len(caps) // 2 and any(len(w) > fc.MAX_EVENTS for w in want)


# ------------------------------------------------------------------ 2. the plan, by equivalence, and the whole call to the two models
@pytest.mark.parametrize("joint", [False, True], ids=["per-stream", "joint"])
def test_plan_equals_the_descriptor_call_on_the_translated_records(env, joint):
    torch, sora = env
    caps, iq, descs, want = case_set(joint)
    mf = fc.MAX_EVENTS
    f0, f1 = dev(env, iq)
    rx, t, got = raw_call(env, f0, f1, descs, mf, joint)
    check_records([c.name for c in caps], got, want, mf, "joint coding" if joint else "per-stream coding")
    raw = rx.results(ticket=t)
    check_rows_against_the_front_model(raw, descs, want, mf, joint, "raw-capture rows")
    # the records -> descriptors, by the stated rule, with the call's own measured noise_var
    fdescs = [fm.descriptor(d[0], r, float(r["noise_var"]), joint, d[2]) for d, g in zip(descs, got) for r in g if r["error_code"] == 0]
    assert len(fdescs) >= 50 and sum(d[6] > 0 for d in fdescs) >= 30, len(fdescs)
    assert any(r["error_code"] == 0 and r["cfo"] < 0 and r["cfo"] % 2 for g in got for r in g)         # cfo / 2 is not cfo >> 1 there
    w = torch.zeros((len(fdescs), 4, 128, 2), dtype=torch.int16, device="cuda")
    td = rx.process_dev(f0, f1, fdescs, w)
    rows = rx.results(ticket=td)
    jpf = 1 if joint else 2
    soft = [rx.soft(f, 0, ticket=td) if joint else [rx.soft(f, s, ticket=td) for s in range(2)] for f in range(len(fdescs))]
    rx.close()
    # the raw-capture call's rows of recorded frames are the descriptor call's, byte for byte
    framed = [r for r in raw if r["error_code"] != E_PLCP]
    assert len(framed) == len(rows) == jpf * len(fdescs)
    for a, b in zip(framed, rows):
        nb, cr = fm.MCS2[a["rate_kbps"]]
        assert (a["stream"], a["error_code"], a["length"], a["crc32"], a["nsym"], 10 * nb + cr, a["capture_id"], a["mpdu"]) == \
               (b["stream"], b["error_code"], b["length"], b["crc32"], b["nsym"], b["rate_kbps"], b["capture_id"], b["mpdu"]), (a["capture_id"], a["stream"])
    # ... and the descriptor call is the data-field model's, every soft byte, row field and PSDU byte
    got_d = {"rows": rows, "soft": soft, "w": w.cpu().numpy()}
    if joint:
        sc.assert_is_the_joint_model(got_d, sc.joint_models(iq, fdescs, got_d["w"]), fdescs, "joint")
    else:
        sc.assert_is_the_model(got_d, sc.models(iq, fdescs, got_d["w"]), fdescs, "per-stream")
    assert sum(r["error_code"] == 1 for r in rows) >= len(rows) // 2               # most of them are frames that decode


# ------------------------------------------------------------------ 3. more captures than one chunk of k_ht40_plan
@functools.lru_cache(maxsize=None)
def chunk_set():
    """1030 captures: 28 zeros each but 0, 1022, 1023, 1024, 1025 and 1029 -- frames of all three code rates and a header failure on each side of capture 1024"""
    caps = {c.name: c for c in case_set(False)[0]}
    pick = {0: "mcs13 len106", 1022: "mcs9 len105", 1023: "gate crc8", 1024: "mcs10 len118", 1025: "gate mcs15", 1029: "mcs14 len119"}
    parts, descs, pos, which = [], [], 0, []
    for i in range(1030):
        c = caps[pick[i]].iq if i in pick else (np.zeros((28, 2), np.int16),) * 2
        parts.append(np.stack(c)); descs.append((pos, len(c[0]), 5000 + i)); pos += len(c[0]); which.append(caps[pick[i]] if i in pick else None)
    want = [fm.front(c.iq[0], c.iq[1]) if c is not None else [] for c in which]
    assert [fm.MCS2[w[0]["mcs"]][1] for i, w in enumerate(want) if i in (0, 1022, 1024)] == [1, 0, 2]
    assert [w[0]["error_code"] for i, w in enumerate(want) if i in (1023, 1025)] == [E_PLCP, E_PLCP]
    return np.concatenate(parts, axis=1), descs, want


def test_1030_captures_carry_the_plan_across_its_chunk_boundary(env):
    _, sora = env
    iq, descs, want = chunk_set()
    f0, f1 = dev(env, iq)
    key = lambda r: (r["capture_id"], r["stream"], r["end_sample"], r["error_code"], r["rate_kbps"], r["length"], r["nsym"], r["crc32"], r["flags"], r["mpdu"])
    rx, t, got = raw_call(env, f0, f1, descs, 2, max_frames=16, max_soft=1 << 18)
    check_records(["capture %d" % i for i in range(1030)], got, want, 2, "1030 captures")
    buf = sora.HostResults(2 * 2 * 1030, 1 << 16)
    t2 = rx.process_captures_dev(f0, f1, descs, max_frames_per_capture=2)
    rx.deliver_async(t2, buf); rx.wait(t2)
    whole = rx.results(ticket=t2)
    check_rows_against_the_front_model(whole, descs, want, 2, False, "1030 captures")
    assert [key(r) for r in buf.results()] == [key(r) for r in whole]                # evbase, evn and the templates behind the boundary
    halves = []
    for part in (descs[:1024], descs[1024:]):
        tp = rx.process_captures_dev(f0, f1, part, max_frames_per_capture=2)
        halves += rx.results(ticket=tp)
    assert [key(r) for r in whole] == [key(r) for r in halves] and len(whole) == 2 * 4 + 2
    assert sum(r["error_code"] == 1 for r in whole) == 8
    buf.close(); rx.close()


# ------------------------------------------------------------------ 4. row slots
@pytest.mark.parametrize("mf", [1, 2])
def test_row_slots_keep_the_first_events_and_flag_the_last(env, mf):
    caps, _, _, _ = case_set(False)
    c = next(c for c in caps if c.name.startswith("three frames") and len(fm.front(c.iq[0], c.iq[1])) == 3)
    want = [fm.front(c.iq[0], c.iq[1])]
    iq = np.stack(c.iq); descs = [(0, len(c.iq[0]), 9)]
    f0, f1 = dev(env, iq)
    rx, t, got = raw_call(env, f0, f1, descs, mf, max_frames=8, max_soft=1 << 18)
    assert len(got[0]) == mf                                                       # the capped count
    check_records([c.name], got, want, mf, "%d row slots" % mf)
    rows = rx.results(ticket=t)
    check_rows_against_the_front_model(rows, descs, want, mf, False, "%d row slots" % mf)
    assert [r["flags"] for r in rows] == [0] * (2 * mf - 2) + [ROW_TRUNCATED] * 2
    rx.close()


# ------------------------------------------------------------------ 5. stream mode
def test_a_capture_fed_in_pieces_leaves_the_uncut_captures_records(env):
    caps, _, _, _ = case_set(False)
    c = next(c for c in caps if c.name == "three frames, gaps (200, 300, 444)")
    want = fm.front(c.iq[0], c.iq[1])
    assert len(want) == 3 and all(e["error_code"] == 0 for e in want)
    n = len(c.iq[0])
    _, sora = env
    f0, f1 = dev(env, np.stack(c.iq))
    uncut, _, ref = raw_call(env, f0, f1, [(0, n, 3)], 4, max_frames=8, max_soft=1 << 18)
    uncut.close()
    check_records([c.name], ref, [want], 4, "uncut")
    for cuts in ((28 * 40, 28 * 41, 28 * 100, 28 * 180), (28 * 73, 28 * 74, 28 * 150)):      # inside the first frame's preamble and data field, between frames ...
        rx = sora.RxHt40(8, 1 << 18)
        assert rx.set_stream_mode(1) == 0
        pos, got = 0, []
        for end in cuts + (n,):
            t = rx.process_captures_dev(f0[pos:], f1[pos:], [(0, end - pos, 3)], max_frames_per_capture=4)
            rx.wait(t)
            for r in rx.found(0, ticket=t):                                        # a20 and end_sample count from the piece's first sample
                got.append(dict(r, a20=r["a20"] + pos // 2, end_sample=r["end_sample"] + pos))
            used = int(rx.stream_consumed(t, 1)[0])
            assert used % 28 == 0 and used <= end - pos
            pos += used
        rx.close()
        check_records([c.name], [got], [want], 4, "cut at %r" % (cuts,))
        assert [r["noise_var"].tobytes() for r in got] == [r["noise_var"].tobytes() for r in ref[0]], cuts      # noise_var: the same bits


# ------------------------------------------------------------------ 6. the read-out's own contract
def test_found_of_answers_what_it_says_and_refuses_the_rest(env):
    torch, sora = env
    caps, _, _, _ = case_set(False)
    pick = [next(c for c in caps if c.name == n) for n in ("mcs9 len105", "gate crc8", "10 events")]
    iq, descs = fc.layout(pick)
    want = [fm.front(c.iq[0], c.iq[1]) for c in pick]
    f0, f1 = dev(env, iq)
    L = sora.load(); nf = ctypes.c_size_t(77); one = (sora.capi.Ht40Found * 1)()
    # a handle with room for three frames: the captures hold nine -- SORA_ERR_CAPACITY, and the records are there all the same
    rx = sora.RxHt40(3, 1 << 20)
    t = rx.process_captures_dev(f0, f1, descs, max_frames_per_capture=fc.MAX_EVENTS)
    with pytest.raises(sora.SoraError) as e:
        rx.wait(t)
    assert e.value.code == -6
    check_records([c.name for c in pick], [rx.found(c, ticket=t) for c in range(3)], want, fc.MAX_EVENTS, "after SORA_ERR_CAPACITY")
    # the count also when the buffer is too small, and nothing copied
    assert L.sora_ht40_found_of(rx._h, t, 2, one, 1, ctypes.byref(nf)) == -6 and nf.value == fc.MAX_EVENTS and one[0].end_sample == 0
    assert L.sora_ht40_found_of(rx._h, t, 0, one, 1, ctypes.byref(nf)) == 0 and nf.value == 1 and one[0].end_sample == want[0][0]["end_sample"]
    with pytest.raises(sora.SoraError) as e:
        rx.found(3, ticket=t)                                                      # a capture index past the call's
    assert e.value.code == -1 and "no such capture" in str(e.value)
    td = rx.process_dev(f0, f1, [])                                                # a descriptor call
    with pytest.raises(sora.SoraError) as e:
        rx.found(0, ticket=td)
    assert e.value.code == -1 and "raw-capture calls" in str(e.value)
    rx.synchronize(); rx.close()
    # nine calls over the eight slots: the oldest answers while its ticket is live, and no longer once its slot is reused
    rx = sora.RxHt40(16, 1 << 20)
    assert rx.calls_in_flight() == 8
    tickets = [rx.process_captures_dev(f0, f1, descs[k % 3:k % 3 + 1], max_frames_per_capture=fc.MAX_EVENTS) for k in range(8)]
    check_records([pick[0].name], [rx.found(0, ticket=tickets[0])], want[:1], fc.MAX_EVENTS, "the oldest of eight calls")
    tickets.append(rx.process_captures_dev(f0, f1, descs[2:3], max_frames_per_capture=fc.MAX_EVENTS))
    with pytest.raises(sora.SoraError) as e:
        rx.found(0, ticket=tickets[0])
    assert e.value.code == -1 and "stale ticket" in str(e.value)
    for k in range(1, 9):
        check_records([pick[k % 3].name], [rx.found(0, ticket=tickets[k])], want[k % 3:k % 3 + 1], fc.MAX_EVENTS, "call %d of nine" % k)
    assert rx.found(0) == rx.found(0, ticket=tickets[-1])                          # ticket None: the most recent call
    rx.synchronize(); rx.close()
