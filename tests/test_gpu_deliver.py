"""Result delivery of the four receive handles against tests/deliver_model.py, the contract of include/sora_hip.h in plain Python: every row field, both counts and
every MPDU byte of *_deliver_async (k_dense_rows / k_dense_mpdu, k_pack) and of *_results_of (the host walks), on the calls of tests/deliver_cases.py -- scan tiles
crossed, truncated and empty captures at a tile's edges, an empty tile, rows without bytes between rows with bytes -- with MPDU buffers that are exactly full, one
byte short, cut inside the second tile, 16 bytes and absent, and guard patterns behind everything the caller offered.

The truth per distinct capture is the CPU model's of the handle's parity tests (deliver_cases.truth); test_the_truth_* hold it to the transmitted bytes, to the
frames the captures were built to yield and to a lone call of the eight captures.  For the 40 MHz handle the front-end model and the transmitted PSDUs are the
truth; the bytes and FCS word of its one frame whose FCS fails are not known to either and are taken from that lone call (results_of)."""
import ctypes

import numpy as np
import pytest

import deliver_cases as dc
import deliver_model as dm

capi = None                                                 # sora_amd.capi, once the sora fixture has imported it

pytestmark = pytest.mark.gpu
GUARD = 0xA5
PRE = {"11a": "sora_rx", "11b": "sora_rx11b", "11n": "sora_rx11n", "ht40": "sora_ht40"}
# what the 802.11b / 802.11n rows report: position, verdict, rate, length, FCS word, flags (sora_hip.h); the other fields are 0
REPORTED = ("end_sample", "error_code", "rate_kbps", "length", "crc32", "flags", "mpdu")


@pytest.fixture(scope="module")
def sora():
    import sora_amd
    if sora_amd.device_count() <= 0:
        pytest.skip("no HIP device")
    global capi
    from sora_amd import capi
    return sora_amd


_worlds = {}


class World:
    """one handle's base captures on the device side of things: the captures, their truth, and the means to run a call of them"""
    def __init__(self, sora, oracle, handle):
        self.sora, self.handle, self.L = sora, handle, sora.load()
        self.base = dc.BUILD[handle](sora)
        self.truth = dc.truth(self.base, oracle)
        if handle in ("11b", "11n"):
            self.truth = {k: [{f: r.get(f, 0) for f in REPORTED} for r in fr] for k, fr in self.truth.items()}
        self.lone, rx, _, _ = self.run(list(range(8)), 8)
        rx.close()
        if handle == "ht40":                                 # (module docstring) the decoded bytes of the frame whose FCS fails
            got = [r for r in self.lone if r["capture_id"] == dc.capture_id(dc.CRC)]
            ev = [e for e in self.truth[dc.CRC] if e["streams"]]
            assert len(got) == 2 and len(ev) == 1
            for s, r in zip(ev[0]["streams"], got):
                s["mpdu"], s["crc32"] = r["mpdu"], r["crc32"]

    def open(self, kinds, mf):
        sora, b = self.sora, self.base
        n = int(sum(b.length(k) for k in kinds))
        if self.handle == "11a":
            rx = sora.Rx(len(kinds), n, sample_rate_mhz=40, max_frames_per_capture=mf)
        elif self.handle == "11b":
            rx = sora.Rx11b(len(kinds), n, max_frames_per_capture=mf)
            assert rx.set_preamble(1) == 0
        elif self.handle == "11n":
            rx = sora.Rx11n(len(kinds), n, max_frames_per_capture=mf)
        else:
            import ht40_front_model as fm
            frames = soft = 0
            for k in kinds:
                for e in self.truth[int(k)]:
                    if e["streams"]:
                        frames += 1; soft += 2 * (e["nsym"] * 108 * fm.MCS2[e["rate_kbps"]][0] + 64)
            rx = sora.RxHt40(frames + 16, soft + 4096)
        return rx

    def process(self, rx, d_iq, descs, mf):
        if self.handle == "11a" or self.handle == "11b":
            return rx.process_dev(d_iq, descs)
        if self.handle == "11n":
            return rx.process_dev(d_iq[0], d_iq[1], descs)
        return rx.process_captures_dev(d_iq[0], d_iq[1], descs, max_frames_per_capture=mf)

    def upload(self, kinds):
        import torch
        iq, descs = dc.tile(self.base, kinds)
        d = tuple(torch.from_numpy(x).cuda() for x in iq) if self.base.chains == 2 else torch.from_numpy(iq).cuda()
        return d, descs

    def min_rows(self, ncaps, mf):
        """the least max_rows the header lets *_deliver_async take for such a call"""
        return ncaps * mf * (2 if self.handle == "ht40" else 1)

    def run(self, kinds, mf):
        """a call through the wrapper's results() -> (rows as dicts, rx, ticket, device buffers)"""
        d, descs = self.upload(kinds)
        rx = self.open(kinds, mf)
        t = self.process(rx, d, descs, mf)
        rows = rx.results(ticket=t)
        return rows, rx, t, d

    def model(self, kinds, mf):
        return dc.model_captures(self.handle, self.truth, kinds, mf)

    # ---- the C entry points, with max_rows and mpdu_cap of the test's choosing
    def deliver(self, rx, t, buf, max_rows, mpdu_cap):
        """mpdu_cap None: h_mpdu NULL"""
        return getattr(self.L, PRE[self.handle] + "_deliver_async")(rx._h, int(t), buf.rows.ctypes.data, max_rows, buf.counts.ctypes.data,
                                                                    buf.mpdu.ctypes.data if mpdu_cap is not None else None, mpdu_cap or 0)

    def results_of(self, rx, t, max_out, mpdu_cap, room=None):
        """-> (rc, nout, rows (ROW_DTYPE, all `room` of them), mpdu bytes (all of the allocation)); both pre-filled with the guard"""
        room = room if room is not None else max_out + 4
        rows = np.full(room * 36, GUARD, np.uint8)
        mp = np.full((mpdu_cap or 0) + 64, GUARD, np.uint8)
        n = ctypes.c_size_t(0)
        rc = getattr(self.L, PRE[self.handle] + "_results_of")(rx._h, int(t), ctypes.cast(rows.ctypes.data, ctypes.POINTER(capi.FrameResult)), max_out,
                                                               ctypes.byref(n), mp.ctypes.data if mpdu_cap is not None else None, mpdu_cap or 0)
        return rc, n.value, rows.view(capi.ROW_DTYPE), mp


def world(sora, oracle, handle):
    if handle not in _worlds:
        _worlds[handle] = World(sora, oracle, handle)
    return _worlds[handle]


def row_array(sora, rows):
    a = np.zeros(len(rows), capi.ROW_DTYPE)
    for f in dm.FIELDS:
        a[f] = np.array([r[f] for r in rows], np.int64).astype(a.dtype[f]) if rows else []
    return a


def same_rows(sora, got, want, what):
    """got: rows of the caller's OWN memory -- a copy, never a view of a page-locked buffer: when an assertion below fails, pytest prints this function's arguments
    after the test's `finally` has given that buffer back"""
    want = row_array(sora, want)
    assert len(got) == len(want), (what, len(got), len(want))
    for f in dm.FIELDS:
        bad = np.flatnonzero(got[f] != want[f])
        assert not len(bad), "%s: row %d of %d, %s: %r, the model says %r" % (what, bad[0], len(want), f, got[f][bad[0]], want[f][bad[0]])


def count_bytes(buf):
    """all 64 bytes of the allocation the counts lie in"""
    return np.ctypeslib.as_array((ctypes.c_uint8 * 64).from_address(buf.counts.ctypes.data))


def guard_fill(buf):
    buf.rows.view(np.uint8)[:] = GUARD
    count_bytes(buf)[:] = GUARD
    if buf.mpdu is not None:
        buf.mpdu[:] = GUARD


def untouched(a):
    return bool((np.asarray(a).view(np.uint8) == GUARD).all())


# ---- the truth ------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("handle", dc.HANDLES)
def test_the_truth_is_what_was_sent_and_what_a_lone_call_reports(sora, oracle, handle):
    w = world(sora, oracle, handle)
    spec = dc.spec(handle)
    for k in range(8):
        fr = w.truth[k]
        if handle == "ht40":
            flat = [(s["error_code"], s["length"], s["mpdu"]) for e in fr for s in (e["streams"] or [{"error_code": e["error_code"], "length": 0, "mpdu": None}])]
            assert [(e, n) for e, n, _ in flat] == [x for x in spec[k] for _ in range(1 if x[0] == dm.E_PLCP_HEADER_FAIL else 2)], (dc.NAMES[k], flat)
            sent = [p for pair in w.base.sent[k] for p in pair]
        else:
            flat = [(r["error_code"], r["length"], r["mpdu"]) for r in fr]
            assert [(e, n) for e, n, _ in flat] == spec[k], (dc.NAMES[k], [(hex(e), n) for e, n, _ in flat])
            sent = w.base.sent[k]
        if k in (dc.ONE, dc.TWO, dc.FOUR, dc.LARGEST):
            # (the 802.11b frame sink gives its verdict with three FCS bytes in hand, as the reference's does: the row's last byte is not the frame's)
            known = slice(None, -1) if handle == "11b" else slice(None)
            assert [m[known] for _, _, m in flat] == [dc._fcs(p)[known] for p in sent], dc.NAMES[k]
        if k == dc.CRC:
            assert all(m != dc._fcs(p) and len(m) == len(p) + 4 for (_, _, m), p in zip(flat, sent))
    want = dm.results_of(w.model(list(range(8)), 8), 64, 1 << 20)
    assert len(w.lone) == want["nout"]
    for g, r in zip(w.lone, want["rows"]):
        assert {f: g[f] for f in dm.FIELDS} == r, (g, r)
        n = dm.owned(r)
        assert g["mpdu"][:n] == want["mpdu"][r["mpdu_offset"]:r["mpdu_offset"] + n]


# ---- *_deliver_async and *_results_of of the handles that deliver dense MPDUs -----------------------------------------------------------------------------------------
def caps_of(want):
    """the MPDU buffer sizes of the issue: exactly full; one byte short (only the last MPDU is left out); a cut inside the second tile of rows (every later MPDU is
    left out); 16; none"""
    total = want["counts"][1]
    out = [total, total - 1]
    rows = want["rows"]
    if len(rows) > dc.TILE + 8:
        out.append(rows[dc.TILE + 8]["mpdu_offset"] + 1)
    return [c for c in dict.fromkeys(out + [16]) if c > 0] + [None]


def check_delivery(w, rx, t, caps, ncaps, mf, name):
    sora = w.sora
    full = dm.deliver(caps, 1 << 32)
    total = full["counts"][1]
    max_rows = w.min_rows(ncaps, mf)
    buf = sora.HostResults(max_rows + 8, total + 4096)
    try:
        assert len(full["rows"]) <= max_rows
        for cap in caps_of(full):
            want = dm.deliver(caps, cap)
            what = "%s %s, mpdu_cap %s" % (w.handle, name, cap)
            guard_fill(buf)
            assert w.deliver(rx, t, buf, max_rows, cap) == 0, (what, w.L.sora_hip_last_error())
            rx.wait(t)
            assert [int(v) for v in buf.counts[:2]] == want["counts"], what
            same_rows(sora, buf.rows[:want["counts"][0]].copy(), want["rows"], what)
            if cap is not None:
                got = buf.mpdu[:len(want["mpdu"])]
                bad = np.flatnonzero(got != np.frombuffer(want["mpdu"], np.uint8))
                assert not len(bad), "%s: MPDU byte %d of %d" % (what, bad[0], len(want["mpdu"]))
                if cap == total - 1:
                    assert sum(want["present"]) == sum(full["present"]) - 1 and not want["present"][max(i for i, p in enumerate(full["present"]) if p)]
                if cap not in (total, total - 1, 16):
                    assert 0 < sum(want["present"]) < sum(full["present"]) - 1
            assert untouched(buf.rows[max_rows:]) and untouched(count_bytes(buf)[8:]), what
            assert untouched(buf.mpdu[cap or 0:]), what
        # one row less than the header demands: refused, nothing enqueued, the buffers as they were
        guard_fill(buf)
        assert w.deliver(rx, t, buf, max_rows - 1, total) == dm.ERR_CAPACITY
        rx.wait(t)
        assert untouched(buf.rows) and untouched(count_bytes(buf)) and untouched(buf.mpdu)
    finally:
        buf.close()
    return full


def check_results_of(w, rx, t, caps, name):
    full = dm.deliver(caps, 1 << 32)
    nrows, total = full["counts"]
    for max_out, cap in ((nrows, total), (nrows, None)):
        want = dm.results_of(caps, max_out, cap)
        rc, nout, rows, mp = w.results_of(rx, t, max_out, cap)
        what = "%s %s results_of(%d, %s)" % (w.handle, name, max_out, cap)
        assert (rc, nout) == (want["rc"], want["nout"]), what
        same_rows(w.sora, rows[:nout], want["rows"], what)
        assert untouched(rows[max_out:]) and untouched(mp[cap or 0:]), what
        assert bytes(mp[:len(want["mpdu"])]) == want["mpdu"], what


DENSE = ("11b", "11n", "ht40")


@pytest.mark.parametrize("name", [c.name for c in dc.cases()])
@pytest.mark.parametrize("handle", DENSE)
def test_delivery_equals_the_contract(sora, oracle, handle, name):
    w = world(sora, oracle, handle)
    case = dc.by_name(name)
    dc.check_coverage(handle, case)
    d, descs = w.upload(case.kinds)
    rx = w.open(case.kinds, case.mf)
    try:
        t = w.process(rx, d, descs, case.mf)
        caps = w.model(case.kinds, case.mf)
        full = check_delivery(w, rx, t, caps, len(case.kinds), case.mf, name)
        assert tuple(full["counts"]) == dc.totals(handle, case)
        check_results_of(w, rx, t, caps, name)
    finally:
        rx.close()


@pytest.mark.parametrize("handle", ("11b", "11n"))
def test_results_of_with_a_buffer_one_short(sora, oracle, handle):
    """max_out one short: the first max_out rows, SORA_ERR_CAPACITY.  mpdu_cap one short: every row, the last MPDU skipped, SORA_ERR_CAPACITY.  mpdu_cap cut inside
    the table: offsets count copied bytes only, and a later MPDU that still fits is copied."""
    w = world(sora, oracle, handle)
    case = dc.by_name("mixed_1025")
    d, descs = w.upload(case.kinds)
    rx = w.open(case.kinds, case.mf)
    try:
        t = w.process(rx, d, descs, case.mf)
        caps = w.model(case.kinds, case.mf)
        nrows, total = dm.deliver(caps, None)["counts"]
        for max_out, cap in ((nrows - 1, total), (nrows, total - 1), (nrows, 100), (1, 16)):
            want = dm.results_of(caps, max_out, cap)
            rc, nout, rows, mp = w.results_of(rx, t, max_out, cap)
            what = "%s results_of(%d, %d)" % (handle, max_out, cap)
            assert (rc, nout) == (dm.ERR_CAPACITY, want["nout"]) and want["rc"] == dm.ERR_CAPACITY, what
            same_rows(sora, rows[:nout], want["rows"], what)
            assert untouched(rows[max_out:]) and untouched(mp[cap:]) and bytes(mp[:len(want["mpdu"])]) == want["mpdu"], what
    finally:
        rx.close()


@pytest.mark.parametrize("handle", DENSE)
def test_two_calls_in_flight_share_nothing_but_the_handle(sora, oracle, handle):
    """a 2049-capture call and a 1-capture call behind it, both in flight, delivered into different buffers: the second table carries nothing of the first"""
    w = world(sora, oracle, handle)
    big, small = dc.by_name("truncated_then_empty_mf3"), dc.by_name("single")
    d1, descs1 = w.upload(big.kinds)
    d2, descs2 = w.upload(small.kinds)
    rx = w.open(big.kinds, 3)
    if handle == "11n":                                      # (the 802.11n handle keeps one call in flight unless told otherwise)
        rx.set_depth(2)
    b1 = sora.HostResults(w.min_rows(2049, 3) + 8, 1 << 20); b2 = sora.HostResults(w.min_rows(1, 3) + 8, 4096)
    try:
        guard_fill(b1); guard_fill(b2)
        t1 = w.process(rx, d1, descs1, 3)
        assert w.deliver(rx, t1, b1, w.min_rows(2049, 3), 1 << 19) == 0
        t2 = w.process(rx, d2, descs2, 3)
        assert w.deliver(rx, t2, b2, w.min_rows(1, 3), 1024) == 0
        rx.wait(t2); rx.wait(t1)
        for buf, case, cap in ((b1, big, 1 << 19), (b2, small, 1024)):
            want = dm.deliver(w.model(case.kinds, 3), cap)
            assert [int(v) for v in buf.counts[:2]] == want["counts"], case
            same_rows(sora, buf.rows[:want["counts"][0]].copy(), want["rows"], "%s %s in flight" % (handle, case))
            assert bytes(buf.mpdu[:len(want["mpdu"])]) == want["mpdu"] and want["counts"][1] == len(want["mpdu"])
            assert untouched(buf.mpdu[cap:]) and untouched(buf.rows[w.min_rows(len(case.kinds), 3):])
    finally:
        b1.close(); b2.close(); rx.close()


# ---- the 40 MHz descriptor form ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("joint", [False, True])
@pytest.mark.parametrize("nframes", dc.HT40_DESC_FRAMES)
def test_ht40_descriptor_calls_cross_the_scan_tiles(sora, nframes, joint):
    """frames of the shortest data field (one symbol), three distinct ones over and over under frame ids out of order: a host template, no per-frame counts"""
    import torch
    import tx_ht40_model as T
    rng = np.random.default_rng(4105 + joint)
    gain = 250.0 * 128.0 / T.A
    lens = (1, 2, 5)
    mp = [[rng.integers(0, 256, n, dtype=np.uint8).tobytes() for _ in range(1 if joint else 2)] for n in lens]
    if joint:
        o0, o1, off = sora.tx_ht40_joint([m[0] for m in mp], [14] * 3, gaps=[64] * 3)
        nsym = [sora.ht40_symbols_joint(n + 4, 6, 2) for n in lens]
    else:
        o0, o1, off = sora.tx_ht40([m[0] for m in mp], [m[1] for m in mp], [14] * 3, gaps=[64] * 3)
        nsym = [sora.ht40_symbols(n + 4, n + 4, 6, 2) for n in lens]
    assert nsym == [1, 1, 1]
    scale = lambda o: torch.clamp(torch.round(torch.cat([o, torch.zeros_like(o[:256])]).double() * gain), -32768, 32767).to(torch.int16)
    which = [(5 * i + i // 7) % 3 for i in range(nframes)]
    descs = [(off[k] + 64 + 1280, 6, 2, lens[k] + 4, 0 if joint else lens[k] + 4, 0, 0.0, dc.capture_id(i)) for i, k in enumerate(which)]
    rx = sora.RxHt40(nframes, nframes * 2 * (108 * 6 + 64))
    per = 1 if joint else 2
    try:
        if joint:
            rx.set_coding(sora.HT40_CODING_JOINT)
        t = rx.process_dev(scale(o0), scale(o1), descs, None)
        stream = lambda p: {"error_code": dm.E_FRAME_OK, "length": len(p) + 4, "crc32": int.from_bytes(dc._fcs(p)[-4:], "little"), "mpdu": dc._fcs(p)}
        caps = dm.ht40_descriptor_call([(dc.capture_id(i), 62, 1, [stream(p) for p in mp[k]]) for i, k in enumerate(which)], joint)
        w = World.__new__(World); w.sora, w.handle, w.L = sora, "ht40", sora.load()
        w.min_rows = lambda ncaps, mf: ncaps * per          # what the descriptor form needs: two rows per frame, one in joint coding
        full = check_delivery(w, rx, t, caps, nframes, 1, "descriptors %d joint %d" % (nframes, joint))
        assert full["counts"] == [per * nframes, per * sum(lens[k] + 4 for k in which)]
        rc, nout, rows, mpd = w.results_of(rx, t, per * nframes, full["counts"][1])
        assert (rc, nout) == (0, per * nframes)
        same_rows(sora, rows[:nout], full["rows"], "descriptors results_of")
        assert bytes(mpd[:len(full["mpdu"])]) == full["mpdu"] and untouched(mpd[len(full["mpdu"]):]) and untouched(rows[nout:])
    finally:
        rx.close()


# ---- the 802.11a handle: rows point into the handle's own MPDU array --------------------------------------------------------------------------------------------------
def check_11a(w, rx, t, case, buf, bound=False):
    sora = w.sora
    kinds, mf = case.kinds, case.mf
    caps = w.model(kinds, mf)
    nslots = [dm.slots_11a(w.base.length(int(k)) // 2) for k in kinds]
    need = rx.mpdu_bytes(t)
    max_rows = len(kinds) * mf
    want = dm.deliver_11a(caps, nslots, max_rows, need)
    assert want["rc"] == 0 and want["mpdu_bytes"] == need, (want["mpdu_bytes"], need)
    if not bound:
        guard_fill(buf)
    else:
        buf.rows.view(np.uint8)[:] = GUARD; count_bytes(buf)[:] = GUARD
    what = "11a %s bound %d" % (case, bound)
    assert w.deliver(rx, t, buf, max_rows, need) == 0, what
    rx.wait(t)
    assert int(buf.nrows[0]) == want["nrows"], what
    same_rows(sora, buf.rows[:want["nrows"]].copy(), want["rows"], what)
    for off, data in want["mpdus"]:
        assert bytes(buf.mpdu[off:off + len(data)]) == data, (what, off)
    assert untouched(buf.rows[max_rows:]) and untouched(buf.mpdu[need:]) and untouched(count_bytes(buf)[4:]), what
    if bound:                                               # words no frame owns are left as they were
        own = np.zeros(need, bool)
        for r in want["rows"]:
            if dm.owned(r):
                own[r["mpdu_offset"]:(r["mpdu_offset"] + r["nsym"] * 32)] = True
        assert (buf.mpdu[:need][~own] == GUARD).all(), what
    return want, need, max_rows


@pytest.mark.parametrize("name", [c.name for c in dc.cases()])
def test_11a_delivery_equals_the_contract(sora, oracle, name):
    w = world(sora, oracle, "11a")
    case = dc.by_name(name)
    dc.check_coverage("11a", case)
    d, descs = w.upload(case.kinds)
    rx = w.open(case.kinds, case.mf)
    buf = None
    try:
        t = w.process(rx, d, descs, case.mf)
        buf = sora.HostResults(len(case.kinds) * case.mf + 8, rx.mpdu_bytes(t) + 4096)
        want, need, max_rows = check_11a(w, rx, t, case, buf)
        assert (want["nrows"], sum(len(m) for _, m in want["mpdus"])) == dc.totals("11a", case)
        if want["nrows"] > 1:                                # at most max_rows rows are copied; the count is the call's
            guard_fill(buf)
            assert w.deliver(rx, t, buf, want["nrows"] - 1, need) == 0
            rx.wait(t)
            assert int(buf.nrows[0]) == want["nrows"] and untouched(buf.rows[want["nrows"] - 1:])
            same_rows(sora, buf.rows[:want["nrows"] - 1].copy(), want["rows"][:-1], "11a %s, a row less" % name)
        guard_fill(buf)                                      # an h_mpdu smaller than the handle's array: refused before anything is enqueued
        assert w.deliver(rx, t, buf, max_rows, need - 1) == dm.ERR_CAPACITY
        rx.wait(t)
        assert untouched(buf.rows) and untouched(count_bytes(buf)) and untouched(buf.mpdu)
        caps = w.model(case.kinds, case.mf)
        check_results_of(w, rx, t, caps, name)
    finally:
        if buf is not None:
            buf.close()
        rx.close()


def test_11a_results_with_buffers_one_short_device_rows_and_bound_delivery(sora, oracle):
    """1025 captures: sora_rx_results with max_out and mpdu_cap one short against the model's error form; sora_rx_results_dev's packed rows through the row codec;
    sora_rx_deliver_async behind sora_rx_bind_mpdu"""
    from sora_amd.shard import results_from_rows
    w = world(sora, oracle, "11a")
    case = dc.by_name("mixed_1025")
    d, descs = w.upload(case.kinds)
    rx = w.open(case.kinds, case.mf)
    rx.set_depth(2)
    buf = None
    try:
        t = w.process(rx, d, descs, case.mf)
        caps = w.model(case.kinds, case.mf)
        nslots = [dm.slots_11a(w.base.length(int(k)) // 2) for k in case.kinds]
        nrows, total = dm.deliver(caps, None)["counts"]
        for max_out, cap in ((nrows - 1, total), (nrows, total - 1)):
            want = dm.results_of(caps, max_out, cap)
            rows = np.full((max_out + 4) * 36, GUARD, np.uint8); mp = np.full(cap + 64, GUARD, np.uint8); n = ctypes.c_size_t(0)
            rc = w.L.sora_rx_results(rx._h, ctypes.cast(rows.ctypes.data, ctypes.POINTER(capi.FrameResult)), max_out, ctypes.byref(n), mp.ctypes.data, cap)
            assert (rc, n.value) == (dm.ERR_CAPACITY, want["nout"]) and want["rc"] == dm.ERR_CAPACITY
            same_rows(sora, rows.view(capi.ROW_DTYPE)[:n.value], want["rows"], "sora_rx_results(%d, %d)" % (max_out, cap))
            assert untouched(rows[36 * max_out:]) and untouched(mp[cap:]) and bytes(mp[:len(want["mpdu"])]) == want["mpdu"]
        want = dm.deliver_11a(caps, nslots, nrows)
        drows, dn, mpdu_ptr = rx.results_dev(ticket=t)
        rx.wait(t)
        assert int(dn.item()) == nrows and mpdu_ptr
        packed = drows[:nrows].cpu().numpy()
        same_rows(sora, np.ascontiguousarray(packed).view(capi.ROW_DTYPE).reshape(-1), want["rows"], "results_dev")
        for g, r in zip(results_from_rows(packed), want["rows"]):
            assert all(g[f] == r[f] for f in dm.FIELDS if f in g), (g, r)
        buf = sora.HostResults(len(case.kinds) * case.mf + 8, rx.mpdu_bytes(t) + 4096)
        check_11a(w, rx, t, case, buf)
        guard_fill(buf)
        rx.bind_mpdu(buf)
        tb = w.process(rx, d, descs, case.mf)
        check_11a(w, rx, tb, case, buf, bound=True)
    finally:
        if buf is not None:
            buf.close()
        rx.close()


def test_11a_two_calls_in_flight_share_nothing_but_the_handle(sora, oracle):
    w = world(sora, oracle, "11a")
    big, small = dc.by_name("truncated_then_empty_mf3"), dc.by_name("single")
    d1, descs1 = w.upload(big.kinds)
    d2, descs2 = w.upload(small.kinds)
    rx = w.open(big.kinds, 3)
    rx.set_depth(2)
    b1 = b2 = None
    try:
        t1 = w.process(rx, d1, descs1, 3)
        b1 = sora.HostResults(2049 * 3 + 8, rx.mpdu_bytes(t1) + 64)
        guard_fill(b1)
        assert w.deliver(rx, t1, b1, 2049 * 3, rx.mpdu_bytes(t1)) == 0
        t2 = w.process(rx, d2, descs2, 3)
        b2 = sora.HostResults(3 + 8, rx.mpdu_bytes(t2) + 64)
        guard_fill(b2)
        assert w.deliver(rx, t2, b2, 3, rx.mpdu_bytes(t2)) == 0
        rx.wait(t2); rx.wait(t1)
        for buf, case, t in ((b1, big, t1), (b2, small, t2)):
            nslots = [dm.slots_11a(w.base.length(int(k)) // 2) for k in case.kinds]
            want = dm.deliver_11a(w.model(case.kinds, 3), nslots, len(case.kinds) * 3, rx.mpdu_bytes(t))
            assert want["rc"] == 0 and int(buf.nrows[0]) == want["nrows"]
            same_rows(sora, buf.rows[:want["nrows"]].copy(), want["rows"], "11a %s in flight" % case)
            for off, data in want["mpdus"]:
                assert bytes(buf.mpdu[off:off + len(data)]) == data
            assert untouched(buf.mpdu[rx.mpdu_bytes(t):]) and untouched(buf.rows[len(case.kinds) * 3:])
    finally:
        for b in (b1, b2):
            if b is not None:
                b.close()
        rx.close()
