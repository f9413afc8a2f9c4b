"""tests/deliver_model.py against a table written out by hand, and tests/deliver_cases.py's named calls against closed forms: the model the GPU delivery is held
to (tests/test_gpu_deliver.py) is not checked only by itself, and no case can lose what it is for."""
import numpy as np
import pytest

import deliver_cases as dc
import deliver_model as dm

OK, CRC, HDR = dm.E_FRAME_OK, dm.E_CRC32_FAIL, dm.E_PLCP_HEADER_FAIL
A, B, C, D, E, F = b"A" * 10, b"B" * 7, b"C" * 3, b"D" * 5, b"E" * 4, b"F" * 1


def fr(err, length, mpdu=None, end=0, flags=0):
    return {"error_code": err, "length": length, "end_sample": end, "flags": flags, "mpdu": mpdu}


# six captures, ids out of order: two frames; nothing; a header failure between two frames; four frames at three rows (truncated; the fourth's bytes never count);
# nothing; one frame behind the short preamble whose header announces 5000 bytes (4096 are owned)
BIG = bytes(range(256)) * 16
TABLE = [(70, [fr(OK, 10, A, 100), fr(CRC, 7, B, 200)], 3),
         (3, [], 3),
         (41, [fr(OK, 3, C, 50), fr(HDR, 0, None, 60), fr(OK, 5, D, 70)], 3),
         (9, [fr(OK, 4, E, 10), fr(HDR, 9, None, 20), fr(OK, 1, F, 30), fr(OK, 10, A, 40)], 3),
         (8, [], 3),
         (5, [fr(OK, 5000, BIG + b"x" * 904, 999, flags=dm.ROW_SHORT_PREAMBLE)], 3)]
# (capture_id, end_sample, error_code, length, flags, mpdu_offset) of the nine rows
ROWS = [(70, 100, OK, 10, 0, 0), (70, 200, CRC, 7, 0, 10), (41, 50, OK, 3, 0, 17), (41, 60, HDR, 0, 0, 20), (41, 70, OK, 5, 0, 20),
        (9, 10, OK, 4, 0, 25), (9, 20, HDR, 9, 0, 29), (9, 30, OK, 1, dm.ROW_TRUNCATED, 29), (5, 999, OK, 5000, dm.ROW_SHORT_PREAMBLE, 30)]
DENSE = A + B + C + D + E + F + BIG                          # 30 + 4096 bytes


def key(r):
    return (r["capture_id"], r["end_sample"], r["error_code"], r["length"], r["flags"], r["mpdu_offset"])


def test_the_delivered_table_of_six_captures():
    got = dm.deliver(TABLE, 1 << 20)
    assert [key(r) for r in got["rows"]] == ROWS
    assert got["counts"] == [9, 4126] and got["mpdu"] == DENSE
    assert got["present"] == [True, True, True, False, True, True, False, True, True]
    assert all(r["start_sample"] == r["nsym"] == r["crc32"] == r["cfo_est"] == 0 for r in got["rows"])


def test_a_full_buffer_leaves_out_what_would_reach_past_it_and_nothing_else():
    exact = dm.deliver(TABLE, 4126)
    assert exact["mpdu"] == DENSE and exact["counts"] == [9, 4126]
    short = dm.deliver(TABLE, 4125)                          # only the last MPDU is left out
    assert [key(r) for r in short["rows"]] == ROWS and short["counts"] == [9, 4126]
    assert short["mpdu"] == DENSE[:30] and short["present"] == [True, True, True, False, True, True, False, True, False]
    cut = dm.deliver(TABLE, 19)                              # C would end at 20: it and everything behind it is left out; rows, offsets and the total stay
    assert [key(r) for r in cut["rows"]] == ROWS and cut["counts"] == [9, 4126]
    assert cut["mpdu"] == A + B and cut["present"] == [True, True] + [False] * 7
    edge = dm.deliver(TABLE, 20)                             # offset + len <= mpdu_cap: C fits exactly
    assert edge["mpdu"] == A + B + C and edge["present"][:5] == [True, True, True, False, False]
    none = dm.deliver(TABLE, None)                           # no MPDU buffer: the offsets and the total are the same
    assert [key(r) for r in none["rows"]] == ROWS and none["counts"] == [9, 4126] and none["mpdu"] == b"" and not any(none["present"])


def test_results_of_reports_the_same_rows_and_says_where_a_buffer_was_short():
    whole = dm.results_of(TABLE, 9, 4126)
    assert whole["rc"] == dm.OK and whole["nout"] == 9 and [key(r) for r in whole["rows"]] == ROWS and whole["mpdu"] == DENSE
    rows_short = dm.results_of(TABLE, 8, 4126)
    assert rows_short["rc"] == dm.ERR_CAPACITY and rows_short["nout"] == 8 and [key(r) for r in rows_short["rows"]] == ROWS[:8] and rows_short["mpdu"] == DENSE[:30]
    bytes_short = dm.results_of(TABLE, 9, 4125)
    assert bytes_short["rc"] == dm.ERR_CAPACITY and bytes_short["nout"] == 9 and [key(r) for r in bytes_short["rows"]] == ROWS and bytes_short["mpdu"] == DENSE[:30]
    # offsets count copied bytes only.  19 bytes: A and B fit, C, D and E do not and the rows behind them keep offset 17, F fits there.  16 bytes: B does not fit,
    # C moves up to 10, D and E do not fit, F lands at 13
    cut = dm.results_of(TABLE, 9, 19)
    assert cut["rc"] == dm.ERR_CAPACITY and cut["nout"] == 9
    assert [r["mpdu_offset"] for r in cut["rows"]] == [0, 10, 17, 17, 17, 17, 17, 17, 18] and cut["mpdu"] == A + B + F
    cut = dm.results_of(TABLE, 9, 16)
    assert [r["mpdu_offset"] for r in cut["rows"]] == [0, 10, 10, 13, 13, 13, 13, 13, 14] and cut["mpdu"] == A + C + F
    none = dm.results_of(TABLE, 9, None)                     # h_mpdu NULL: every offset is 0
    assert none["rc"] == dm.OK and [r["mpdu_offset"] for r in none["rows"]] == [0] * 9 and none["mpdu"] == b""
    assert [key(r)[:5] for r in none["rows"]] == [r[:5] for r in ROWS]


def test_more_frames_than_rows_flags_the_last_row_only_when_frames_were_lost():
    two = [fr(OK, 3, C), fr(OK, 5, D)]
    assert [r["flags"] for r in dm.deliver([(1, two, 2)], 64)["rows"]] == [0, 0]                      # found == mf: nothing lost
    assert [r["flags"] for r in dm.deliver([(1, two, 1)], 64)["rows"]] == [dm.ROW_TRUNCATED]
    assert dm.deliver([(1, two, 1)], 64)["counts"] == [1, 3]
    short = [fr(OK, 3, C, flags=dm.ROW_SHORT_PREAMBLE), fr(OK, 5, D)]
    assert [r["flags"] for r in dm.deliver([(1, short, 1)], 64)["rows"]] == [dm.ROW_TRUNCATED | dm.ROW_SHORT_PREAMBLE]


def test_the_80211a_form_indexes_the_handles_own_array():
    f = lambda err, length, mpdu, start: {"error_code": err, "length": length, "mpdu": mpdu, "start_sample": start}
    caps = [(7, [f(OK, 10, A, 16)], 2), (2, [], 2), (5, [f(HDR, 0, None, 0), f(OK, 7, B, 500), f(OK, 3, C, 900)], 2)]
    nsamples20 = [400, 14, 1200]
    nslots = [dm.slots_11a(n) for n in nsamples20]
    assert nslots == [6, 1, 16]
    got = dm.deliver_11a(caps, nslots, max_rows=4, mpdu_bytes=32 * 23)
    assert got["rc"] == dm.OK and got["nrows"] == 3 and got["mpdu_bytes"] == 32 * 23
    # slot of a frame: (start_sample + 144) // 80 -- 2, 1, 8; capture bases 0, 6, 7
    assert [(r["capture_id"], r["mpdu_offset"], r["flags"]) for r in got["rows"]] == [(7, 64, 0), (5, 256, 0), (5, 480, dm.ROW_TRUNCATED)]
    assert got["mpdus"] == [(64, A), (480, B)]
    assert dm.deliver_11a(caps, nslots, max_rows=4, mpdu_bytes=32 * 23 - 1) == {"rc": dm.ERR_CAPACITY}
    assert dm.deliver_11a(caps, nslots, max_rows=2)["rows"] == got["rows"][:2] and dm.deliver_11a(caps, nslots, max_rows=2)["nrows"] == 3


def test_the_40_mhz_forms():
    s = lambda err, length, mpdu: {"error_code": err, "length": length, "crc32": 5, "mpdu": mpdu}
    desc = dm.ht40_descriptor_call([(9, 41, 1, [s(OK, 3, C), s(CRC, 5, D)]), (4, 62, 2, [s(OK, 4, E), s(OK, 1, F)])])
    got = dm.deliver(desc, 64)
    assert [(r["capture_id"], r["start_sample"], r["rate_kbps"], r["nsym"], r["length"], r["mpdu_offset"], r["flags"]) for r in got["rows"]] == \
        [(9, 0, 41, 1, 3, 0, 0), (9, 1, 41, 1, 5, 3, 0), (4, 0, 62, 2, 4, 8, 0), (4, 1, 62, 2, 1, 12, 0)]
    assert got["counts"] == [4, 13] and got["mpdu"] == C + D + E + F
    joint = dm.deliver(dm.ht40_descriptor_call([(9, 41, 1, [s(OK, 3, C)]), (4, 62, 2, [s(OK, 4, E)])], joint=True), 64)
    assert [(r["capture_id"], r["start_sample"], r["mpdu_offset"]) for r in joint["rows"]] == [(9, 0, 0), (4, 0, 3)] and joint["counts"] == [2, 7]
    ev = lambda end, streams, mcs=9, nsym=1: {"end_sample": end, "error_code": 0 if streams else HDR, "rate_kbps": mcs, "nsym": nsym, "streams": streams}
    raw = dm.ht40_capture_call([(30, [ev(100, [s(OK, 3, C), s(OK, 5, D)]), ev(200, None), ev(300, [s(OK, 4, E), s(OK, 1, F)])], 2), (20, [], 2),
                                (10, [ev(50, None)], 2)])
    got = dm.deliver(raw, 64)
    assert [(r["capture_id"], r["start_sample"], r["end_sample"], r["error_code"], r["rate_kbps"], r["nsym"], r["length"], r["flags"], r["mpdu_offset"])
            for r in got["rows"]] == [(30, 0, 100, OK, 9, 1, 3, 0, 0), (30, 1, 100, OK, 9, 1, 5, 0, 3), (30, 0, 200, HDR, 0, 0, 0, dm.ROW_TRUNCATED, 8),
                                      (10, 0, 50, HDR, 0, 0, 0, 0, 8)]
    assert got["counts"] == [4, 8] and got["mpdu"] == C + D
    flagged = dm.deliver(dm.ht40_capture_call([(30, [ev(100, [s(OK, 3, C), s(OK, 5, D)]), ev(200, None)], 1)]), 64)
    assert [r["flags"] for r in flagged["rows"]] == [dm.ROW_TRUNCATED] * 2                             # both rows of the last event that has rows
    one = dm.deliver(dm.ht40_capture_call([(30, [ev(100, [s(OK, 3, C)])], 1)], joint=True), 64)
    assert [(r["start_sample"], r["flags"]) for r in one["rows"]] == [(0, 0)]


# ---- the named calls ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("handle", dc.HANDLES)
def test_every_named_call_covers_what_it_is_for(handle):
    names = [c.name for c in dc.cases()]
    assert len(set(names)) == len(names)
    assert {len(c.kinds) for c in dc.cases()} == set(dc.COUNTS)
    for c in dc.cases():
        dc.check_coverage(handle, c)
    assert {c.purpose for c in dc.cases()} == {"single", "truncated_last_lane", "truncated_first_lane", "empty_tile", "all_truncated", "mixed"}
    assert {c.mf for c in dc.cases() if c.purpose == "all_truncated"} == {1, 2}


def synthetic_truth(handle):
    """frames that have what SPEC says and nothing else, with bytes that tell the frames apart"""
    out = {}
    for k, frames in dc.spec(handle).items():
        out[k] = []
        for i, (err, length) in enumerate(frames):
            row = {"error_code": err, "length": length, "end_sample": 100 * (i + 1), "mpdu": bytes([16 * k + i]) * length if err != HDR else None}
            if handle == "ht40":
                row = {"end_sample": row["end_sample"], "error_code": 0 if err != HDR else err, "rate_kbps": 9, "nsym": 1,
                       "streams": None if err == HDR else [dict(row, crc32=s) for s in range(2)]}
            out[k].append(row)
    return out


# rows and bytes of every named call, worked out by hand from PAYLOAD: a one-frame capture is 5 or 44 bytes or a header failure; TWO is 37 + 65; FOUR is 11, 24, 13,
# 19; 40 MHz rows and bytes are twice that, but for header failures (one row)
CLOSED = {
    "single": (2, 102),
    "all_truncated_mf1": (1025, 1025 * 37), "all_truncated_mf2": (2 * 1023, 1023 * 35),
}


@pytest.mark.parametrize("handle", dc.HANDLES)
def test_totals_of_every_named_call_equal_the_closed_forms(handle):
    tr = synthetic_truth(handle)
    two = dc.ROWS_PER_FRAME[handle]
    for c in dc.cases():
        got = dm.deliver(dc.model_captures(handle, tr, c.kinds, c.mf), None)
        rows, nbytes = dc.totals(handle, c)
        assert got["counts"] == [rows, nbytes], (handle, c)
        ids = [r["capture_id"] for r in got["rows"]]
        assert len(set(ids)) > 1 or len(c.kinds) == 1
        if len(c.kinds) > 1:
            first = [ids.index(i) for i in dict.fromkeys(ids)]
            assert first == sorted(first) and ids != sorted(ids) and max(np.diff(sorted(set(ids)))) > 1      # call order; ids neither ascending nor contiguous
        if CLOSED.get(c.name):
            r, b = CLOSED[c.name]
            assert (rows, nbytes) == (two * r, two * b), (handle, c)
        if c.name.startswith(("truncated_then", "empty_then")):
            kinds = list(c.kinds)
            n1 = {k: kinds.count(k) for k in (dc.ONE, dc.HEADER, dc.CRC)}
            assert sum(n1.values()) == 2045 and kinds.count(dc.SILENCE) == 2
            t_rows, t_bytes = (3, 48) if c.mf == 3 else (1, 37)
            assert rows == two * (n1[dc.ONE] + n1[dc.CRC] + 2 * t_rows) + n1[dc.HEADER]
            assert nbytes == two * (5 * n1[dc.ONE] + 44 * n1[dc.CRC] + 2 * t_bytes)
    lg = dc.LARGEST_PAYLOAD[handle] + 4
    assert lg == {"11a": 2500, "11b": 4096, "11n": 1500, "ht40": 4000}[handle]
    m = dc.by_name("mixed_1025")
    kinds = list(m.kinds)
    per = {dc.ONE: (1, 5), dc.HEADER: (0, 0), dc.CRC: (1, 44), dc.TWO: (2, 102), dc.NOISE: (0, 0), dc.LARGEST: (1, lg)}
    assert dc.totals(handle, m) == (two * sum(per[k][0] * kinds.count(k) for k in per) + kinds.count(dc.HEADER), two * sum(per[k][1] * kinds.count(k) for k in per))


def test_tiling_gives_aligned_offsets_and_distinct_ids():
    base = dc.Base("11b", {k: np.full((28 * (k + 1), 2), k, np.int16) for k in range(8)}, {})
    kinds = [3, 0, 7, 7, 1]
    iq, descs = dc.tile(base, kinds)
    assert list(descs["nsamples"]) == [112, 28, 224, 224, 56] and list(descs["offset"]) == [0, 112, 140, 364, 588] and len(iq) == 644
    for d, k in zip(descs, kinds):
        assert (iq[int(d["offset"]):int(d["offset"]) + int(d["nsamples"])] == k).all()
    ids = [dc.capture_id(i) for i in range(3073)]
    assert len(set(ids)) == 3073 and ids != sorted(ids)
