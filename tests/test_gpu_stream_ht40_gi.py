"""Stream continuation of the 40 MHz HT handle in SORA_HT40_GUARD_SIGNALLED (k_scan_ht40_stream_gi): a two-chain stream that holds short-GI and
long-GI frames, handed to sora_ht40_process_captures_dev in pieces, must yield the rows, the MPDUs and the final resume point of the same stream handed over in one
call -- and the rows the handle reports on it with stream mode off.  The cuts: inside a frame's legacy preamble, inside a frame's HT-SIG, in the middle of a short
frame's data field (the frame is saved and found by the next call), and just behind a short frame's extent at a point its LONG extent would pass (the frame is taken
in that call because it is short).  Both codings; the frames are tests/ht40_gi_captures.py's, the positions of the cuts come from tests/ht40_front_gi_model.py."""
import numpy as np
import pytest

import ht40_front_captures as fc
import ht40_front_gi_model as fg
import ht40_gi_captures as gc
from level_captures import whole

pytestmark = pytest.mark.gpu
FRAME_OK, ROW_SHORT_GI = 1, 4
KEY = ("error_code", "rate_kbps", "stream", "length", "crc32", "end_sample", "flags", "nsym", "mpdu")
FRAMES = [(9, 80, 1), (12, 120, 0), (10, 100, 1), (13, 400, 1), (11, 260, 1), (14, 90, 0), (8, 60, 1)]        # (mcs, PSDU bytes, kind)


@pytest.fixture(scope="module")
def env():
    import torch
    import sora_amd
    if sora_amd.device_count() <= 0:
        pytest.skip("no HIP device")
    return torch, sora_amd


def _stream(joint, oracle):
    """-> (iq int16 [2, n, 2], first samples of the frames, psdus, the model's events on the whole)"""
    rng = np.random.default_rng(8200 + joint)
    parts, starts, sent, pos = [], [], [], 0
    for mcs, ln, gi in FRAMES:
        lead = int(rng.integers(300, 900))
        x, nsym, ps = gc.frame(rng, mcs, ln, gi, joint, oracle=oracle)
        parts += [fc.quiet(lead), fc.through(x, cfo_step=21.0)]
        starts.append(pos + lead); sent.append(ps); pos += lead + x.shape[1]
    pair = fc.each(whole, fc.gauss(fc.cat(*parts, fc.quiet(28 * 40)), rng, 8.0))
    ev = fg.front(pair[0], pair[1], guard=True, joint=joint)
    return np.stack(pair), starts, sent, ev


def _call(env, rx, piece, mf=8):
    torch, _ = env
    t = rx.process_captures_dev(torch.from_numpy(piece[0].copy()).cuda(), torch.from_numpy(piece[1].copy()).cuda(), [(0, piece.shape[1], 0)], max_frames_per_capture=mf)
    return t, rx.results(ticket=t)


def _key(r, base=0):
    return tuple(r[f] + base if f == "end_sample" else r[f] for f in KEY)


@pytest.mark.parametrize("joint", [0, 1], ids=["per_stream", "joint"])
def test_a_stream_of_short_and_long_frames_in_pieces_is_the_one_call_result(env, oracle, joint):
    torch, sora = env
    iq, starts, sent, ev = _stream(joint, oracle)
    n = iq.shape[1]
    assert [(e["error_code"], e["short_gi"]) for e in ev] == [(0, gi) for _, _, gi in FRAMES]
    short_end = lambda e: 2 * (e["a20"] + 240 + 72 * e["nsym"]); long_end = lambda e: 2 * (e["a20"] + 240 + 80 * e["nsym"])
    up28 = lambda v: -(-v // 28) * 28
    cuts = [up28(starts[1] + 400),                                        # inside frame 1's legacy preamble
            up28(starts[2] + 900),                                        # inside frame 2's HT-SIG
            up28(starts[3] + 1600 + 72 * ev[3]["nsym"]),                  # the middle of frame 3's data field: a short frame that runs past the piece
            up28(short_end(ev[4]) + 16)]                                  # behind frame 4's short extent, in front of the end of its long one
    assert starts[3] + 1600 < cuts[2] < short_end(ev[3]) and short_end(ev[4]) + 16 <= cuts[3] < long_end(ev[4]) and cuts == sorted(cuts) and cuts[-1] < starts[5]
    arrivals = cuts + [n]

    def handle(stream_mode):
        rx = sora.RxHt40(32, 1 << 21)
        rx.set_coding(joint); assert rx.set_guard(1) == 0
        if stream_mode:
            assert rx.set_stream_mode(1) == 0
        return rx

    # ---- the yardsticks: stream mode off, and stream mode on in one call
    rx = handle(False); _, off_rows = _call(env, rx, iq); rx.close()
    rx = handle(True); t, one_rows = _call(env, rx, iq); one_used = int(rx.stream_consumed(t, 1)[0]); rx.close()
    jpf = 1 if joint else 2
    assert [_key(r) for r in one_rows] == [_key(r) for r in off_rows] and len(one_rows) == jpf * len(FRAMES)
    for i, (mcs, ln, gi) in enumerate(FRAMES):
        for s in range(jpf):
            r = one_rows[jpf * i + s]
            assert (r["error_code"], r["rate_kbps"], r["stream"], r["flags"], r["mpdu"]) == (FRAME_OK, mcs, s, ROW_SHORT_GI if gi else 0, sent[i][s]), (i, s, hex(r["error_code"]))
    # ---- in pieces
    rx = handle(True)
    base, got, per_call = 0, [], []
    for a in arrivals:
        assert (a - base) % 28 == 0 and a > base
        t, rows = _call(env, rx, iq[:, base:a])
        got += [_key(r, base) for r in rows]; per_call.append(len(rows) // jpf)
        used = int(rx.stream_consumed(t, 1)[0])
        assert used % 28 == 0 and all(r["end_sample"] <= used for r in rows)
        base += used
    rx.close()
    assert got == [_key(r) for r in one_rows]
    assert base == one_used
    # frame 3 was saved by the call that ended inside it and found by the next; frame 4 was taken by the call that ended just behind its short extent
    assert per_call == [1, 1, 1, 2, 2], per_call
