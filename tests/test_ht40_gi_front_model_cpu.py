"""tests/cxx/ht40_front_gi_model.c (the 40 MHz HT front end with a guard flag) held to tests/ht40_front_model.py without a GPU: with the flag
off it returns that model's records field for field over every capture of tests/ht40_front_captures.py, in both codings; with the flag on, on those captures -- whose
HT-SIG bit 31 is clear -- likewise.  And, with the flag on, a short-GI frame's record: the same header and position, the extent of 240 + 72 nsym kept samples."""
import numpy as np
import pytest

import ht40_front_captures as C
import ht40_front_gi_model as fg
import ht40_front_model as fm
import tx_ht40_gi_model as TG
from level_captures import whole

FIELDS = ("a20", "mcs", "ht_len", "nsym", "cfo", "end_sample", "error_code", "S")


@pytest.mark.parametrize("joint", [False, True], ids=["per_stream", "joint"])
def test_without_short_frames_it_is_the_existing_front_model(joint):
    caps = C.build(joint=joint, full=True)
    nev = 0
    for c in caps:
        want = fm.front(c.iq[0], c.iq[1], flags=fm.OWN | (fm.JOINT if joint else 0))
        for guard in (False, True):
            got = fg.front(c.iq[0], c.iq[1], guard=guard, joint=joint)
            assert [{f: e[f] for f in FIELDS} for e in got] == want, (c.name, guard)
            assert not any(e["short_gi"] for e in got), (c.name, guard)
        nev += len(want)
    assert nev > len(caps) // 2


def _short_capture(oracle, rng, mcs, ln, joint, lead, tail):
    mp = [rng.integers(0, 256, ln, dtype=np.uint8).tobytes() for _ in range(1 if joint else 2)]
    fr = TG.frame_int_nofcs(mp[0] if joint else mp, mcs, 1, joint=joint, oracle=oracle)
    x = (fr[..., 0].astype(float) + 1j * fr[..., 1].astype(float)) * (128.0 / TG.T.A)
    pair = C.cat(C.quiet(lead), C.through(x), C.quiet(tail))
    return C.each(whole, C.gauss(pair, rng, 8.0))


@pytest.mark.parametrize("joint", [False, True], ids=["per_stream", "joint"])
def test_a_short_frame_is_an_event_over_its_short_extent(oracle, joint):
    rng = np.random.default_rng(31 + joint)
    pair = _short_capture(oracle, rng, 11, 150, joint, 404, 600)
    off = fg.front(pair[0], pair[1], guard=False, joint=joint)
    on = fg.front(pair[0], pair[1], guard=True, joint=joint)
    assert len(off) == len(on) == 1 and off[0]["error_code"] == on[0]["error_code"] == 0
    assert (off[0]["short_gi"], on[0]["short_gi"]) == (0, 1)
    for f in ("a20", "mcs", "ht_len", "nsym", "cfo", "S"):
        assert off[0][f] == on[0][f], f
    a, n = on[0]["a20"], on[0]["nsym"]
    src = lambda end20: 2 * min(14 * ((end20 - 1) // 14 + 1), len(pair[0]) // 2)          # the source call that brings the frame's last kept sample
    assert on[0]["end_sample"] == src(a + 240 + 72 * n) and off[0]["end_sample"] == src(a + 240 + 80 * n) and n >= 3
    assert fg.found(on[0])["mcs"] == 11 | 0x100 and fg.found(off[0])["mcs"] == 11
    # cut behind the short extent's last sample: still an event with the flag on, none with it off; one source call earlier: none
    end = 2 * (a + 240 + 72 * n); end += -end % 28
    cut = C.each(lambda c: c[:end], pair)
    assert len(fg.front(cut[0], cut[1], guard=True, joint=joint)) == 1 and fg.front(cut[0], cut[1], guard=False, joint=joint) == []
    early = C.each(lambda c: c[:end - 28], pair)
    assert fg.front(early[0], early[1], guard=True, joint=joint) == []
