"""tests/ht40_mcs15_model.py alone, without a GPU: each of its models equals the existing one with the option off (gate 14, rates 0..2); with no noise through the
identity channel it decodes its own rate 5/6 frames FRAME_OK in both codings and both guard intervals, from the data field alone and through its front end with the
gate at 15; and the three definitions it extends inside `with rate56():` are what they were outside it."""
import numpy as np
import pytest

from oracle import ht40_data_model as dm
from oracle import py_ht40 as m
import ht40_front_captures as fc
import ht40_front_gi_model as fg
import ht40_front_model as fm
import ht40_gi_cases as C
import ht40_gi_model as G
import ht40_mcs15_model as M

FIELDS = ("a20", "mcs", "ht_len", "nsym", "cfo", "end_sample", "error_code", "S")


def test_rate56_extends_three_definitions_and_puts_them_back():
    before = (m.ndbps, m.puncture, m.MCS2)
    with M.rate56():
        assert m.ndbps(6, 3) == 540 and m.ndbps(1, 3) == 90 and m.MCS2[15] == (6, 3)
        assert [m.ndbps(nb, cr) for nb in (1, 2, 4, 6) for cr in range(3)] == [before[0](nb, cr) for nb in (1, 2, 4, 6) for cr in range(3)]
        a = np.arange(30, dtype=np.uint8); b = 100 + a
        assert list(m.puncture(a, b, 3)[:12]) == [0, 100, 1, 102, 3, 104, 5, 105, 6, 107, 8, 109]          # A1 B1 A2 B3 A4 B5
        for cr in range(3):
            assert np.array_equal(m.puncture(a, b, cr), before[1](a, b, cr))
        assert m.nsym_for([100, 90], 6, 3) == 2 and {k: v for k, v in m.MCS2.items() if k != 15} == before[2]
    assert (m.ndbps, m.puncture, m.MCS2) == before and 15 not in m.MCS2
    with pytest.raises(IndexError):
        m.ndbps(6, 3)


@pytest.mark.parametrize("joint", [False, True], ids=["per-stream", "joint"])
def test_front_model_with_the_gate_at_14_is_the_existing_one(joint):
    caps = fc.build(joint, full=False)
    assert any(c.name == "gate mcs15" for c in caps) and len(caps) >= 40
    n = 0
    for c in caps:
        own = fm.front(c.iq[0], c.iq[1], flags=fm.OWN | (fm.JOINT if joint else 0))
        for guard in (False, True):
            got = M.front(c.iq[0], c.iq[1], mcs_max=14, guard=guard, joint=joint)
            assert got == fg.front(c.iq[0], c.iq[1], guard=guard, joint=joint), (c.name, guard)
        got = M.front(c.iq[0], c.iq[1], mcs_max=14, joint=joint)
        assert [[e[f] for f in FIELDS] for e in got] == [[e[f] for f in FIELDS] for e in own], c.name
        n += len(got)
        # the gate at 15 changes the one capture whose HT-SIG says MCS 15, and that one into a recorded frame of one symbol
        at15 = M.front(c.iq[0], c.iq[1], mcs_max=15, joint=joint)
        if c.name == "gate mcs15":
            assert got[0]["error_code"] == fm.E_PLCP_HEADER_FAIL and (at15[0]["error_code"], at15[0]["mcs"], at15[0]["ht_len"], at15[0]["nsym"]) == (0, 15, 60, 1)
        else:
            assert at15 == got, c.name
    assert n > len(caps) // 2


def test_data_field_model_at_rates_0_to_2_is_the_existing_one():
    rng = np.random.default_rng(15)
    for joint in (False, True):
        for nb, cr, nsym, gi in ((1, 2, 2, 0), (2, 0, 2, 1), (6, 1, 1, 1), (4, 2, 3, 0)):
            lens = C.lengths(rng, nb, cr, nsym, joint, 1)
            seg, ps = C.frame(rng, nb, cr, lens, gi, joint, 6.0, 37)
            w = dm.zf_weights(seg, 0, 37)
            a = M.model(seg, 0, nb, cr, lens[0] if joint else lens, 37, w, gi=gi, joint=joint)
            b = G.model(seg, 0, nb, cr, lens[0] if joint else lens, 37, w, gi=gi, joint=joint)
            assert a.nsym == b.nsym and np.array_equal(a.theta, b.theta)
            assert [(s.error_code, s.crc32, s.psdu) for s in a.streams] == [(s.error_code, s.crc32, s.psdu) for s in b.streams]
            assert all(s.error_code == 1 for s in a.streams) and [s.psdu for s in a.streams] == ps


@pytest.mark.parametrize("joint", [False, True], ids=["per-stream", "joint"])
@pytest.mark.parametrize("gi", [0, 1], ids=["long", "short"])
def test_model_decodes_its_own_rate_56_frames(joint, gi):
    rng = np.random.default_rng(150 + 2 * joint + gi)
    for nb, nsym in ((6, 1), (6, 2), (6, 12), (1, 1), (1, 12), (2, 2), (4, 3)):
        with M.rate56():
            lens = C.lengths(rng, nb, 3, nsym, joint, nsym & 1)
            assert C.symbols(lens, nb, 3, joint) == nsym
            seg, ps = C.frame(rng, nb, 3, lens, gi, joint, 0.0, 0)
        assert seg.shape[1] == 320 + (144 if gi else 160) * nsym
        r = M.model(seg, 0, nb, 3, lens[0] if joint else lens, 0, dm.zf_weights(seg, 0, 0), gi=gi, joint=joint)
        assert r.nsym == nsym and all(s.error_code == 1 for s in r.streams) and [s.psdu for s in r.streams] == ps, (nb, nsym)


@pytest.mark.parametrize("joint", [False, True], ids=["per-stream", "joint"])
def test_whole_mcs15_frames_through_the_front_model_and_the_data_field_model(joint):
    """identity channel, no noise: the front end at gate 15 records the frame with HT-SIG's fields, its translated record decodes FRAME_OK; at gate 14 it is a header failure"""
    rng = np.random.default_rng(1515 + joint)
    for L in (4 + joint, 64, 65, 700):
        with M.rate56():
            x, nsym, ps = fc.frame(rng, 15, L, joint)
        pair = fc.each(fc.whole, fc.cat(fc.quiet(400), fc.through(x, fc.H_UNIT), fc.quiet(600)))
        ev = M.front(pair[0], pair[1], mcs_max=15, joint=joint)
        assert len(ev) == 1 and (ev[0]["error_code"], ev[0]["mcs"], ev[0]["ht_len"], ev[0]["nsym"]) == (0, 15, L, nsym), (L, ev)
        assert nsym == -(-(22 + 8 * L) // (1080 if joint else 540))
        low = M.front(pair[0], pair[1], mcs_max=14, joint=joint)
        assert len(low) == 1 and low[0]["error_code"] == fm.E_PLCP_HEADER_FAIL and low[0]["mcs"] == 0
        d = M.descriptor(0, ev[0], 0.0, joint, 7)
        assert d[1:5] == (6, 3, L, 0 if joint else L)
        iq = np.stack(pair)
        r = M.model(iq, d[0], 6, 3, L if joint else (L, L), d[5], dm.zf_weights(iq, d[0], d[5]), joint=joint)
        assert all(s.error_code == 1 for s in r.streams) and [s.psdu for s in r.streams] == ps, L
