"""The oracle's stage functions behind the oldest stage entry points -- so_lts, so_sym_front, so_sym_track, so_demap, so_deinterleave -- and the thin 802.11n rows
(demap11n, sig_demap11n, siso_est11n, mimo_est11n) against the REFERENCE's own bricks on the families of tests/stage_edge_cases.py: rails, zeros, nulled bins, the
carrier-offset sum past 2^31, symbol_count past 126, the demap clamp edges, channels singular on some carriers only.  0 LSB everywhere.

  live      (skipped without oracle/_ref): every case of every family, context and state after each call included, against ref_11a_lts, ref_11a_sym_front,
            ref_11a_pilot_track, ref_11a_deinterleave (oracle/ref_graph_shim.cpp), the demap primitives of oracle/ref_shim.cpp and the existing ref_11n_* shims
  recorded  (always): the subset stored in tests/golden/ref_vectors_11a_stages.npz (tests/golden/make_ref_vectors_11a_stages.py)
  coverage  (always): that the families reach the branches they are there for, worked out from the inputs in int64 numpy and from the recorded reference output,
            never from the code under test.

CFO_est: the reference's arctangent table (intalglut.h) holds nothing below -32686, so T11aLTS's estimate (>> 6) spans -511 .. 511; -512 cannot come out of it."""
import os

import numpy as np
import pytest

import stage_edge_cases as sc
from oracle.pyoracle import Oracle, Reference, ReferenceGraph

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_vectors_11a_stages.npz")


@pytest.fixture(scope="module")
def o():
    return Oracle()


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


@pytest.fixture(scope="module")
def ref():
    g = ReferenceGraph(); r = Reference()
    if not (g.available() and r.available()):
        pytest.skip("oracle/_ref not built (needs the reference tree)")
    assert g.has_11a_bricks(), "oracle/_ref/libsora_refgraph.so predates the ref_11a_* shims: rebuild it"
    return g, r


@pytest.fixture(scope="module")
def lts(o):
    names, x = sc.lts_cases(o)
    rec, post = sc.run_lts(sc.Engine(o), x)
    return names, x, rec, post


@pytest.fixture(scope="module")
def frames(o):
    return sc.track_frames(o)


def _rows(a, b):
    return np.argwhere((a != b).reshape(len(a), -1).any(1)).ravel()[:8].tolist()


# ---------------------------------------------------------------------------------------------- live
def test_live_lts(o, ref, lts):
    names, x, rec, post = lts
    want, wpost = sc.run_lts(sc.Engine(o, ref[0]), x)
    assert np.array_equal(rec, want), [names[i] for i in _rows(rec, want)]
    assert np.array_equal(post, wpost) and not post.any()


def test_live_sym_front(o, ref, lts):
    x = sc.symfront_symbols(); cr = np.concatenate([lts[2], sc.random_ctx_records()]); idx = sc.symfront_index(len(x), len(cr))
    got = sc.run_symfront(sc.Engine(o), x, cr, idx); want = sc.run_symfront(sc.Engine(o, ref[0]), x, cr, idx)
    assert np.array_equal(got, want), _rows(got, want)
    assert not got[:, 28:36].any() and got.any()


def test_live_sym_track(o, ref, frames):
    got = sc.run_track(sc.Engine(o), frames); want = sc.run_track(sc.Engine(o, ref[0]), frames)
    assert np.array_equal(got[0], want[0]), _rows(got[0], want[0])            # every tracked symbol
    assert np.array_equal(got[1], want[1]), _rows(got[1], want[1])            # the whole state record after every symbol
    assert np.array_equal(got[2], want[2]), _rows(got[2], want[2])


def test_live_demap_deinterleave(o, ref):
    g, r = ref
    x = sc.demap_symbols()
    for nb in (1, 2, 4, 6):
        for i in range(len(x)):
            assert np.array_equal(o.demap(nb, x[i]), r.demap(nb, x[i])), (nb, i)
        s = sc.deint_bytes(nb)
        for i in range(len(s)):
            assert np.array_equal(o.deinterleave(nb, s[i]), g.deinterleave11a(nb, s[i])), (nb, i)
        perm = o.deinterleave(nb, s[0]).astype(int) | (o.deinterleave(nb, s[1]).astype(int) << 8)      # the permutation itself, through two byte planes
        assert sorted(perm.tolist()) == list(range(48 * nb))


def test_live_11n_rows(o, ref):
    g, _ = ref
    x = sc.demap11n_symbols()
    for nb in (1, 2, 4, 6):
        for i in range(len(x)):
            assert np.array_equal(o.demap11n(nb, x[i]), g.demap11n(nb, x[i])), (nb, i)
    for i, s in enumerate(sc.sig_demap11n_symbols()):
        assert np.array_equal(o.sig_demap11n(s), g.sig_demap11n(s)), i
    for i, (a, b) in enumerate(zip(*sc.siso_est11n_lltfs())):
        assert np.array_equal(o.siso_est11n(a, b), g.siso_est11n(a, b)), i
    for i, (a, b) in enumerate(zip(*sc.mimo_est11n_ltfs())):
        h, hi = o.mimo_est11n(a, b); rh, rhi = g.mimo_est11n(a, b)
        assert np.array_equal(h, rh) and np.array_equal(hi, rhi), i


# ---------------------------------------------------------------------------------------------- recorded
@pytest.fixture(scope="module")
def mine(o):
    return sc.recorded_vectors(o, sc.Engine(o), sc.cpu_functions(o))


def test_recorded_seeds_and_keys(gold, mine):
    assert np.array_equal(gold["seeds"], sc.SEEDS) and set(gold.files) == set(mine)
    assert os.path.getsize(GOLD) <= 512 * 1024


def test_recorded_lts(gold, mine, lts):
    assert np.array_equal(mine["lts_rec"], gold["lts_rec"]), [lts[0][i] for i in _rows(mine["lts_rec"], gold["lts_rec"])]
    assert np.array_equal(mine["lts_post"], gold["lts_post"])


def test_recorded_sym_front(gold, mine):
    assert np.array_equal(mine["sym_eq"], gold["sym_eq"]), _rows(mine["sym_eq"], gold["sym_eq"])


def test_recorded_sym_track(gold, mine):
    assert np.array_equal(mine["trk_out"], gold["trk_out"]), _rows(mine["trk_out"], gold["trk_out"])
    assert np.array_equal(mine["trk_end"], gold["trk_end"]), _rows(mine["trk_end"], gold["trk_end"])


def test_recorded_demap_deinterleave(gold, mine):
    for nb in (1, 2, 4, 6):
        for k in ("demap_%d" % nb, "deint_%d" % nb):
            assert np.array_equal(mine[k], gold[k]), (k, _rows(mine[k], gold[k]))


def test_recorded_11n_rows(gold, mine):
    for k in ["demap11n_%d" % nb for nb in (1, 2, 4, 6)] + ["sig_demap11n", "siso_ch", "mimo_h", "mimo_hinv"]:
        assert np.array_equal(mine[k], gold[k]), (k, _rows(mine[k], gold[k]))


# ---------------------------------------------------------------------------------------------- coverage
def test_coverage_lts_family(o, gold, lts):
    names, x = lts[0], lts[1]
    assert len(x) > max(sc.LTS_ROWS)
    re, im = sc.lts_sums(x)                                                    # exact 64-term sums
    beyond = (re < -2 ** 31) | (re >= 2 ** 31) | (im < -2 ** 31) | (im >= 2 ** 31)
    assert beyond.sum() >= 2 and names[int(np.argmax(beyond))] == "const-", [names[i] for i in np.flatnonzero(beyond)]
    assert (np.abs(re) >= 2 ** 31 - 2 ** 24).sum() + (np.abs(im) >= 2 ** 31 - 2 ** 24).sum() >= 8      # and several within half a percent of the wrap
    # the angle of the wrapped sums on both sides of +-pi, within the last step of CFO_est (pi / 512)
    ang = np.arctan2(sc.wrap32(im).astype(np.float64), sc.wrap32(re).astype(np.float64))
    assert (ang > np.pi * (1 - 1 / 512)).any() and (ang < -np.pi * (1 - 1 / 512)).any() and (np.abs(ang) < 0.01).any()
    # what the reference itself estimated: the ends of the range its table allows, both signs, many values
    lut = o.uatan2_lut().astype(int)
    cfo = gold["lts_rec"][:, 0].astype(int)
    assert (int(lut.min()) >> 6, int(lut.max()) >> 6) == (-511, 511)
    assert cfo.min() == -511 and cfo.max() == 511 and (cfo < 0).sum() > 10 and (cfo > 0).sum() > 10 and len(set(cfo.tolist())) > 40
    assert cfo[names.index("const-")] == 511 and cfo[names.index("const+")] == 0
    # zero channel coefficients per frame (of the 56 bins T11aLTS writes): all, none and a mixture
    chan = gold["lts_rec"][:, 130:].reshape(-1, 64, 2)
    assert not chan[:, 28:36].any()
    zeros = set(((chan == 0).all(-1).sum(1) - 8).tolist())
    assert 56 in zeros and 0 in zeros and len([z for z in zeros if 0 < z < 56]) >= 5, sorted(zeros)


def test_coverage_tracker_family(frames):
    nsym = frames["nsym"].tolist(); c0 = [sc.start_count(s) for s in frames["state0"]]
    assert set(nsym) == set(sc.TRACK_NSYM)
    wraps = [sc.count_wraps(c, n) for c, n in zip(c0, nsym)]
    assert max(wraps) >= 2 and sum(w >= 2 for w in wraps) >= 5 and wraps.count(1) >= 5 and wraps.count(0) >= 5
    for c in sc.START_COUNTS:
        assert any(a == c and n > 0 for a, n in zip(c0, nsym)), c
    order = np.lexsort((frames["first"] + frames["nsym"], frames["first"])); first = frames["first"][order]; end = first + frames["nsym"][order]
    assert (np.diff(frames["first"]) < 0).any() and (first[1:] > end[:-1]).any() and (first[1:] >= end[:-1]).all()     # unsorted, gaps, no overlap
    assert (frames["state0"][:, 6:] == -32768).any(1).sum() > 20
    for k in ("zero", "pilots"):
        f = frames["kind"].index(k) + len(sc.TRACK_NSYM) - 1
        e = frames["eq"][frames["first"][f]:frames["first"][f] + frames["nsym"][f]]
        assert len(e) == 300 and not np.delete(e, sc.PILOTS, axis=1).any() and (k == "zero") == (not e.any())


def test_coverage_demap_family():
    x = sc.demap_symbols()[:, sc.DATA48].astype(int) >> 4                       # what demap_limit clamps, on the carriers that are demapped
    for v in (-130, -129, -128, -127, 126, 127, 128, 129):                      # both clamp edges from both sides, in re and in im
        assert (x[..., 0] == v).any() and (x[..., 1] == v).any(), v
    assert x.min() == -2048 and x.max() == 2047
    assert max(sc.DEMAP_ROWS) == len(sc.demap_symbols())


def test_coverage_mimo_family():
    l0, l1 = sc.mimo_est11n_ltfs()
    sing = sc.mimo_singular_carriers(l0, l1).tolist()
    assert len({s for s in sing if 1 <= s <= 55}) >= 4 and 64 in sing and 0 in sing, sing
    assert (np.abs(l0).reshape(len(l0), -1).max(1) <= 3).sum() >= 15
