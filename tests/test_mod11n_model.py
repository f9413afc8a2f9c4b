"""tests/mod11n_model.py, the per-brick numpy model of the 802.11n 2x2 modulation graphs, pinned without a GPU: its composition equals the recorded output of
the reference modulator sample for sample (tests/golden/refgraph_11n.npz, refmod_11n_mcs11_14.npz) and, where oracle/_ref is built, the compiled one."""
import os

import numpy as np
import pytest

import mod11n_model as M
from mod11a_model import PILOT_SGN
from test_tx11n_cpu import sweep_lengths

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def same(got, want, what):
    for ch in (0, 1):
        g, w = np.asarray(got[ch], np.int16), np.asarray(want[ch], np.int16)
        assert g.shape == w.shape, (what, ch, g.shape, w.shape)
        bad = np.flatnonzero((g != w).any(axis=1))
        assert len(bad) == 0, (what, ch, bad[:8])


def test_tables_are_the_bricks():
    assert len(M.PILOT_SIGN) == 127 and np.array_equal(M.PILOT_SIGN, 1 - 2 * PILOT_SGN[:127].astype(int))   # _b_dot11_pilot.h:37-43 = pilot.hpp:10-28
    for n in range(4):                                                           # _pilot[n][iss] is Psi_iss rotated by n
        assert np.array_equal(M.PILOT[n][0], np.roll([1, 1, -1, -1], -n)) and np.array_equal(M.PILOT[n][1], np.roll([1, -1, -1, 1], -n))
    for nb in (1, 2, 4, 6):
        for iss in (0, 1):
            r = M.interleave_targets(nb, iss)
            assert sorted(r[:52 * nb]) == list(range(52 * nb))                   # a permutation of the symbol's bits ...
    assert [len(M.interleave_targets(nb, 0)) for nb in (1, 2, 4, 6)] == [56, 104, 208, 312]
    assert list(M.interleave_targets(1, 0)[52:]) == [4, 8, 12, 16]               # ... and, for BPSK, four more onto positions that are taken


def test_parser_and_interleaver_keep_every_bit():
    rng = np.random.default_rng(1)
    for nb in (1, 2, 4, 6):
        x = rng.integers(0, 256, (5, 13 * nb)).astype(np.uint8)
        a, b = M.stream_parse(x, nb)
        assert a.shape == b.shape == (5, M.row_bytes(nb))
        bits = np.unpackbits(x, axis=1, bitorder="little")
        s = max(nb // 2, 1)
        k = np.arange(104 * nb)
        for iss, o in enumerate((a, b)):                                         # 802.11n 20.3.11.7.2: blocks of s bits alternate between the streams
            ob = np.unpackbits(o, axis=1, bitorder="little")
            assert np.array_equal(ob[:, :52 * nb], bits[:, (k // s) % 2 == iss])
            assert not ob[:, 52 * nb:].any()                                     # BPSK: the seventh byte's upper half is 0
            il = M.interleave(o, nb, iss)
            assert np.array_equal(np.unpackbits(il, axis=1).sum(1), np.unpackbits(o, axis=1).sum(1))


def test_compose_equals_the_recorded_reference_frames():
    z = np.load(os.path.join(GOLD, "refgraph_11n.npz"))
    for k, mcs in enumerate((8, 9, 10, 12)):
        same(M.compose(z["mpdu%d" % k].tobytes(), mcs), (z["tx%d_0" % k], z["tx%d_1" % k]), ("refgraph_11n", k, mcs))
    y = np.load(os.path.join(GOLD, "refmod_11n_mcs11_14.npz"))
    for mcs in (9, 11, 12, 13, 14):
        if "tx%d_0" % mcs in y.files:
            same(M.compose(y["mpdu%d" % mcs].tobytes(), mcs), (y["tx%d_0" % mcs], y["tx%d_1" % mcs]), ("refmod_11n_mcs11_14", mcs))
    assert all("tx%d_0" % mcs in y.files for mcs in (11, 13, 14))


@pytest.mark.parametrize("mcs", range(8, 15))
def test_compose_equals_the_compiled_reference_modulator(mcs):
    from oracle.pyoracle import ReferenceGraph
    g = ReferenceGraph()
    if not g.available():
        pytest.skip("oracle/_ref/libsora_refgraph.so not built (needs the reference tree)")
    for ln in sweep_lengths(mcs):
        mp = bytes(np.random.default_rng([mcs, ln]).integers(0, 256, ln).astype(np.uint8))
        same(M.compose(mp, mcs), g.tx11n(mp, mcs), (mcs, ln))
