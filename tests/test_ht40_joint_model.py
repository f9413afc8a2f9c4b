"""The joint coding of the 40 MHz HT pair, the parts that need no GPU: the test-side models of tests/ht40_joint_model.py held to each other
and to what exists -- the stream parser is a bijection; the integer receive model (oracle/ht40_data_model.py's per-stream soft bytes, de-parsed, the oracle's
T11aViterbi<.., 192, 36> and its sink) recovers what the float model of the format sends through a 2x2 channel; the integer frame is the float frame within the
transform's rounding, and its preamble is the per-stream integer frame's."""
import numpy as np
import pytest

from oracle import ht40_data_model as dm
from oracle import py_ht40 as m
import ht40_joint_model as J
import tx_ht40_model as T
from test_tx_ht40_cpu import LIMIT_LSB

FRAME_OK = 1
H0 = np.array([[1.0 * np.exp(0.3j), 0.35 * np.exp(-1.1j)], [0.3 * np.exp(2.0j), 0.9 * np.exp(-0.4j)]])     # tests/test_gpu_ht40_soft.py's channel


def _psdu(rng, length):
    return m.add_fcs(rng.integers(0, 256, length - 4, dtype=np.uint8).tobytes())


@pytest.mark.parametrize("nb", [1, 2, 4, 6])
def test_parser_map_is_a_bijection_onto_both_streams(nb):
    iss, k = J.parser_map(nb)
    ncb = 108 * nb
    assert len(iss) == 2 * ncb and set(iss) == {0, 1}
    flat = iss * ncb + k
    assert sorted(flat) == list(range(2 * ncb))
    s = max(1, nb // 2)                                                   # the rule as the 20 MHz transmitter states it: blocks of s bits alternate between the streams
    for kc in (0, s - 1, s, 2 * s - 1, 2 * s, 2 * ncb - 1):
        assert (iss[kc], k[kc]) == ((kc // s) & 1, (kc // (2 * s)) * s + kc % s)
    # de-parsing what was parsed gives the symbol back
    sym = np.arange(3 * 2 * ncb) % 251
    st = [np.zeros(3 * ncb, np.int64), np.zeros(3 * ncb, np.int64)]
    for d in range(3):
        for s_ in range(2):
            st[s_][d * ncb + k[iss == s_]] = sym[d * 2 * ncb:(d + 1) * 2 * ncb][iss == s_]
    assert np.array_equal(J.deparse(st[0], st[1], nb), sym)


def test_symbol_counts():
    assert J.nsym_for(4000, 1, 0) == 297 and 297 * 216 == 64152           # the largest decoder job
    assert J.nsym_for(4000, 6, 1) * J.ndbps(6, 1) == 32832                # the largest bit field (MCS 13)
    for mcs, (nb, cr) in m.MCS2.items():
        for ln in (4, 5, 37, 200, 1504, 4000):
            n = J.nsym_for(ln, nb, cr)
            assert (n - 1) * J.ndbps(nb, cr) < 22 + 8 * ln <= n * J.ndbps(nb, cr)


CASES = [(mcs, ln) for mcs in range(8, 15) for ln in (5, 37, 200, 1504)] + [(8, 4000), (13, 4000), (14, 4000)]


@pytest.mark.parametrize("mcs,length", CASES)
def test_integer_receive_model_recovers_what_the_float_model_sends(mcs, length):
    nb, cr = m.MCS2[mcs]
    rng = np.random.default_rng(100 * mcs + length)
    psdu = _psdu(rng, length)
    x, nsym = J.tx_joint(psdu, nb, cr, seed=int(rng.integers(1, 128)))
    assert nsym == J.nsym_for(length, nb, cr) and x.shape == (2, (2 + nsym) * 160)
    iq = m.channel(x, H0, 6.0, rng)
    r = J.rx_model(iq, 0, nb, cr, length, 0, dm.zf_weights(iq, 0, 0))
    assert r.nsym == nsym and r.soft.shape == (nsym * 216 * nb,)
    assert r.error_code == FRAME_OK, (mcs, length, hex(r.error_code))
    assert r.psdu == psdu, (mcs, length)


@pytest.mark.parametrize("mcs", range(8, 15))
def test_integer_frame_against_the_float_frame_and_the_per_stream_preamble(oracle, mcs):
    """|frame_int_joint - tx_frame_joint x A / 128| within the project's limit for the transform's rounding (LIMIT_LSB of tests/test_tx_ht40_cpu.py: the
    constellation points are the same); the first 1280 samples equal frame_int's for the same MCS, LENGTH and N_SYM"""
    nb, cr = m.MCS2[mcs]
    for ln in (5, 200, 1500):
        rng = np.random.default_rng(2000 * mcs + ln)
        psdu = _psdu(rng, ln)
        xi, nsym, pre = J.frame_int_joint(psdu, mcs, oracle=oracle)
        xf, nsym_f, pre_f = J.tx_frame_joint(psdu, mcs)
        assert (nsym, pre) == (nsym_f, pre_f) and pre == 1280 and xi.shape == (2, xf.shape[1], 2) and xi.shape[1] == 1280 + 160 * (2 + nsym)
        xf = xf * T.A / 128.0
        d = max(np.abs(xi[..., 0] - xf.real).max(), np.abs(xi[..., 1] - xf.imag).max())
        print("joint integer frame vs float frame: MCS %d len %d nsym %d worst %.2f LSB" % (mcs, ln, nsym, d))
        assert d <= LIMIT_LSB, (mcs, ln, d)
        # a per-stream frame of the same LENGTH has the same HT-SIG; the same N_SYM gives the same L-SIG.  Its preamble comes from its own symbol count, so compare
        # against preamble bins made for (mcs, LENGTH, nsym) through the same transform
        P = T.preamble_bins(mcs, ln, nsym)
        f = lambda b: T.ifft128(b, oracle)
        stf, ltf = f(P["stf"]), f(P["lltf"])
        want = np.concatenate([np.tile(stf, (3, 1))[:320], ltf[-64:], ltf, ltf, T._cp(f(P["lsig"])), T._cp(f(P["htsig0"])), T._cp(f(P["htsig1"])), np.tile(stf, (2, 1))[:160]])
        assert np.array_equal(xi[0, :1280], want) and np.array_equal(xi[1, :1280], want)
    # ... and literally frame_int's first 1280 samples, where a per-stream frame of the same MCS and LENGTH has the same N_SYM too: LENGTH 4 (one symbol in both
    # codings at every MCS) and the longest LENGTH whose per-stream frame is one symbol
    for ln in sorted({4, (m.ndbps(nb, cr) - 22) // 8}):
        psdu = _psdu(np.random.default_rng(mcs + ln), ln)
        xi, nsym, _ = J.frame_int_joint(psdu, mcs, oracle=oracle)
        xp, nsym_p, _ = T.frame_int([psdu, psdu], mcs, oracle=oracle)
        assert nsym == nsym_p == 1
        assert np.array_equal(xi[:, :1280], xp[:, :1280]), (mcs, ln)
