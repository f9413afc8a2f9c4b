"""The integer models of the short guard interval held to the models that exist, without a GPU:
  * tests/tx_ht40_gi_model.py: kind 0 is tx_ht40_model / ht40_joint_model sample for sample; kind 1 differs from it exactly where the format says;
  * tests/ht40_gi_model.py: at the long guard interval it is oracle/ht40_data_model.model (soft bytes, theta, xs, streams); at the short one and cfo = 0 it is that model
    on the re-spaced frame; and a re-spaced short-GI loop-back frame decodes in the float64 receiver oracle/ht40_rx_f64.py too."""
import numpy as np
import pytest

from oracle import ht40_data_model as dm
from oracle import ht40_rx_f64 as rx64
from oracle import py_ht40 as m
import ht40_gi_model as G
import ht40_joint_model as J
import tx_ht40_gi_model as TG
import tx_ht40_model as T

GAIN = 250.0 * 128.0 / T.A                                              # the level of tests/test_gpu_tx_ht40.py's loop-back


def _psdus(rng, ln):
    return [m.add_fcs(rng.integers(0, 256, ln, dtype=np.uint8).tobytes()) for _ in range(2)]


@pytest.mark.parametrize("mcs", [8, 11, 14])
def test_kind_0_is_the_existing_transmit_models(oracle, mcs):
    rng = np.random.default_rng(mcs)
    ps = _psdus(rng, 77)
    a, na, la = TG.frame_int(ps, mcs, 0, (0x31, 0x62), oracle=oracle); b, nb_, lb = T.frame_int(ps, mcs, (0x31, 0x62), oracle=oracle)
    assert (na, la) == (nb_, lb) and np.array_equal(a, b)
    a, na, la = TG.frame_int(ps[0], mcs, 0, 0x47, joint=True, oracle=oracle); b, nb_, lb = J.frame_int_joint(ps[0], mcs, 0x47, oracle=oracle)
    assert (na, la) == (nb_, lb) and np.array_equal(a, b)


@pytest.mark.parametrize("joint", [False, True])
@pytest.mark.parametrize("mcs", [8, 10, 13])
def test_kind_1_differs_from_the_long_frame_where_the_format_says(oracle, mcs, joint):
    rng = np.random.default_rng(100 + mcs)
    ps = _psdus(rng, 140)
    arg = ps[0] if joint else ps
    long, nsym, ltf = TG.frame_int(arg, mcs, 0, joint=joint, oracle=oracle)
    short, ns, ls = TG.frame_int(arg, mcs, 1, joint=joint, oracle=oracle)
    assert (ns, ls) == (nsym, ltf) and short.shape == (2, 1600 + 144 * nsym, 2) and nsym >= 2
    same = np.ones(1600, bool); same[640:1120] = False                   # L-SIG and the two HT-SIG symbols
    assert np.array_equal(short[:, :1600][:, same], long[:, :1600][:, same])
    assert not np.array_equal(short[:, 800:1120], long[:, 800:1120])
    for d in range(nsym):
        s = short[:, 1600 + 144 * d:1600 + 144 * (d + 1)]
        assert np.array_equal(s[:, 16:], long[:, 1600 + 160 * d + 32:1600 + 160 * (d + 1)]), d
        assert np.array_equal(s[:, :16], s[:, 128:]), d                    # the prefix: the last 16 of the 128
    assert np.array_equal(TG.respace(short, nsym)[:, 1600:].reshape(2, nsym, 160, 2)[:, :, 32:], long[:, 1600:].reshape(2, nsym, 160, 2)[:, :, 32:])


def test_ht_sig_bits_differ_in_bit_31_and_the_crc_only():
    for mcs, ln in ((8, 4), (12, 1504), (14, 4000)):
        a, b = m.ht_sig_bits(mcs, ln), TG.ht_sig_bits(mcs, ln, 1)
        assert np.array_equal(TG.ht_sig_bits(mcs, ln, 0), a)
        diff = set(np.nonzero(a != b)[0].tolist())
        assert 31 in diff and diff - {31} and diff - {31} <= set(range(34, 42)), diff
        v = sum(int(x) << i for i, x in enumerate(b))
        crc = 0xFF
        for i in range(34):
            crc ^= (v >> i) & 1
            crc = (crc >> 1) ^ 0xE0 if crc & 1 else crc >> 1
        assert ((~crc) & 0xFF) == (v >> 34) & 0xFF and (v >> 42) == 0


def test_l_sig_length_counts_the_short_symbols_in_whole_4_us():
    assert [TG.l_length(n, 0) for n in (1, 9, 10, 11)] == [15, 39, 42, 45]
    assert [TG.l_length(n, 1) for n in (1, 9, 10, 11, 20, 593)] == [15, 39, 39, 42, 66, 12 + 3 * 534]


# ------------------------------------------------------------------ the data field
H0 = np.array([[1.0 * np.exp(0.3j), 0.35 * np.exp(-1.1j)], [0.3 * np.exp(2.0j), 0.9 * np.exp(-0.4j)]])


def _capture(rng, frame, sigma, cfo_step=0.0, lead=0, tail=0):
    """an integer transmit frame [2, n, 2] through H0 x GAIN, a carrier offset and noise -> int16 [2, lead + n + tail, 2]"""
    x = (frame[..., 0].astype(float) + 1j * frame[..., 1].astype(float)) * GAIN
    y = H0 @ x
    if cfo_step:
        y = y * np.exp(2j * np.pi * cfo_step / 65536.0 * np.arange(y.shape[1]))[None]
    y = np.concatenate([np.zeros((2, lead), complex), y, np.zeros((2, tail), complex)], axis=1)
    y = np.stack([y.real, y.imag], axis=-1) + sigma * rng.standard_normal(y.shape + (2,))
    return np.clip(np.rint(y), -32768, 32767).astype(np.int16)


@pytest.mark.parametrize("mcs,cfo", [(8, 0), (9, 13), (12, -7), (14, 40)])
def test_long_guard_interval_is_the_data_model(oracle, mcs, cfo):
    rng = np.random.default_rng(200 + mcs)
    nb, cr = m.MCS2[mcs]
    ps = _psdus(rng, 120)
    frame, nsym, ltf = T.frame_int(ps, mcs, oracle=oracle)
    iq = _capture(rng, frame, 2.0, cfo_step=-float(cfo), lead=5)
    off = 5 + ltf
    w = dm.zf_weights(iq, off, cfo)
    want = dm.model(iq, off, nb, cr, [len(ps[0]), len(ps[1])], cfo, w)
    got = G.model(iq, off, nb, cr, [len(ps[0]), len(ps[1])], cfo, w, gi=0)
    assert got.nsym == want.nsym == nsym
    assert np.array_equal(got.theta, want.theta) and np.array_equal(got.xs, want.xs)
    for s in range(2):
        assert np.array_equal(got.soft[s], want.soft[s]), s
        assert (got.streams[s].error_code, got.streams[s].crc32, got.streams[s].psdu) == (want.streams[s].error_code, want.streams[s].crc32, want.streams[s].psdu)
        assert got.streams[s].error_code == 1 and got.streams[s].psdu == ps[s]


@pytest.mark.parametrize("mcs", [8, 10, 11, 13, 14])
def test_short_guard_interval_at_cfo_0_is_the_data_model_on_the_respaced_frame(oracle, mcs):
    rng = np.random.default_rng(300 + mcs)
    nb, cr = m.MCS2[mcs]
    ps = _psdus(rng, 150)
    frame, nsym, ltf = TG.frame_int(ps, mcs, 1, oracle=oracle)
    iq = _capture(rng, frame, 6.0, lead=3, tail=40)
    off = 3 + ltf
    w = dm.zf_weights(iq, off, 0)
    wide = TG.respace(iq, nsym, off)
    assert np.array_equal(dm.zf_weights(wide, off, 0), w)
    want = dm.model(wide, off, nb, cr, [len(ps[0]), len(ps[1])], 0, w)
    got = G.model(iq, off, nb, cr, [len(ps[0]), len(ps[1])], 0, w, gi=1)
    assert np.array_equal(got.theta, want.theta) and np.array_equal(got.xs, want.xs)
    for s in range(2):
        assert np.array_equal(got.soft[s], want.soft[s]), s
        assert got.streams[s].error_code == want.streams[s].error_code == 1 and got.streams[s].psdu == want.streams[s].psdu == ps[s]


def test_joint_coding_is_the_joint_receive_model(oracle):
    rng = np.random.default_rng(41)
    nb, cr = m.MCS2[12]
    psdu = _psdus(rng, 333)[0]
    for gi in (0, 1):
        frame, nsym, ltf = TG.frame_int(psdu, 12, gi, joint=True, oracle=oracle)
        iq = _capture(rng, frame, 5.0, lead=2, tail=40)
        w = dm.zf_weights(iq, 2 + ltf, 0)
        got = G.model(iq, 2 + ltf, nb, cr, len(psdu), 0, w, gi=gi, joint=True)
        want = J.rx_model(TG.respace(iq, nsym, 2 + ltf) if gi else iq, 2 + ltf, nb, cr, len(psdu), 0, w)
        assert np.array_equal(got.soft, want.soft) and np.array_equal(got.theta, want.theta) and np.array_equal(got.xs, want.xs), gi
        assert (got.streams[0].error_code, got.streams[0].psdu) == (want.error_code, want.psdu) == (1, psdu), gi


def test_respaced_short_frames_decode_in_the_float64_receiver(oracle):
    rng = np.random.default_rng(64)
    for mcs in (8, 12, 14):
        ps = _psdus(rng, 200)
        frame, nsym, ltf = TG.frame_int(ps, mcs, 1, oracle=oracle)
        iq = _capture(rng, frame, 8.0, cfo_step=21.0, lead=400, tail=800)
        frames = rx64.receive(TG.respace(iq, nsym, 400 + ltf))
        assert len(frames) == 1 and frames[0].sig_ok and frames[0].mcs == mcs, mcs
        assert frames[0].fcs_ok == [True, True] and frames[0].psdu == ps, mcs


@pytest.mark.parametrize("joint", [0, 1])
def test_the_stage_composition_of_short_frames_is_the_gi_model(joint):
    """sora_amd.capi.rx_ht40_stages over the model's bricks (tests/ht40_stage_model.by_stages) takes SORA_HT40_SHORT_GI on a descriptor's code rate: 18 bursts of
    freq_comp11n at offset + 320 + 144 d, data_symbol_ht40 from 16 samples earlier -- soft bytes, theta and detected symbols of tests/ht40_gi_model.py"""
    import ht40_gi_cases as C
    import ht40_stage_model as sm
    frames = [f for f in C.bank(joint) if f["nsym"] <= 2][:6]
    assert {f["gi"] for f in frames} == {0, 1}
    iq, offs = C.place(np.random.default_rng(70 + joint), frames, (1, 2, 3, 0))
    descs = C.descs(frames, offs)
    r = sm.by_stages(iq, descs, joint)
    want = C.models(joint, iq, descs, np.asarray(r["weights"]))
    for f in range(len(descs)):
        for a, b in zip([r["soft"][f]] if joint else r["soft"][f], [want[f].soft] if joint else want[f].soft):
            assert np.array_equal(a, b), f
        assert np.array_equal(r["theta"][f], want[f].theta) and np.array_equal(r["xs"][f], want[f].xs), f
        assert all(g["error_code"] == 1 and g["short_gi"] == bool(descs[f][2] & C.SHORT) for g in r["rows"] if g["frame"] == f), f
