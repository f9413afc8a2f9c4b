"""The per-brick model of the 40 MHz HT stage entry points (tests/ht40_stage_model.py) held to what exists, without a GPU: its composition -- sora_amd.rx_ht40_stages,
the very function the GPU runs, over the model's bricks -- equals the integer model of the data field (oracle/ht40_data_model.py; joint coding: tests/ht40_joint_model.py)
in every soft byte, theta entry, detected symbol on the occupied bins and PSDU byte; its zero-forcing weights are so_ht40_zf_weights'; its float32 MMSE restatement is
within +-1 LSB of a float64 evaluation; its decimator and noise sum are tests/ht40_front_model.py's."""
import numpy as np
import pytest

from oracle import ht40_data_model as dm
from oracle import py_ht40 as m
import ht40_joint_model as J
import ht40_stage_model as sm
from test_ht40_data_model import send, H0

NDBPS0 = {1: 54, 2: 108, 4: 216, 6: 324}                                         # per stream at rate 1/2


def lens_for(nb, nsym):
    """PSDU lengths (unequal where the symbol count leaves room) whose longer one needs exactly nsym symbols at rate 1/2"""
    L = (nsym * NDBPS0[nb] - 22) // 8
    assert L >= 4 and m.nsym_for([L, L], nb, 0) == nsym
    return (L, max(4, L - 3 - nb))


def check_against_data_model(iq, desc, r, f=0):
    off, nb, cr, l0, l1, cfo = desc[:6]
    w = np.asarray(r["weights"][f])
    want = dm.model(iq, off, nb, cr, (l0, l1), cfo, w)
    assert want.nsym == len(r["theta"][f]) - 1
    assert np.array_equal(r["theta"][f], want.theta), (r["theta"][f], want.theta)
    assert np.array_equal(r["xs"][f][:, :, sm.OCC], want.xs[:, :, sm.OCC])
    for s in range(2):
        assert np.array_equal(r["soft"][f][s], want.soft[s]), (f, s)
        row = r["rows"][2 * f + s]
        assert (row["frame"], row["stream"], row["nsym"]) == (f, s, want.nsym)
        assert (row["error_code"], row["crc32"], row["mpdu"]) == (want.streams[s].error_code, want.streams[s].crc32, want.streams[s].psdu), (f, s)
    return want


@pytest.mark.parametrize("sigma", [0.0, 6.0])
@pytest.mark.parametrize("nsym", [1, 2, 3, 12])
@pytest.mark.parametrize("nb", [1, 2, 4, 6])
def test_composition_is_the_data_model(nb, nsym, sigma):
    rng = np.random.default_rng(100 * nb + 10 * nsym + int(sigma))
    lens = lens_for(nb, nsym); lead = int(rng.integers(0, 70))
    iq, ps, coded, n = send(rng, nb, 0, lens, sigma, lead=lead)
    assert n == nsym
    nv = 2 * sigma * sigma / 128.0
    desc = (lead, nb, 0, lens[0], lens[1], 0, nv)
    r = sm.by_stages(iq, [desc])
    want = check_against_data_model(iq, desc, r)
    w = np.asarray(r["weights"][0]); rest = np.setdiff1d(np.arange(128), sm.OCC)
    assert not w[:, rest].any() and not np.asarray(r["h"][0])[:, rest].any()
    if sigma == 0.0:
        assert np.array_equal(w[:, sm.OCC], dm.zf_weights(iq, lead, 0)[:, sm.OCC])       # TMimoChannelEst's own inverse, bit for bit
    for s in range(2):
        assert want.streams[s].error_code == sm.E_FRAME_OK and want.streams[s].psdu == ps[s]     # (the frame is decodable: the comparison is not of two failures)


@pytest.mark.parametrize("cfo", [0, 37, -511, 4096])
@pytest.mark.parametrize("nv", [0.0, 3000.0])
def test_described_cfo(cfo, nv):
    """sent with the opposite step, described with `cfo`: TFreqComp_11n's record {k cfo | 8 cfo | theta}, advanced by the brick itself, is the handle's phase n cfo - theta"""
    rng = np.random.default_rng(abs(cfo) + int(nv))
    nb, cr, lens = 4, 2, (61, 50)
    iq, ps, coded, nsym = send(rng, nb, cr, lens, 3.0, cfo_step=float(-cfo), lead=9)
    desc = (9, nb, cr, lens[0], lens[1], cfo, nv)
    r = sm.by_stages(iq, [desc])
    want = check_against_data_model(iq, desc, r)
    if nv == 0.0:
        assert np.array_equal(np.asarray(r["weights"][0])[:, sm.OCC], dm.zf_weights(iq, 9, cfo)[:, sm.OCC])
    assert np.abs(want.theta.astype(int)).max() < 1500, want.theta
    assert all(want.streams[s].psdu == ps[s] for s in range(2))


def test_mistuned_descriptor_wraps_theta_and_a_batch_of_unequal_frames_is_walked_together():
    """tests/test_ht40_data_model.py's mistuned frame (sent with step 37, described as 0: theta passes +-32768) beside two shorter frames of other modulations in one
    call: the frames that have ended take part with a count of 0 and keep their theta"""
    rng = np.random.default_rng(37)
    iq0, ps0, _, n0 = send(rng, 1, 0, (75, 60), 2.0, cfo_step=37.0, lead=3)
    iq1, ps1, _, n1 = send(rng, 6, 1, (80, 33), 4.0, lead=0)
    iq2, ps2, _, n2 = send(rng, 2, 2, (40, 44), 0.0, lead=11)
    assert n0 == 12 and n1 < n0 and n2 < n0
    o1 = iq0.shape[1] + 5; o2 = o1 + iq1.shape[1] + 2
    iq = np.zeros((2, o2 + iq2.shape[1] + 1, 2), np.int16)
    iq[:, :iq0.shape[1]] = iq0; iq[:, o1:o1 + iq1.shape[1]] = iq1; iq[:, o2:o2 + iq2.shape[1]] = iq2
    descs = [(3, 1, 0, 75, 60, 0, 0.0), (o1, 6, 1, 80, 33, 0, 7.0), (o2 + 11, 2, 2, 40, 44, 0, 0.0)]
    r = sm.by_stages(iq, descs)
    wants = [check_against_data_model(iq, d, r, f) for f, d in enumerate(descs)]
    th = wants[0].theta.astype(int)
    assert np.any(np.diff(th) < -30000) and th.max() > 26000 and th.min() < -26000, th
    for want, ps in zip(wants, (ps0, ps1, ps2)):
        assert all(want.streams[s].psdu == ps[s] for s in range(2))


@pytest.mark.parametrize("mcs,length", [(8, 5), (9, 37), (11, 200), (13, 90), (14, 301)])
def test_joint_coding_is_the_joint_model(mcs, length):
    nb, cr = m.MCS2[mcs]
    rng = np.random.default_rng(100 * mcs + length)
    psdu = m.add_fcs(rng.integers(0, 256, length - 4, dtype=np.uint8).tobytes())
    x, nsym = J.tx_joint(psdu, nb, cr, seed=int(rng.integers(1, 128)))
    iq = m.channel(x, H0, 6.0, rng, lead=4)
    desc = (4, nb, cr, length, 0, 0, 0.5625)
    r = sm.by_stages(iq, [desc], coding=1)
    want = J.rx_model(iq, 4, nb, cr, length, 0, np.asarray(r["weights"][0]))
    assert want.nsym == nsym == r["rows"][0]["nsym"] and len(r["rows"]) == 1
    assert np.array_equal(r["soft"][0], want.soft) and r["soft"][0].shape == (nsym * 216 * nb,)
    row = r["rows"][0]
    assert (row["error_code"], row["crc32"], row["mpdu"], row["length"]) == (want.error_code, want.crc32, want.psdu, length)
    assert want.error_code == sm.E_FRAME_OK and want.psdu == psdu


def test_float32_mmse_restatement_is_within_one_lsb_of_float64():
    """The tolerance the project states for the handle's weights, on the population it states it for (tests/test_gpu_ht40.py::test_mmse_weights_against_float64): the
    channel matrices TMimoChannelEst's combination gives on frames through a 2x2 channel of gains 1 / 0.35 / 0.3 / 0.9 with random phases at a 10 LSB floor, noise_var
    3000 (and the floor's own 2 sigma^2 / 128), every occupied carrier whose float64 weight stays inside +-32000.  The float64 evaluation is numpy's own solve of
    (H^H H + s2 I) W' = H^H, not a copy of the restatement's order of operations; the restatement in float64 must agree with it to the rounding of the int16."""
    from test_gpu_ht40 import make_frames
    rng = np.random.default_rng(6)
    iq, descs, _ = make_frames(rng, [(4, 0, 80, 80)] * 4, sigma=10.0)
    ops = sm.ModelOps()
    worst = 0.0; checked = 0
    for d in descs:
        off = d[0]
        rec = np.zeros((1, 24), np.int16)
        c0, c1 = ops.freq_comp(iq[0], iq[1], [off], [40], rec)
        y0, y1 = ops.data_symbol(c0, c1, [off], [2], [0], 2)
        h = sm.mimo_h(ops.fft128(y0), ops.fft128(y1))[:, sm.OCC]
        for nv in (3000.0, 2 * 10.0 * 10.0 / 128.0):
            a = sm.mmse_solve(h, np.float32(nv)).astype(float); b = sm.mmse_solve(h, float(np.float32(nv)), np.float64).astype(float)
            for c in range(h.shape[1]):
                H = (h[:, c, 0].astype(float) + 1j * h[:, c, 1].astype(float)).reshape(2, 2)
                W = np.linalg.solve(H.conj().T @ H + float(np.float32(nv)) * np.eye(2), H.conj().T)
                W = W / np.real(np.diag(W @ H))[:, None] * 65536.0
                want = np.stack([W.reshape(4).real, W.reshape(4).imag], axis=1)
                if np.abs(want).max() > 32000:
                    continue
                assert np.abs(b[:, c] - want).max() <= 0.5 + 1e-6, (c, b[:, c], want)
                worst = max(worst, float(np.abs(a[:, c] - want).max())); checked += 1
    assert checked >= 4 * 2 * 100, checked
    assert worst <= 1.0, worst


def test_decimator_and_noise_sum_are_the_front_models():
    import ht40_front_captures as fc
    import ht40_front_model as fm
    # the decimator on every int16 value that matters, from an even and an odd first kept sample
    x = np.array([[-32768, 32767], [5, 5], [-32768, -32768], [9, 9], [1, -1], [7, 7], [32767, -32768], [3, 3], [0, 0], [2, 2]], np.int16)
    assert sm.downsample(x, 5, 0).tolist() == [[-32768, 32767], [32767, 32767], [1, -1], [-32767, 32767], [0, 0]]
    assert sm.downsample(x, 5, 1).tolist() == [[32767, -32767], [-32768, -32768], [-1, 1], [32767, -32768], [0, 0]]
    assert np.array_equal(np.concatenate([sm.downsample(x, 3, 0), sm.downsample(x[6:], 2, 3)]), sm.downsample(x, 5, 0))
    # S and noise_var on captures: the model's kept samples, the L-LTF where the front model found it (368 kept samples in front of HT-STF), through the oracle's bricks
    O = sm.oracle()
    st = fc._Set(9)
    for mcs, length, sigma, lead in ((9, 60, 5.0, 280), (13, 41, 60.0, 333), (8, 4, 0.0, 400)):
        cap = st.one("mcs%d" % mcs, "plain", mcs, length, lead=lead, sigma=sigma)
        ev = fm.front(cap.iq[0], cap.iq[1])[0]
        assert ev["error_code"] == 0
        n = len(cap.iq[0]) // 2
        k0, k1 = sm.downsample(cap.iq[0], n), sm.downsample(cap.iq[1], n)
        s0 = ev["a20"] - 368
        l0, l1 = k0[s0:s0 + 128], k1[s0:s0 + 128]
        vfo = O.cfo_est11n(l0, l1)
        assert int(vfo[1]) == ev["cfo"]
        _, c0, c1 = O.freq_comp11n(vfo, l0, l1)
        f0 = np.concatenate([O.fft(c0[:64], 64), O.fft(c0[64:], 64)]); f1 = np.concatenate([O.fft(c1[:64], 64), O.fft(c1[64:], 64)])
        S = sm.noise_S(f0, f1)
        assert S == ev["S"] and (S > 0) == (sigma > 0 or S > 0)
        assert sm.noise_var(S) == np.float32(fm.noise_var_of(ev["S"])) and sm.noise_var(S).dtype == np.float32


def test_front_composition_is_the_front_models_first_event():
    """sora_amd.rx_ht40_front_stages over the model's bricks against tests/ht40_front_model.front on the capture set of tests/ht40_front_captures.py (every family but the
    captures that end inside the header: the end-of-capture flush is not composed): the first event's a20, mcs, ht_len, nsym, cfo, end_sample, error_code and S exactly,
    noise_var = S / 416 rounded to float32, and the descriptor by k_ht40_plan's rule.  Every cause of a header failure is among them."""
    import ht40_front_captures as fc
    import ht40_front_model as fm
    caps = [c for c in fc.build(False, full=False) if c.family != "cut"]
    errors = set(); checked = 0
    for cap in caps:
        want = fm.front(cap.iq[0], cap.iq[1])
        got = sm.front_by_stages(cap.iq[0], cap.iq[1], [(0, len(cap.iq[0]))])[0]
        assert (got is None) == (not want), cap.name
        if got is None:
            continue
        w = want[0]
        assert {k: int(got[k]) for k in ("a20", "mcs", "ht_len", "nsym", "cfo", "end_sample", "error_code", "S")} == \
               {k: int(w[k]) for k in ("a20", "mcs", "ht_len", "nsym", "cfo", "end_sample", "error_code", "S")}, cap.name
        assert got["noise_var"] == np.float32(fm.noise_var_of(w["S"])) and got["noise_var"].dtype == np.float32
        if w["error_code"] == 0:
            assert got["descriptor"][:7] == fm.descriptor(0, w, float(got["noise_var"]))[:7], cap.name
        else:
            assert "descriptor" not in got
        errors.add(w["error_code"]); checked += 1
    assert errors == {0, fm.E_PLCP_HEADER_FAIL} and checked >= 40
    assert len([c for c in caps if c.family == "gate"]) >= 9                      # bad parity, CRC-8, MCS 7 / 15, CBW 20, LENGTH 3 / 4001, L-SIG LENGTH 751
