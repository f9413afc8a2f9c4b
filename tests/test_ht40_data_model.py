"""The integer model of the 40 MHz HT data field (oracle/ht40_data_model.py, the yardstick of tests/test_gpu_ht40_soft.py) held to the INDEPENDENT numpy model of
the format (oracle/py_ht40.py, written from IEEE 802.11n-2009 clause 20), so that it is not an echo of the kernel it judges: it must recover, bit for bit, what
py_ht40 transmits -- every coded bit of both streams on every symbol, and both PSDUs with a good FCS -- from weights the float model computes; it must follow a
carrier offset the descriptor does not know about across the int16 wrap of theta; its zero-forcing weights are the float inverse to the brick's rounding; and
its C composition equals the same bricks called one by one from Python."""
import numpy as np
import pytest

from oracle import ht40_data_model as dm
from oracle import py_ht40 as m

H0 = np.array([[1.0 * np.exp(0.3j), 0.35 * np.exp(-1.1j)], [0.3 * np.exp(2.0j), 0.9 * np.exp(-0.4j)]])
MCS = [(1, 0), (2, 0), (2, 2), (4, 0), (4, 2), (6, 1), (6, 2)]


def send(rng, nb, cr, lens, sigma, cfo_step=0.0, lead=0, seeds=(0x5D, 0x2B)):
    """-> (iq int16 [2, n, 2], psdus, coded bits per stream [nsym * 108 nb], nsym)"""
    ps = [m.add_fcs(rng.integers(0, 256, ln - 4, dtype=np.uint8).tobytes()) for ln in lens]
    x, nsym = m.tx(ps, nb, cr, seeds=seeds)
    coded = []
    for s in range(2):
        a, b = m.encode(m.stream_bits(ps[s], nsym, nb, cr, seeds[s]))
        coded.append(m.puncture(a, b, cr)[:nsym * 108 * nb])
    return m.channel(x, H0, sigma, rng, cfo_step=cfo_step, lead=lead), ps, coded, nsym


def q16(W):
    """py_ht40.mmse_weights' W [128, 2, 2] complex -> the kernel's Q16 layout int16 [4, 128, 2] (w00, w01, w10, w11)"""
    w = np.stack([W[:, 0, 0], W[:, 0, 1], W[:, 1, 0], W[:, 1, 1]]) * 65536.0
    return np.clip(np.rint(np.stack([w.real, w.imag], axis=2)), -32768, 32767).astype(np.int16)


@pytest.mark.parametrize("sigma", [0.0, 6.0])
@pytest.mark.parametrize("nb,cr", MCS)
def test_clean_loopback_recovers_every_coded_bit_and_both_psdus(nb, cr, sigma):
    rng = np.random.default_rng(1000 * nb + 10 * cr + int(sigma))
    lens = (int(rng.integers(30, 90)), int(rng.integers(90, 140)))
    lead = int(rng.integers(0, 70))
    iq, ps, coded, nsym = send(rng, nb, cr, lens, sigma, lead=lead)
    W = m.mmse_weights(m.rx_symbols(iq, lead, nsym), 2 * sigma * sigma / 128.0)
    r = dm.model(iq, lead, nb, cr, lens, 0, q16(W))
    assert r.nsym == nsym and nsym >= 2
    for s in range(2):
        hard = (r.soft[s] >= 4).astype(np.uint8)
        assert hard.shape == coded[s].shape
        per = 108 * nb
        for d in range(nsym):
            assert np.array_equal(hard[d * per:(d + 1) * per], coded[s][d * per:(d + 1) * per]), (nb, cr, sigma, s, d)
        assert r.streams[s].error_code == 1 and r.streams[s].psdu == ps[s], (nb, cr, sigma, s)
        assert r.streams[s].crc32 == int.from_bytes(ps[s][-4:], "little")
    assert np.abs(r.theta.astype(int)).max() < 400, r.theta                  # no carrier offset: the tracked phase stays near zero (400 / 65536 of a turn = 2.2 degrees)


def test_mistuned_descriptor_is_tracked_across_the_wrap_of_theta():
    """Sent with cfo_step = 37, described as cfo = 0: theta has to take the whole offset, 160 x 37 = 5920 per symbol, and passes +-32768 inside the frame's 12
    symbols.  The weights are the model's own zero-forcing ones, from HT-LTFs that rotate against each other like everything else."""
    rng = np.random.default_rng(37)
    nb, cr, lens = 1, 0, (75, 60)
    iq, ps, coded, nsym = send(rng, nb, cr, lens, 2.0, cfo_step=37.0, lead=3)
    assert nsym == 12
    r = dm.model(iq, 3, nb, cr, lens, 0, dm.zf_weights(iq, 3, 0))
    for s in range(2):
        assert r.streams[s].error_code == 1 and r.streams[s].psdu == ps[s], s
    th = r.theta.astype(int)
    step = (np.diff(th) + 32768) % 65536 - 32768                             # per-symbol update, unwrapped
    assert np.all(np.abs(step[2:] - 5920) < 600), step                       # the loop has settled on the ramp after two symbols
    assert np.any(np.diff(th) < -30000), th                                  # ... and theta really wrapped from near +32767 to near -32768
    assert th.max() > 26000 and th.min() < -26000, th
    # the same frame described correctly needs no tracking at all
    r2 = dm.model(iq, 3, nb, cr, lens, -37, dm.zf_weights(iq, 3, -37))
    assert np.abs(r2.theta.astype(int)).max() < 400 and all(r2.streams[s].psdu == ps[s] for s in range(2))


@pytest.mark.parametrize("nb", [1, 2, 4, 6])
def test_model_permutation_is_the_format_models(nb):
    for iss in range(2):
        p = dm.permutation(nb, iss)
        assert np.array_equal(p, m.interleave_map(nb, iss)) and sorted(p.tolist()) == list(range(108 * nb))
    assert not np.array_equal(dm.permutation(nb, 0), dm.permutation(nb, 1))
    assert [int(b) for b in dm.DATA_BINS] == [k % 128 for k in m.DATA_CARRIERS] and [int(b) for b in dm.PILOT_BINS] == [k % 128 for k in m.PILOTS]


def test_zero_forcing_weights_are_the_float_inverse_to_the_bricks_rounding():
    """zf_weights on a clean frame against py_ht40.mmse_weights(noise_var = 0) (float64 from the raw samples).  Bound: the GPU test of the same quantity
    (tests/test_gpu_ht40.py: kWeightTolLsb) states 32 LSB of Q16 for the fixed-point FFT<128> path in front of a float solve; the same bound holds here."""
    rng = np.random.default_rng(11)
    iq, ps, coded, nsym = send(rng, 2, 0, (40, 40), 0.0, lead=5)
    w = dm.zf_weights(iq, 5, 0).astype(float)
    want = q16(m.mmse_weights(m.rx_symbols(iq, 5, nsym), 0.0)).astype(float)
    occ = dm.OCCUPIED_BINS
    assert np.abs(want[:, occ]).max() > 100
    assert np.abs(w[:, occ] - want[:, occ]).max() <= 32.0, np.abs(w[:, occ] - want[:, occ]).max()


def test_the_composition_is_the_bricks_called_one_by_one():
    """so_ht40_data_field against the same pinned bricks driven from Python through their own entry points (freq_comp11n, fft, mimo_comp11n, so_dsp_atan16,
    demap11n), on a frame with a carrier offset, noise and a described cfo that is not a multiple of anything."""
    import ctypes
    rng = np.random.default_rng(12)
    nb, cr, lens = 6, 2, (60, 45)
    iq, ps, coded, nsym = send(rng, nb, cr, lens, 40.0, cfo_step=30.0, lead=7)
    cfo = -23
    w = dm.zf_weights(iq, 7, cfo)
    r = dm.model(iq, 7, nb, cr, lens, cfo, w)
    O = dm.oracle()
    O.L.so_dsp_atan16.restype = ctypes.c_int16
    theta = 0
    i16 = lambda v: ((int(v) + 32768) & 0xFFFF) - 32768
    for d in range(nsym):
        assert theta == int(r.theta[d])
        pos = 7 + 320 + 160 * d + 32
        n0 = 320 + 160 * d + 32
        st = np.array([i16((n0 + k) * cfo) for k in range(8)] + [i16(8 * cfo)] * 8 + [theta] * 8, np.int16)
        _, c0, c1 = O.freq_comp11n(st, iq[0, pos:pos + 128], iq[1, pos:pos + 128])
        y0, y1 = O.fft(c0, 128), O.fft(c1, 128)
        xs = np.zeros((2, 128, 2), np.int16)
        for half in range(2):                                               # the 20 MHz brick takes 64 carriers and the weights as [row][64 a | 64 b]
            sl = slice(64 * half, 64 * half + 64)
            hinv = np.stack([np.concatenate([w[0, sl], w[1, sl]]), np.concatenate([w[2, sl], w[3, sl]])])
            xs[0, sl], xs[1, sl] = O.mimo_comp11n(hinv, y0[sl], y1[sl])
        assert np.array_equal(xs, r.xs[d]), d
        t = []
        for s in range(2):
            tot = sum(int(O.L.so_dsp_atan16(ctypes.c_int16(int(xs[s, b, 0])), ctypes.c_int16(int(xs[s, b, 1])))) for b in dm.PILOT_BINS)
            t.append(i16(int(tot / 6)))                                     # C truncation
        theta = i16(theta + i16((t[0] + t[1]) >> 1))
    assert theta == int(r.theta[nsym])
    # demapping + de-interleaving of the last symbol from xs: the 20 MHz brick's tables through so_demap11n on a burst that holds the first 52 data carriers
    per = 108 * nb
    for s in range(2):
        raw = []
        for c0 in range(0, 108, 52):
            bins = dm.DATA_BINS[c0:c0 + 52]
            burst = np.zeros((64, 2), np.int16)
            slots = [i for i in list(range(36, 64)) + list(range(1, 29)) if i not in (43, 57, 7, 21)]       # so_demap11n's carrier order
            burst[slots[:len(bins)]] = r.xs[nsym - 1][s][bins]
            raw.append(O.demap11n(nb, burst)[:len(bins) * nb])
        raw = np.concatenate(raw)
        assert np.array_equal(r.soft[s][(nsym - 1) * per:], raw[dm.permutation(nb, s)]), s
