"""40 MHz HT 2x2 transmitter (sora_hip_tx_ht40), the parts that need no GPU: the exports and the per-chain sample count; the integer model
of the waveform (tests/tx_ht40_model.py) against the float64 model that defines the format (oracle/py_ht40.py::tx_frame); that no stage of
the fixed-point IFFT<128> saturates at A = 16384; that the integer frame is a frame (the float64 receiver oracle/ht40_rx_f64.py decodes
every MCS from it through a channel) and that its preamble is the reference's (the restated reference front end parses it)."""
import ctypes

import numpy as np
import pytest

from oracle import py_ht40 as m
from oracle import ht40_rx_f64 as rxf
import tx_ht40_model as T

# |integer frame - tx_frame x A / 128|, worst component over MCS 8..14 x lengths 5, 200, 1496 (seeds 1000 mcs + len), measured on the CPU
# oracle: 9.2 LSB (at an rms of about 1230).  It is the transform's rounding and does not grow with the frame; the limit is twice that,
# rounded up to a whole LSB, the margin covering other payloads.
MEASURED_LSB = 9.2
LIMIT_LSB = 19


@pytest.fixture(scope="module")
def sora():
    import sora_amd
    sora_amd.load()
    return sora_amd


def _psdus(rng, ln):
    return [m.add_fcs(rng.integers(0, 256, ln, dtype=np.uint8).tobytes()) for _ in range(2)]


_FRAMES = {}


def _frame(oracle, mcs, ln):
    """the integer frame of (mcs, ln bytes without FCS), payload seeded by both; computed once for all tests"""
    if (mcs, ln) not in _FRAMES:
        ps = _psdus(np.random.default_rng(1000 * mcs + ln), ln)
        _FRAMES[mcs, ln] = (ps,) + T.frame_int(ps, mcs, oracle=oracle)
    return _FRAMES[mcs, ln]


def _step_lengths(mcs, max_nsym=12):
    """lengths (without FCS) on both sides of every step of N_SYM up to max_nsym"""
    nd = m.ndbps(*m.MCS2[mcs])
    out = []
    for n in range(1, max_nsym + 1):
        top = (n * nd - 22) // 8 - 4                                 # the longest MPDU that fits n symbols
        out += [v for v in (top, top + 1) if 1 <= v <= 3996]
    return sorted(set(out))


def test_exports_exist_and_are_typed(sora):
    L = sora.load()
    assert L.sora_hip_tx_ht40_samples.restype is ctypes.c_size_t and L.sora_hip_tx_ht40_samples.argtypes == [ctypes.c_uint32] * 2
    assert len(L.sora_hip_tx_ht40.argtypes) == 10 and L.sora_hip_tx_ht40.argtypes[5] is ctypes.c_size_t
    assert callable(sora.tx_ht40) and callable(sora.tx_ht40_samples)
    assert L.sora_hip_abi_version() == 4


@pytest.mark.parametrize("mcs", range(8, 15))
def test_sample_count(sora, mcs):
    nb, cr = m.MCS2[mcs]
    steps = _step_lengths(mcs)
    assert len({m.nsym_for([ln + 4], nb, cr) for ln in steps}) >= 12 or mcs == 8
    for ln in [1, 2, 3, 37, 1496, 3996] + steps:
        nsym = m.nsym_for([ln + 4], nb, cr)
        assert sora.tx_ht40_samples(ln, mcs) == 1280 + 160 * (2 + nsym), (mcs, ln)
        assert nsym == sora.load().sora_ht40_symbols(ln + 4, ln + 4, nb, cr), (mcs, ln)
    assert m.nsym_for([4000], 1, 0) == 593 and sora.tx_ht40_samples(3996, 8) == 1280 + 160 * 595


@pytest.mark.parametrize("mcs,ln", [(7, 100), (15, 100), (32, 100), (8, 0), (14, 0), (8, 3997), (14, 3997)])
def test_frames_that_are_not_accepted_give_zero_samples(sora, mcs, ln):
    assert sora.tx_ht40_samples(ln, mcs) == 0


def test_python_wrapper_refuses_before_any_launch(sora):
    for a, b, mcs in (([b"\x01\x02"], [b"\x03\x04"], [15]), ([b"\x01\x02"], [b"\x03"], [9]), ([b""], [b""], [9]), ([bytes(3997)], [bytes(3997)], [9])):
        with pytest.raises(sora.SoraError):
            sora.tx_ht40(a, b, mcs)


def test_entry_point_refuses_without_a_device(sora):
    if sora.device_count() > 0:
        pytest.skip("a HIP device is present")
    L = sora.load()
    p = ctypes.c_void_p(16)
    assert L.sora_hip_tx_ht40(p, p, p, p, None, 1, p, p, p, None) == -5
    assert b"no HIP device" in L.sora_hip_last_error()


def test_levels_are_the_issued_integers():
    assert T.A == 16384 and [T.level(nb) for nb in (1, 2, 4, 6)] == [6144, 6144, 4000, 2214]
    P = T.preamble_bins(9, 100, 4)
    assert set(np.unique(np.abs(P["stf"]))) == {0, 17053} and set(np.unique(np.abs(P["lltf"]))) == {0, 16384}
    assert not P["lsig"][:, 1][[(k - 32) % 128 for k in range(-26, 27)]].any() and set(np.unique(np.abs(P["htsig0"]))) == {0, 16384}
    k = -26                                                             # the upper half is the lower half times j, exactly
    for name in P:
        lo, up = P[name][(k - 32) % 128], P[name][(k + 32) % 128]
        assert (up[0], up[1]) == (-lo[1], lo[0]), name


@pytest.mark.parametrize("mcs", range(8, 15))
def test_integer_model_against_the_float_model(oracle, mcs):
    """Worst |integer frame - tx_frame x A / 128| over both chains and components, printed per case.  Measured (all MCS, lengths 5, 200,
    1496): 9.2 LSB; asserted at 19 LSB = twice that, rounded up."""
    for ln in (5, 200, 1496):
        ps, xi, nsym, pre = _frame(oracle, mcs, ln)
        xf, nsym_f, pre_f = m.tx_frame(ps, mcs)
        assert (nsym, pre) == (nsym_f, pre_f) and pre == 1280 and xi.shape == (2, xf.shape[1], 2)
        xf = xf * T.A / 128.0
        d = max(np.abs(xi[..., 0] - xf.real).max(), np.abs(xi[..., 1] - xf.imag).max())
        print("tx_ht40 integer model vs float model: MCS %d len %d nsym %d worst %.2f LSB (peak %d)" % (mcs, ln, nsym, d, np.abs(xi.astype(int)).max()))
        assert d <= LIMIT_LSB, (mcs, ln, d)
        assert np.abs(xi.astype(int)).max() < 32767


@pytest.mark.parametrize("si,sq", [(1, 1), (1, -1), (-1, 1), (-1, -1)])
def test_no_stage_of_the_transform_saturates(oracle, si, sq):
    """every data carrier at the 64-QAM corner of one sign, pilots added: the in-phase worst case of a data symbol.  A stage that
    saturated inside the fixed-point IFFT<128> would show as a deviation from the float transform far beyond its rounding."""
    d = T.level(6)
    X = np.zeros((128, 2), np.int64)
    for k in m.DATA_CARRIERS:
        X[k % 128] = (si * 7 * d, sq * 7 * d)
    for k in m.PILOTS:
        X[k % 128, 0] = 2 * T.level(1)
    t = T.ifft128(X, oracle).astype(np.int64)
    f = np.fft.ifft(X[:, 0] + 1j * X[:, 1])
    dev = max(np.abs(t[:, 0] - f.real).max(), np.abs(t[:, 1] - f.imag).max())
    print("corner symbol (%+d, %+d): peak %d, worst deviation %.2f LSB" % (si, sq, np.abs(t).max(), dev))
    assert dev <= LIMIT_LSB
    assert t.max() < 32767 and t.min() > -32767


@pytest.mark.parametrize("mcs", range(8, 15))
def test_the_integer_frame_is_a_frame(oracle, mcs):
    """through a 2x2 channel with cross-talk and noise into the float64 receiver: one frame, the MCS and LENGTH sent, both PSDUs with a good FCS"""
    for ln in (1, 196, 1496):                                           # 5, 200 and 1500 bytes with FCS
        ps, xi, nsym, pre = _frame(oracle, mcs, ln)
        rng = np.random.default_rng(77 * mcs + ln)
        x = xi[..., 0].astype(float) + 1j * xi[..., 1]
        y = m.channel(x, np.array([[1, 0.3j], [0.25, 0.9]]), 8.0, rng, scale=250.0 * 128.0 / T.A, lead=400)
        y = np.concatenate([y, np.zeros((2, 800, 2), np.int16)], axis=1)
        fr = rxf.receive(y)
        assert len(fr) == 1, (mcs, ln, len(fr))
        f = fr[0]
        assert f.sig_ok and f.mcs == mcs and f.length == ln + 4, (mcs, ln, f.mcs, f.length)
        assert list(f.psdu) == [ps[0], ps[1]] and all(f.fcs_ok), (mcs, ln, f.fcs_ok)


@pytest.mark.parametrize("mcs", [8, 9, 10])
def test_the_preamble_is_the_references(oracle, mcs):
    """the even samples of x[n] j^n of each chain (py_ht40.front_end_view) through the restated reference 802.11n front end: one event with
    the MCS and LENGTH that were sent (as tests/test_ht40_preamble_model.py does for the float model)"""
    for ln in (56, 196, 1496):                                          # LENGTH 60, 200, 1500
        ps, xi, nsym, pre = _frame(oracle, mcs, ln)
        rng = np.random.default_rng(5 * mcs + ln)
        x = xi[..., 0].astype(float) + 1j * xi[..., 1]
        y = m.channel(x, [[1.0, 0.2j], [0.15, 0.9]], 0.0 if ln == 56 else 20.0, rng, scale=250.0 * 128.0 / T.A, lead=400)
        y = np.concatenate([y, np.zeros((2, 2000, 2), np.int16)], axis=1)
        y = y[:, :y.shape[1] // 28 * 28]
        ev = oracle.rx11n_capture(m.front_end_view(y[0]), m.front_end_view(y[1]))
        assert len(ev) == 1, (mcs, ln, ev)
        e = ev[0]
        assert e["error_code"] != 0x80000005 and e["rate_kbps"] == mcs and e["length"] == ln + 4, (mcs, ln, hex(e["error_code"]), e["rate_kbps"], e["length"])
