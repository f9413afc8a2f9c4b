"""802.11n 2x2 transmitter (sora_hip_tx11n), the parts that need no GPU: the per-chain sample count against the recorded
waveforms of the reference modulator and, where oracle/_ref is built, against the live one; the refusals; the C entry point
failing loudly without a device; and the recipe of the fixed preamble fields, pinned in numpy against the recording."""
import ctypes
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "refgraph_11n.npz")
FIXTURE = [(8, 40, 2880), (9, 90, 2880), (10, 150, 3200), (12, 30, 1760)]    # frames 0..3 of refgraph_11n.npz


@pytest.fixture(scope="module")
def sora():
    import sora_amd
    sora_amd.load()
    return sora_amd


def test_sample_count_matches_the_recorded_frames(sora):
    z = np.load(GOLD)
    for k, (mcs, ln, n) in enumerate(FIXTURE):
        assert len(z["mpdu%d" % k]) == ln and len(z["tx%d_0" % k]) == len(z["tx%d_1" % k]) == n
        assert sora.tx11n_samples(ln, mcs) == n, (mcs, ln)


def test_sample_count_has_the_reference_extra_symbol(sora):
    """150 bytes at MCS 10: the standard's N_SYM is 9, the reference's graph emits 10 (N_SYM x N_DBPS = 1404 bits is not whole bytes)."""
    assert sora.tx11n_samples(150, 10) == 1600 + 10 * 160
    assert sora.tx11n_samples(151, 10) == 1600 + 10 * 160           # 9 x 156 bits ... still odd N_SYM
    assert sora.tx11n_samples(7, 8) == 1600 + 4 * 160               # MCS 8, N_SYM 3 (156 bits): four symbols
    assert sora.tx11n_samples(1, 14) == 1600 + 2 * 160              # MCS 14, N_SYM 1 (468 bits): two symbols
    assert sora.tx11n_samples(30, 12) == 1600 + 1 * 160             # MCS 12: 312 bits per symbol are whole bytes


def sweep_lengths(mcs):
    ndbps = {8: 52, 9: 104, 10: 156, 11: 208, 12: 312, 13: 416, 14: 468}[mcs]
    lens = {1, 2, 3, 4, 5, 37, 100, 151, 1000, 1500, 4092}
    for nstd in range(1, 12):                                       # the longest MPDU of nstd standard symbols: both parities of nstd
        ln = (nstd * ndbps - 22) // 8 - 4
        if ln >= 1:
            lens.add(ln)
    return sorted(lens)


def test_sample_count_equals_the_reference_modulator(sora):
    from oracle.pyoracle import ReferenceGraph
    g = ReferenceGraph()
    if not g.available():
        pytest.skip("oracle/_ref/libsora_refgraph.so not built (needs the reference tree)")
    extra = set()
    for mcs in range(8, 15):
        for ln in sweep_lengths(mcs):
            n = len(g.tx11n(bytes(ln), mcs)[0])
            assert sora.tx11n_samples(ln, mcs) == n, (mcs, ln)
            ndbps = {8: 52, 9: 104, 10: 156, 11: 208, 12: 312, 13: 416, 14: 468}[mcs]
            if n != 1600 + 160 * -(-((ln + 4) * 8 + 22) // ndbps):
                extra.add(mcs)
    assert extra == {8, 10, 14}, extra                              # both rounding branches were crossed where they exist


@pytest.mark.parametrize("mcs,ln", [(m, 100) for m in list(range(0, 8)) + [15, 16, 255]] + [(8, 0), (14, 0), (8, 4093), (14, 4093), (10, 65535)])
def test_unsupported_frames_give_zero_samples(sora, mcs, ln):
    assert sora.tx11n_samples(ln, mcs) == 0


def test_python_wrapper_refuses_an_unsupported_frame_before_any_launch(sora):
    with pytest.raises(sora.SoraError):
        sora.tx11n([b"\x01\x02\x03"], [15])
    with pytest.raises(sora.SoraError):
        sora.tx11n([b"\x01\x02\x03", b"\x04"], [9, 7])
    with pytest.raises(sora.SoraError):
        sora.tx11n([b""], [9])


def test_entry_point_refuses_without_a_device(sora):
    if sora.device_count() > 0:
        pytest.skip("a HIP device is present")
    L = sora.load()
    p = ctypes.c_void_p(16)
    assert L.sora_hip_tx11n(p, p, p, p, None, 1, p, p, p, None) == -5
    assert b"no HIP device" in L.sora_hip_last_error()


def preamble_recipe():
    """The fixed fields per chain, as the library builds them on the host: round(s * sum_k X_k exp(2 pi i k n / 128)) with
    s = 256 sqrt(2) (L-STF, HT-STF), K / sqrt(52) (L-LTF), K / sqrt(56) (HT-LTF), K = 1773.7209."""
    ltf = np.array([1, 1, -1, -1, 1, 1, -1, 1, -1, 1, 1, 1, 1, 1, 1, -1, -1, 1, 1, -1, 1, -1, 1, 1, 1, 1, 0,
                    1, -1, -1, 1, 1, -1, 1, -1, 1, -1, -1, -1, -1, -1, 1, 1, -1, -1, 1, -1, 1, -1, 1, 1, 1, 1], float)
    stf = np.array([1, -1, 1, -1, -1, 1, 0, -1, -1, 1, 1, 1, 1], float) * (1 + 1j)
    K = 1773.7209

    def sym(carriers, values, s):
        X = np.zeros(128, complex)
        X[np.asarray(carriers) % 128] = values
        t = s * np.fft.ifft(X) * 128
        return np.rint(t.real) + 1j * np.rint(t.imag)
    ts = sym(np.arange(-24, 25, 4), stf, 256 * np.sqrt(2))
    tl = sym(np.arange(-26, 27), ltf, K / np.sqrt(52))
    th = sym(np.arange(-28, 29), np.concatenate([[1, 1], ltf, [-1, -1]]), K / np.sqrt(56))
    out = []
    for ch in range(2):
        cyc = lambda t, n, start: t[(np.arange(n) - start) % 128]
        dl, dh = 8 * ch, 16 * ch
        out.append(np.concatenate([cyc(ts, 320, dl), cyc(tl, 320, 64 + dl), cyc(ts, 160, 32 + dh), cyc(th, 160, 32 + dh),
                                   (1 if ch else -1) * cyc(th, 160, 32 + dh)]))
    return out


def test_preamble_recipe_reproduces_the_recorded_training_fields():
    """L-STF + L-LTF (samples 0..639) and HT-STF + HT-LTF1 + HT-LTF2 (1120..1599) of both chains, all four recorded frames."""
    want = preamble_recipe()
    z = np.load(GOLD)
    for k in range(4):
        for ch in range(2):
            x = z["tx%d_%d" % (k, ch)].astype(np.int64)
            got = np.concatenate([x[:640], x[1120:1600]])
            w = want[ch]
            assert np.array_equal(got[:, 0], w.real.astype(np.int64)) and np.array_equal(got[:, 1], w.imag.astype(np.int64)), (k, ch)
