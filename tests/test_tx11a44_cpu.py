"""802.11a transmitter at 44 MHz (sora_hip_tx11a44), the parts that need no GPU: the closed form of TUpsample40MTo44M
(tests/tx11a44_model.py) against what the reference's CreateModGraph11a_44M + CreatePreamble11a_44M sent for the recorded frames
(tests/golden/reftx11a_44.npz, tests/golden/make_reftx11a_44.py); why the brick has to see 16-bit samples; the sample count of
the C entry point; and model-made frames through the oracle's 44 MHz receive path."""
import os

import numpy as np
import pytest

from oracle.pyoracle import RATES
from tx11a44_model import capture44, compared, excluded, frame44_from_tx40, has_rail, rail_free_seed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def frames():
    """-> [(mpdu, rate, seed, tx40, tx44)] of the fixture"""
    z = np.load(os.path.join(ROOT, "tests", "golden", "reftx11a_44.npz"))
    return [(z["mpdu_%d" % i].tobytes(), int(z["rate"][i]), int(z["seed"][i]), z["tx40_%d" % i], z["tx44_%d" % i]) for i in range(len(z["rate"]))]


@pytest.fixture(scope="module")
def sora():
    import sora_amd
    sora_amd.load()
    return sora_amd


def test_fixture_holds_every_rate_and_two_rail_frames(frames, oracle):
    plain = [f for f in frames if not has_rail(f[3])]
    assert sorted((f[1], len(f[0]), f[2]) for f in plain) == sorted([(r, 1, 0xFF) for r in RATES] + [(r, 37, 0x5B) for r in RATES])
    assert len(frames) - len(plain) == 2
    for mpdu, rate, seed, tx40, tx44 in frames:                                  # the 40 MHz half is the stream the oracle's transmitter is pinned to
        assert np.array_equal(oracle.tx(mpdu, rate, seed), tx40)
        assert len(tx44) * 10 == len(tx40) * 11 and len(tx40) % 160 == 0


def test_closed_form_reproduces_the_reference_on_every_rail_free_frame(frames):
    n = 0
    for mpdu, rate, seed, tx40, tx44 in frames:
        if has_rail(tx40):
            continue
        nblocks = len(tx40) // 160
        ex = excluded(len(tx44))
        assert len(ex) == nblocks - 3 and np.array_equal(ex, [176 * j + 175 for j in range(3, nblocks)])
        keep = compared(len(tx44))
        assert keep.sum() == len(tx44) - (nblocks - 3)
        got = frame44_from_tx40(tx40)
        assert np.array_equal(got[keep], tx44[keep]), (rate, len(mpdu), np.flatnonzero((got != tx44).any(axis=1) & keep)[:8])
        n += 1
    assert n == 16


def test_upsampling_the_packed_bytes_is_not_what_the_reference_sends(frames):
    """The brick runs in front of TPackSample16to8: on a frame whose 40 MHz stream touches an int8 rail, upsampling the bytes gives other
    samples than the reference's, away from the indices where it read behind its input.  Hence the kernel upsamples in 16 bits and clamps last."""
    rail = [f for f in frames if has_rail(f[3])]
    assert len(rail) == 2
    for mpdu, rate, seed, tx40, tx44 in rail:
        with pytest.raises(AssertionError):
            frame44_from_tx40(tx40)
        keep = compared(len(tx44))
        bad = (frame44_from_tx40(tx40, allow_rails=True) != tx44).any(axis=1) & keep
        assert bad.any()
        # ... and only next to a rail sample: output j of a block lies between inputs j - m - 1 and j - m
        at_rail = ((tx40 == 127) | (tx40 == -128)).any(axis=1)
        for i in np.flatnonzero(bad):
            b, j = divmod(int(i), 176)
            hi = 160 * b + j - j // 11
            assert at_rail[max(hi - 1, 0):hi + 1].any(), (rate, i)


def test_sample_count(sora, frames):
    for mpdu, rate, seed, tx40, tx44 in frames:
        assert sora.tx11a_samples(len(mpdu), rate, sample_rate_mhz=44) == len(tx44)
        assert sora.tx11a_samples(len(mpdu), rate) == len(tx40)
    L = sora.load()
    for rate in RATES:
        for ln in list(range(1, 300)) + [700, 1496, 1500, 2312, 4090, 4091]:
            n40 = sora.tx11a_samples(ln, rate)
            assert n40 > 0 and n40 % 160 == 0
            assert L.sora_hip_tx11a44_samples(ln, rate) == 11 * n40 // 10 == sora.tx11a_samples(ln, rate, 44)
    for rate in RATES:
        assert L.sora_hip_tx11a44_samples(4092, rate) == 0 and L.sora_hip_tx11a44_samples(5000, rate) == 0
    assert L.sora_hip_tx11a44_samples(100, 11000) == 0 and L.sora_hip_tx11a44_samples(100, 0) == 0


def test_sample_rate_other_than_40_or_44_is_refused(sora):
    for bad in (20, 0, None, 44.5):
        with pytest.raises(ValueError):
            sora.tx11a_samples(100, 6000, sample_rate_mhz=bad)
        with pytest.raises(ValueError):
            sora.tx11a([b"x" * 10], [6000], sample_rate_mhz=bad)


def test_c_entry_point_without_a_device_or_with_a_null_pointer_fails_loudly(sora):
    L = sora.load()
    assert L.sora_hip_tx11a44(None, None, None, None, None, 1, None, None, None) < 0


def test_model_made_frames_decode_through_the_oracles_44mhz_receive_path(oracle):
    """One frame per rate, made with x[160] = 0 by the model, shifted << 8 with silence behind it, whole 28-sample bursts:
    TDownSample44_40 and the 44 MHz receive graph's restatement report FRAME_OK with the MPDU that went in."""
    rng = np.random.default_rng(4404)
    for i, rate in enumerate(RATES):
        mpdu = bytes(rng.integers(0, 256, 60 + 37 * i).astype(np.uint8))
        tx40 = oracle.tx(mpdu, rate, rail_free_seed(oracle, mpdu, rate, 2 + 9 * i))
        assert not has_rail(tx40)
        x40 = oracle.down44to40(capture44(frame44_from_tx40(tx40)))
        res = oracle.rx_capture(x40[:len(x40) // 28 * 28], 44)
        assert [(r["error_code"], r["rate_kbps"], r["mpdu"][:-4]) for r in res] == [(1, rate, mpdu)], (rate, res)
