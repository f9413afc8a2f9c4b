"""GPU transmitter at 44 MHz (sora_hip_tx11a44: k_tx11a with TUpsample40MTo44M in front of the pack) against what the reference's
CreateModGraph11a_44M + CreatePreamble11a_44M sent (tests/golden/reftx11a_44.npz), against the closed form over the oracle's 40 MHz
frames (tests/tx11a44_model.py), at sample offsets off the wide store's alignment, and looped back through ingest and the 44 MHz receiver."""
import os

import numpy as np
import pytest

from oracle.pyoracle import RATES
from tx11a44_model import capture44, compared, excluded, frame44_from_tx40, has_rail, rail_free_seed

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sora():
    import sora_amd
    if sora_amd.device_count() <= 0:
        pytest.skip("no HIP device")
    return sora_amd


def blocks_of(sora, length, rate):
    return sora.tx11a_samples(length, rate) // 160


def test_fixture_frames_in_one_mixed_call(sora):
    """Outside the indices where the reference read behind its input block: its samples.  At those indices: the closed form with x[160] = 0,
    wherever the block's last sample is known from the 40 MHz bytes (not at a rail)."""
    z = np.load(os.path.join(ROOT, "tests", "golden", "reftx11a_44.npz"))
    n = len(z["rate"])
    mpdus = [z["mpdu_%d" % i].tobytes() for i in range(n)]
    out, off = sora.tx11a(mpdus, [int(r) for r in z["rate"]], [int(s) for s in z["seed"]], sample_rate_mhz=44)
    got = out.cpu().numpy()
    nrail = nheld = 0
    for i in range(n):
        tx40, tx44 = z["tx40_%d" % i], z["tx44_%d" % i]
        g = got[off[i]:off[i + 1]]
        assert len(g) == len(tx44) == sora.tx11a_samples(len(mpdus[i]), int(z["rate"][i]), 44)
        keep = compared(len(tx44))
        assert np.array_equal(g[keep], tx44[keep]), (i, int(z["rate"][i]), np.flatnonzero((g != tx44).any(axis=1) & keep)[:8])
        model = frame44_from_tx40(tx40, allow_rails=True)
        at_rail = ((tx40 == 127) | (tx40 == -128)).any(axis=1)
        ex = [e for e in excluded(len(tx44)) if not at_rail[e // 176 * 160 + 159]]
        assert np.array_equal(g[ex], model[ex]), (i, int(z["rate"][i]))
        nrail += has_rail(tx40); nheld += len(ex)
    assert nrail == 2 and nheld > 150


def lengths_around_whole_passes(sora, rate):
    """MPDU lengths whose symbol count, SIGNAL included, is one below, at and one above a multiple of eight -- the kernel makes eight symbols
    per pass -- plus 1 and 260 bytes.  (9 Mbps pads to an even number of data symbols: no frame of exactly 16.)"""
    out = [1, 260]
    for want in (15, 16, 17):
        hit = [ln for ln in range(1, 600) if blocks_of(sora, ln, rate) - 4 == want]
        assert hit or (rate == 9000 and want == 16), (rate, want)
        out += hit[:1]
    return out


def test_model_parity_around_whole_passes(sora, oracle):
    rng = np.random.default_rng(4416)
    mpdus, rates, seeds, want = [], [], [], []
    for rate in RATES:
        for k, ln in enumerate(lengths_around_whole_passes(sora, rate)):
            mp = bytes(rng.integers(0, 256, ln).astype(np.uint8))
            sd = rail_free_seed(oracle, mp, rate, (0xFF, 0x5B, 0x02, 0x7E, 0xA5)[k])
            tx40 = oracle.tx(mp, rate, sd)
            assert not has_rail(tx40)                                            # none is skipped: every frame is one the model is exact for
            mpdus.append(mp); rates.append(rate); seeds.append(sd); want.append(frame44_from_tx40(tx40))
    assert len(mpdus) == 39
    out, off = sora.tx11a(mpdus, rates, seeds, sample_rate_mhz=44)
    got = out.cpu().numpy()
    for f in range(len(mpdus)):
        assert np.array_equal(got[off[f]:off[f + 1]], want[f]), (rates[f], len(mpdus[f]), hex(seeds[f]), np.flatnonzero((got[off[f]:off[f + 1]] != want[f]).any(axis=1))[:8])


def test_frames_at_sample_offsets_that_are_not_multiples_of_four(sora, oracle):
    """Eight bytes at a time where a frame starts on an 8-byte boundary, two bytes at a time elsewhere: the same samples, and the gaps stay untouched."""
    rng = np.random.default_rng(4499)
    rates = [RATES[i % 8] for i in range(16)]
    gaps = [(1, 2, 3, 5, 0, 7, 4, 6)[i % 8] for i in range(16)]
    mpdus = [bytes(rng.integers(0, 256, 20 + 41 * i).astype(np.uint8)) for i in range(16)]
    seeds = [rail_free_seed(oracle, mpdus[i], rates[i], 0x5B + i) for i in range(16)]
    out, off = sora.tx11a(mpdus, rates, seeds, gaps=gaps, sample_rate_mhz=44)
    got = out.cpu().numpy()
    for f in range(16):
        tx40 = oracle.tx(mpdus[f], rates[f], seeds[f])
        assert not has_rail(tx40)
        assert not got[off[f]:off[f] + gaps[f]].any()
        assert np.array_equal(got[off[f] + gaps[f]:off[f + 1]], frame44_from_tx40(tx40)), (f, rates[f], gaps[f])


def test_mixed_batch_loops_back_through_ingest_and_the_44mhz_receiver(sora):
    import torch
    rng = np.random.default_rng(4477)
    rates = [RATES[i % 8] for i in range(24)]
    mpdus = [bytes(rng.integers(0, 256, 60 + 53 * i).astype(np.uint8)) for i in range(24)]
    out, off = sora.tx11a(mpdus, rates, [2 + (i * 7) % 126 for i in range(24)], sample_rate_mhz=44)
    tx = out.cpu().numpy()
    parts, descs, pos = [], [], 0
    for f in range(24):
        x = sora.ingest(torch.from_numpy(capture44(tx[off[f]:off[f + 1]])).cuda(), sora.INGEST_44TO40)
        n = x.shape[0] // 28 * 28                                                # whole bursts of TDownSample44_40
        parts.append(x[:n]); descs.append((pos, n, f)); pos += n
    iq = torch.cat(parts)
    rx = sora.Rx(24, iq.shape[0], sample_rate_mhz=44)
    rx.process_dev(iq, descs)
    res = rx.results(); rx.close()
    assert len(res) == 24
    for r in res:
        assert r["error_code"] == sora.E_FRAME_OK and r["mpdu"][:-4] == mpdus[r["capture_id"]] and r["rate_kbps"] == rates[r["capture_id"]]


def test_a_44mhz_call_between_two_40mhz_calls_leaves_them_alone(sora, oracle):
    rng = np.random.default_rng(4440)
    rates = [RATES[i % 8] for i in range(16)]
    mpdus = [bytes(rng.integers(0, 256, 30 + 67 * i).astype(np.uint8)) for i in range(16)]
    seeds = [int(s) for s in rng.integers(0, 256, 16)]
    a, off_a = sora.tx11a(mpdus, rates, seeds, sync=False)
    m, off_m = sora.tx11a(mpdus, rates, seeds, sync=False, sample_rate_mhz=44)
    b, off_b = sora.tx11a(mpdus, rates, seeds)
    a, b = a.cpu().numpy(), b.cpu().numpy()
    assert off_a == off_b and [11 * v // 10 for v in off_a] == off_m
    for f in range(16):
        want = oracle.tx(mpdus[f], rates[f], seeds[f])
        assert np.array_equal(a[off_a[f]:off_a[f + 1]], want) and np.array_equal(b[off_b[f]:off_b[f + 1]], want), (f, rates[f])


def test_unsupported_rate_and_sample_rate_are_refused(sora):
    assert sora.tx11a_samples(100, 11000, sample_rate_mhz=44) == 0
    with pytest.raises(sora.SoraError):
        sora.tx11a([b"x" * 10], [11000], sample_rate_mhz=44)
    with pytest.raises(ValueError):
        sora.tx11a([b"x" * 10], [6000], sample_rate_mhz=20)
