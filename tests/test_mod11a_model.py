"""tests/mod11a_model.py -- the per-brick numpy models of the 802.11a modulation graph, the truth of tests/test_gpu_mod_stages.py -- pinned without a GPU: the
model chain against the oracle's transmitter (itself pinned to the compiled reference modulator), against that modulator where oracle/_ref is built, and brick by
brick where the oracle has the brick or its inverse."""
import os

import numpy as np
import pytest

import mod11a_model as M
from oracle.pyoracle import RATES, REFGRAPH_SO
from tx11a44_model import compared

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = (1, 2, 3, 37, 260, 1496)
SEEDS = (0x00, 0x01, 0xFF, 0x5B)


def cases():
    """every rate x every length, the seeds in rotation so that each (rate, seed) and each (length, seed) pair occurs"""
    out = []
    for i, rate in enumerate(RATES):
        for j, ln in enumerate(LENGTHS):
            out.append((rate, ln, SEEDS[(i + j) % 4]))
        out += [(rate, 37, s) for s in SEEDS]
    return sorted(set(out))


def mpdu_of(rate, ln, seed):
    return bytes(np.random.default_rng([rate, ln, seed]).integers(0, 256, ln).astype(np.uint8))


@pytest.fixture(scope="module")
def model_frames():
    return {c: M.frame40(mpdu_of(*c), c[0], c[2]) for c in cases()}


def test_cases_cover_what_they_should():
    cs = cases()
    assert {c[0] for c in cs} == set(RATES) and len(RATES) == 8
    assert {(c[0], c[1]) for c in cs} == {(r, ln) for r in RATES for ln in LENGTHS}
    assert {(c[0], c[2]) for c in cs} >= {(r, s) for r in RATES for s in (0x00, 0x01, 0xFF)}


def test_model_chain_equals_the_oracles_transmitter(oracle, model_frames):
    for (rate, ln, seed), got in model_frames.items():
        want = oracle.tx(mpdu_of(rate, ln, seed), rate, seed)
        assert got.shape == want.shape and np.array_equal(got, want), (rate, ln, seed)


def test_model_chain_equals_the_compiled_reference_modulator(model_frames):
    """CreatePreamble11a_40M + CreateModGraph11a_40M compiled from the reference's sources, where oracle/_ref is built"""
    if not os.path.exists(REFGRAPH_SO):
        pytest.skip("oracle/_ref/libsora_refgraph.so not built (reference tree absent)")
    from oracle.pyoracle import ReferenceGraph
    g = ReferenceGraph()
    for (rate, ln, seed), got in model_frames.items():
        want = g.tx11a(mpdu_of(rate, ln, seed), rate, seed)
        assert got.shape == want.shape and np.array_equal(got, want), (rate, ln, seed)


def test_ifftx_is_the_fixed_point_ifft128_with_shift_guard_interval_and_window(oracle):
    rng = np.random.default_rng(128)
    bins = [rng.integers(-a, a + 1, (4, 64, 2)) for a in (300, 11000, 32767)]
    bins.append(np.where(rng.integers(0, 2, (6, 64, 2)) == 1, 32767, -32767))    # full scale: the saturating butterflies
    bins.append(np.full((1, 64, 2), 32767)); bins.append(np.full((1, 64, 2), -32767))
    bins = np.concatenate(bins).astype(np.int16)
    got = M.ifftx(bins)
    assert got.shape == (len(bins), 160, 2)
    for b, g in zip(bins, got):
        x = np.zeros((128, 2), np.int16)
        x[0:32] = b[0:32]; x[96:128] = b[32:64]
        t = oracle.fft(x, n=128, inverse=True).astype(np.int32) >> 4
        want = np.concatenate([t[96:], t])
        for i in (0, 1, 158, 159):
            want[i] >>= 1
        assert np.array_equal(g, want.astype(np.int16))
    assert np.abs(got.astype(np.int32)).max() >= 1000                            # (not a test of zeros: 64 bins of 32767, gain 1 / 128, >> 4, is about 1024 at its peak)


@pytest.mark.parametrize("nb", [1, 2, 4, 6])
def test_interleaver_is_undone_by_the_oracles_deinterleaver(oracle, nb):
    n = 48 * nb
    for k in range(n):
        bits = np.zeros(n, np.uint8); bits[k] = 1
        sym = np.packbits(bits, bitorder="little")
        il = np.unpackbits(M.interleave(sym, nb), bitorder="little")
        assert il.sum() == 1
        assert np.array_equal(oracle.deinterleave(nb, il), bits), k
    assert sorted(M.interleave_map(nb)) == list(range(n))


def test_scrambler_register_and_tail():
    """all 8 bits of the seed are stored, bit 0 is never read; seeds 0 and 1 are the all-zero scrambler; TAIL_SCRAMBLE keeps two bits and advances the register"""
    x = np.random.default_rng(7).integers(0, 256, 300).astype(np.uint8)
    assert np.array_equal(M.scramble(x, 0x00), x) and np.array_equal(M.scramble(x, 0x01), x)
    assert np.array_equal(M.scramble(x, 0xFE), M.scramble(x, 0xFF)) and not np.array_equal(M.scramble(x, 0xFF), x)
    a, b = M.scramble(x, 0x5B), M.scramble(x, 0x5B, tail=100)
    assert b[100] == a[100] & 0xC0 and np.array_equal(np.delete(a, 100), np.delete(b, 100))
    assert np.array_equal(M.scramble(x, 0x5B, tail=300), a)
    mask = M.scramble(np.zeros(254, np.uint8), 0x5B)
    assert np.array_equal(mask[:127], mask[127:]) and len(set(mask[:127].tolist())) == 127    # period 127 bits = 127 bytes


def test_encoder_leaves_a_partial_burst_queued():
    x = np.random.default_rng(8).integers(0, 256, 301).astype(np.uint8)
    for cr, bin_ in ((M.CR_12, 1), (M.CR_23, 2), (M.CR_34, 3)):
        for ln in (1, 2, 3, 4, 5, 6, 7, 300, 301):
            y = M.conv_encode(x[:ln], cr)
            assert len(y) == ln // bin_ * (bin_ + 1)
            assert np.array_equal(y, M.conv_encode(x[:ln // bin_ * bin_], cr))
            assert np.array_equal(y, M.conv_encode(x, cr)[:len(y)])


def test_pilot_index_starts_at_127_and_wraps_at_127():
    car = np.zeros((300, 48, 2), np.int16)
    out = M.add_pilot(car)
    for j in range(300):
        idx = 127 if j == 0 else (j - 1) % 127
        p = -M.BPSK_MOD if M.PILOT_SGN[idx] else M.BPSK_MOD
        assert out[j, 7, 0] == p and out[j, 21, 0] == -p and out[j, 43, 0] == p and out[j, 57, 0] == p
    assert not out[:, :, 1].any() and not out[:, [0] + list(range(27, 38))].any()


def test_mapper_amplitudes():
    assert [M.MOD_OF[nb] for nb in (1, 2, 4, 6)] == [10720, 7581, 3390, 1654]
    for nb in (1, 2, 4, 6):
        sym = np.random.default_rng(nb).integers(0, 256, (8, 6 * nb)).astype(np.uint8)
        a = M.map11a(sym, nb).astype(np.int32)
        odd = (1 << max(nb // 2, 1)) - 1
        assert np.abs(a[..., 0]).max() == odd * M.MOD_OF[nb] and set(np.unique(np.abs(a[..., 0]) // M.MOD_OF[nb])) == set(range(1, odd + 1, 2))
        assert (nb == 1) == (not a[..., 1].any())


def test_44mhz_model_chain_equals_the_recorded_reference_frames():
    """tests/golden/reftx11a_44.npz: what CreatePreamble11a_44M + CreateModGraph11a_44M sent, rail frames included (the model upsamples the 16-bit stream), on the
    samples where the reference did not read behind its input"""
    z = np.load(os.path.join(ROOT, "tests", "golden", "reftx11a_44.npz"))
    n = len(z["rate"])
    assert n == 18
    for i in range(n):
        mpdu, rate, seed, tx40, tx44 = z["mpdu_%d" % i].tobytes(), int(z["rate"][i]), int(z["seed"][i]), z["tx40_%d" % i], z["tx44_%d" % i]
        assert np.array_equal(M.frame40(mpdu, rate, seed), tx40)
        got = M.frame44(mpdu, rate, seed)
        keep = compared(len(tx44))
        assert got.shape == tx44.shape and np.array_equal(got[keep], tx44[keep]), (i, rate)
