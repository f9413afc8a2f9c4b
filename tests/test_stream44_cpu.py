"""The premise of stream mode at 44 MHz (sora_rx_set_stream_mode with sample_rate_mhz = 44, include/sora_hip.h): TDownSample44_40 is
periodic.  308 source samples (11 RX_BLOCKs) give exactly 280 resampled samples and leave the brick empty, so a 44 MHz stream cut at
multiples of 308 and resampled piece by piece gives the uncut stream's resampled samples bit for bit.  Cuts elsewhere do not.  No GPU needed."""
import numpy as np

from gpu_util import random_capture, source_position_44, upsample_40_to_44
from test_oracle_ingest import make_dump


def _stream44(oracle, rng, ncaps):
    x = np.concatenate([upsample_40_to_44(random_capture(oracle, rng, 40)) for _ in range(ncaps)])
    return np.ascontiguousarray(x[:len(x) // 28 * 28])


def _resamplers(oracle):
    from oracle.pyoracle import Reference
    out = [("oracle", oracle.down44to40)]
    ref = Reference()
    if ref.available():                                                  # the reference's own Down44to40, where oracle/_ref is built
        out.append(("reference", ref.down44to40))
    return out


def _piecewise(down, x, cuts):
    return np.concatenate([down(x[a:b]) for a, b in zip([0] + cuts[:-1], cuts)])


def test_cuts_on_the_resampler_period_reproduce_the_uncut_stream(oracle):
    rng = np.random.default_rng(4404)
    for trial in range(6):
        x = _stream44(oracle, rng, 3)
        n = len(x) // 308 * 308
        x = x[:n]
        for name, down in _resamplers(oracle):
            whole = down(x)
            assert len(whole) == n * 10 // 11
            inner = sorted(set(int(c) * 308 for c in rng.integers(1, n // 308, size=4)))
            got = _piecewise(down, x, inner + [n])
            assert np.array_equal(got, whole), (name, trial, inner)
            for k in (924, 5236, 7700):                                  # the cuts of the issue
                if k < n:
                    assert np.array_equal(_piecewise(down, x, [k, n]), whole), (name, k)


def test_cuts_off_the_period_do_not(oracle):
    rng = np.random.default_rng(4405)
    x = _stream44(oracle, rng, 2)
    n = len(x) // 308 * 308
    x = x[:n]
    for name, down in _resamplers(oracle):
        whole = down(x)
        for k in (140, 336, 28 * 12, 308 * 3 + 28):                      # RX_BLOCK boundaries (multiples of 28), not of 308
            got = _piecewise(down, x, [k, n])
            assert not (len(got) == len(whole) and np.array_equal(got, whole)), (name, k)


def test_source_position_44_is_periodic():
    for e in list(range(0, 600, 2)) + [1234, 5678, 99990]:
        for k in (1, 2, 7, 100):
            assert source_position_44(e + 140 * k) == source_position_44(e) + 308 * k, (e, k)
    assert source_position_44(0) == 0 and source_position_44(140) == 308


def test_dump_layout_rule_gives_each_piece_its_own_resampled_samples(oracle):
    """Several pieces in one RX_BLOCK dump, each starting a multiple of 11 blocks in (zero blocks as padding): ingesting the whole dump puts
    piece j's samples at (first block / 11) * 280, and the first ingest_count(piece bytes) of them are what the piece gives on its own."""
    import sora_amd
    flags = sora_amd.INGEST_RXBLOCK | sora_amd.INGEST_44TO40
    rng = np.random.default_rng(4406)
    pieces = [_stream44(oracle, rng, 1)[:28 * int(rng.integers(1, 200))] for _ in range(4)]
    blocks, firsts = [], []
    nb = 0
    for p in pieces:
        d = make_dump(p, raw14=False).reshape(-1, 128)
        firsts.append(nb)
        pad = (-len(d)) % 11
        blocks += [d, np.zeros((pad, 128), np.uint8)]
        nb += len(d) + pad
    dump = np.concatenate(blocks).reshape(-1)
    whole = oracle.down44to40(oracle.load_dump(dump.tobytes()))
    for p, f in zip(pieces, firsts):
        own = oracle.down44to40(p)
        n = sora_amd.ingest_count(len(p) // 28 * 128, flags)
        assert n == len(own) // 28 * 28 and f % 11 == 0
        off = f // 11 * 280
        assert np.array_equal(whole[off:off + n], own[:n])
