"""GPU 802.11b transmitter with the short preamble (sora_hip_tx11b_pre) against tests/tx11b_model.py, sample for sample -- the model that
tests/test_11b_short_cpu.py pins to the reference's modulator at preamble 0 -- and, for the long preamble, against sora_hip_tx11b itself."""
import numpy as np
import pytest

import tx11b_model as txm

pytestmark = pytest.mark.gpu
SHORT_RATES = (2000, 5500, 11000)
# 1, 2, 3: the fewest bytes a workgroup's run can hold; 4092: 17 bytes per lane in the scans and several tiles per run
LENS = (1, 2, 3, 13, 14, 64, 257, 1500, 4092)


@pytest.fixture(scope="module")
def sora():
    import sora_amd
    if sora_amd.device_count() <= 0:
        pytest.skip("no HIP device")
    return sora_amd


@pytest.mark.parametrize("rate", SHORT_RATES)
def test_short_frames_equal_the_model(sora, rate):
    """every length from every one of the four last_phase values, in one call; phase_out is the model's"""
    rng = np.random.default_rng(1110 + rate)
    mpdus, pin = [], []
    for ln in LENS:
        mp = rng.integers(0, 256, ln).astype(np.uint8).tobytes()
        for p in range(4):
            mpdus.append(mp); pin.append(p)
    out, off, ph = sora.tx11b(mpdus, rate, pin, return_phase=True, preamble=1)
    out = out.cpu().numpy()
    for f, (mp, p) in enumerate(zip(mpdus, pin)):
        want, last = txm.tx11b(mp, rate, phase_in=p, preamble=1)
        assert off[f + 1] - off[f] == len(want) == sora.tx11b_samples(len(mp), rate, 1), (len(mp), p)
        assert np.array_equal(out[off[f]:off[f + 1]], want), (rate, len(mp), p)
        assert ph[f] == last, (rate, len(mp), p)


def _raw_call(sora, frames, ooff, out, kinds):
    """sora_hip_tx11b_pre straight: frames [(mpdu, rate, kind, phase_in)]; kinds False passes d_preamble = NULL"""
    import torch
    from sora_amd import capi
    dev = out.device
    lens = [len(m) for m, *_ in frames]
    moff = np.zeros(len(frames), np.int32); moff[1:] = np.cumsum([(l + 3) // 4 * 4 for l in lens])[:-1]
    blob = np.zeros(int(moff[-1]) + 4096, np.uint8)
    for m, o in zip(frames, moff):
        blob[o:o + len(m[0])] = np.frombuffer(m[0], np.uint8)
    d = lambda a, t: torch.from_numpy(np.asarray(a, t)).to(dev)
    d_blob, d_moff, d_len = d(blob, np.uint8), d(moff, np.int32), d(lens, np.int32)
    d_rate, d_kind, d_pin = d([f[1] for f in frames], np.int32), d([f[2] for f in frames], np.uint8), d([f[3] for f in frames], np.uint8)
    d_pout = torch.full((len(frames),), 0xEE, dtype=torch.uint8, device=dev)
    d_ooff = d(ooff, np.int64)
    rc = capi.load().sora_hip_tx11b_pre(capi._dev_ptr(d_blob), capi._dev_ptr(d_moff), capi._dev_ptr(d_len), capi._dev_ptr(d_rate),
                                        capi._dev_ptr(d_kind) if kinds else None, capi._dev_ptr(d_pin), capi._dev_ptr(d_pout), len(frames),
                                        capi._dev_ptr(out), capi._dev_ptr(d_ooff), capi._stream_ptr(None))
    assert rc == 0
    torch.cuda.synchronize()
    return d_pout.cpu().numpy()


def test_mixed_kinds_unaccepted_frames_and_odd_offsets(sora):
    """Long and short frames in one call at sample offsets that are no multiple of eight (no 16-byte stores); a 1 Mbps frame behind a short
    preamble, a frame of length 0 and a kind of 7 between them: their ranges, their phase_out and every gap stay as they were."""
    import torch
    rng = np.random.default_rng(1120)
    mk = lambda n: rng.integers(0, 256, n).astype(np.uint8).tobytes()
    frames = [(mk(5), 11000, 1, 0), (mk(10), 1000, 1, 1), (mk(7), 2000, 0, 3), (b"", 5500, 1, 0), (mk(3), 5500, 1, 2), (mk(9), 11000, 7, 0),
              (mk(2), 1000, 0, 1), (mk(300), 2000, 1, 3)]
    valid = [txm.samples(len(m), r, k) for m, r, k, _ in frames]
    assert [v > 0 for v in valid] == [True, False, True, False, True, False, True, True]
    room = [v if v else 5000 for v in valid]
    ooff, at = [], 3
    for n in room:
        ooff.append(at); at += n + 11
    out = torch.full((at + 64, 2), 0x55, dtype=torch.int8, device="cuda:0")
    pout = _raw_call(sora, frames, ooff, out, True)
    got = out.cpu().numpy()
    touched = np.zeros(len(got), bool)
    for f, (m, r, k, p) in enumerate(frames):
        if not valid[f]:
            assert pout[f] == 0xEE, f
            continue
        want, last = txm.tx11b(m, r, phase_in=p, preamble=k)
        assert np.array_equal(got[ooff[f]:ooff[f] + len(want)], want), f
        assert pout[f] == last, f
        touched[ooff[f]:ooff[f] + len(want)] = True
    assert (got[~touched] == 0x55).all() and (~touched).sum() > 3 * 5000


def test_all_long_is_sora_hip_tx11b_byte_for_byte(sora):
    """preamble None (sora_hip_tx11b), a kind array of zeros and d_preamble = NULL: one output, all four rates, frames up to 4092 bytes"""
    import torch
    rng = np.random.default_rng(1121)
    frames = [(rng.integers(0, 256, ln).astype(np.uint8).tobytes(), rate, 0, int(rng.integers(0, 4))) for rate in (1000, 2000, 5500, 11000) for ln in (1, 2, 14, 257, 4092)]
    mp, rates, pin = [f[0] for f in frames], [f[1] for f in frames], [f[3] for f in frames]
    base, off, ph = sora.tx11b(mp, rates, pin, return_phase=True)
    zeros, off0, ph0 = sora.tx11b(mp, rates, pin, return_phase=True, preamble=0)
    assert off == off0 and ph == ph0 and torch.equal(base, zeros)
    null = torch.full_like(base, 0x55)
    pout = _raw_call(sora, frames, off[:-1], null, False)
    assert torch.equal(base, null) and [int(v) for v in pout] == ph
    assert off[-1] == sum(sora.tx11b_samples(len(m), r) for m, r in zip(mp, rates))
