"""The index arithmetic of the 802.11a symbol chain (k_frame, k_sym_front / k_track_lds / k_sym_back, k_pipe: the pieces of dev_sym11a.h) at its edges.

sora_amd.Rx on 1, 3, 4 and 5 captures -- k_frame's workgroup holds four frames: a partial one, a full one, and one more -- at 6, 12, 24 and 54 Mbps
(every modulation), with payload lengths whose symbol counts are congruent to 0, 1, 2 and 3 modulo 4 (a wave takes four symbols per pass: the last
pass's remainder).  Every capture is placed so that its frame ends on the LAST sample of its capture, and the last capture ends the sample buffer:
whatever a wave loads for the symbols its last pass does not have must not reach past the frame.  Result rows and MPDU bytes are the oracle's,
with the library choosing the kernels (front 0), with k_frame (1) and with the three-kernel form (3)."""
import numpy as np
import pytest

from gpu_util import same_results

pytestmark = pytest.mark.gpu

# (rate, payload bytes, symbols): for each rate one length per residue of the symbol count modulo 4, chosen among those whose frame the receive chain completes
# on the capture's last sample (the chain takes its samples in bursts of 14: with some leads the burst that completes the frame lies past the frame's end)
FRAMES = [(6000, 39, 16), (6000, 42, 17), (6000, 45, 18), (6000, 48, 19), (12000, 60, 12), (12000, 42, 9), (12000, 48, 10), (12000, 54, 11),
          (24000, 30, 4), (24000, 42, 5), (24000, 102, 10), (24000, 114, 11), (54000, 75, 4), (54000, 102, 5), (54000, 30, 2), (54000, 48, 3)]
_MADE = {}


def capture_ending_with_its_frame(o, rate, length):
    """20 MHz capture, a whole number of 14-sample bursts, whose last sample is the frame's last"""
    rng = np.random.default_rng(length)
    mp = rng.integers(0, 256, length).astype(np.uint8).tobytes()
    x = o.tx_capture(mp, rate, seed=1 + length % 127, lead=0, tail=0)
    lead20 = (-(len(x) // 2)) % 14 + 28
    return np.concatenate([np.zeros((2 * lead20, 2), np.int16), x])[::2].copy()


def made(o):
    """the sixteen captures and the oracle's rows for each, once"""
    if not _MADE:
        caps = [capture_ending_with_its_frame(o, rate, length) for rate, length, _ in FRAMES]
        rows = [o.rx_capture(c, 20) for c in caps]
        for (rate, length, nsym), c, r in zip(FRAMES, caps, rows):
            assert len(c) % 14 == 0 and len(r) == 1, (rate, length)
            assert (r[0]["error_code"], r[0]["rate_kbps"], r[0]["length"], r[0]["nsym"], r[0]["end_sample"]) == (1, rate, length + 4, nsym, len(c)), (rate, length, r[0])
        assert {(rate, nsym % 4) for rate, _, nsym in FRAMES} == {(rate, k) for rate in (6000, 12000, 24000, 54000) for k in range(4)}
        _MADE["caps"], _MADE["rows"] = caps, rows
    return _MADE["caps"], _MADE["rows"]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.mark.parametrize("front", (0, 1, 3))
@pytest.mark.parametrize("ncaps", (1, 3, 4, 5))
def test_frames_that_end_their_capture(oracle, torch_cuda, ncaps, front):
    import sora_amd
    torch = torch_cuda
    caps, rows = made(oracle)
    rx = sora_amd.Rx(ncaps, sum(sorted(len(c) for c in caps)[-ncaps:]) + 4 * ncaps, sample_rate_mhz=20)
    rx.set_front(front)
    for start in range(0, len(caps), ncaps):                                  # every one of the sixteen frames, ncaps at a time
        pick = [(start + i) % len(caps) for i in range(ncaps)]
        descs, parts, off = [], [], 0
        for i, k in enumerate(pick):
            pad = (-off) % 4                                                   # captures start at multiples of four samples
            parts.append(np.zeros((pad, 2), np.int16)); off += pad
            descs.append((off, len(caps[k]), i)); parts.append(caps[k]); off += len(caps[k])
        iq = np.concatenate(parts)                                             # (the last capture's last sample is the buffer's last)
        assert len(iq) == descs[-1][0] + descs[-1][1]
        rx.process_dev(torch.from_numpy(iq).to("cuda:0"), descs)
        got = rx.results()
        if front:
            assert rx.call_front() == front
        want = []
        for i, k in enumerate(pick):
            for r in rows[k]:
                r = dict(r); r["capture_id"] = i; want.append(r)
        ok, why = same_results(got, want)
        assert ok, "front %d, captures %s: %s" % (front, [FRAMES[k] for k in pick], why)
