"""GPU 802.11n 2x2 transmitter (sora_hip_tx11n) against the reference modulator, sample for sample on both TX chains: the recorded
waveforms of tests/golden/refgraph_11n.npz, the live compiled graphs (ref_tx11n) where oracle/_ref is built, frames at any sample
offset, unsupported frames next to valid ones, batch independence, and the loop back through the GPU receiver."""
import os

import numpy as np
import pytest

from gpu_util import same_events_11n

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "refgraph_11n.npz")
# 2560: the FCS's second wave is empty; 2561, 2563: the first four bytes, which the CRC complements, straddle its two waves
LENS = [1, 2, 3, 4, 5, 37, 100, 151, 1000, 1500, 2560, 2561, 2563, 4092]
EXTRA = {8: 7, 10: 150, 14: 1}          # a length per MCS whose data field has the reference's extra symbol (MCS 9, 11, 12, 13 have none)


@pytest.fixture(scope="module")
def sora():
    import sora_amd
    if sora_amd.device_count() <= 0:
        pytest.skip("no HIP device")
    return sora_amd


@pytest.fixture(scope="module")
def graph():
    from oracle.pyoracle import ReferenceGraph
    g = ReferenceGraph()
    if not g.available():
        pytest.skip("oracle/_ref/libsora_refgraph.so not present")
    return g


def chains(sora, mpdus, mcs, seeds=None, gaps=None):
    o0, o1, off = sora.tx11n(mpdus, mcs, seeds, gaps=gaps)
    return o0.cpu().numpy(), o1.cpu().numpy(), off


def mixed_batch():
    rng = np.random.default_rng(1411)
    frames = []
    for mcs in range(8, 15):
        for ln in LENS + ([EXTRA[mcs]] if mcs in EXTRA else []):
            frames.append((rng.integers(0, 256, ln).astype(np.uint8).tobytes(), mcs))
    return frames


def test_recorded_frames_in_one_batch(sora):
    z = np.load(GOLD)
    mpdus = [z["mpdu%d" % k].tobytes() for k in range(4)]
    a, b, off = chains(sora, mpdus, [8, 9, 10, 12])
    for k in range(4):
        assert off[k + 1] - off[k] == len(z["tx%d_0" % k])
        assert np.array_equal(a[off[k]:off[k + 1]], z["tx%d_0" % k]), ("chain 0", k)
        assert np.array_equal(b[off[k]:off[k + 1]], z["tx%d_1" % k]), ("chain 1", k)


def test_mixed_batch_equals_the_live_reference_modulator(sora, graph):
    frames = mixed_batch()
    a, b, off = chains(sora, [m for m, _ in frames], [c for _, c in frames])
    for f, (mp, mcs) in enumerate(frames):
        w0, w1 = graph.tx11n(mp, mcs)
        assert off[f + 1] - off[f] == len(w0) == sora.tx11n_samples(len(mp), mcs)
        assert np.array_equal(a[off[f]:off[f + 1]], w0), ("chain 0", mcs, len(mp))
        assert np.array_equal(b[off[f]:off[f + 1]], w1), ("chain 1", mcs, len(mp))


def test_frames_at_sample_offsets_that_are_not_multiples_of_four(sora, graph):
    """The kernel stores four samples at a time where a frame starts on a 16-byte boundary and one at a time elsewhere: frames behind gaps
    of 1, 2, 3, 5 .. samples come out as the reference's, and the gaps stay untouched."""
    frames = mixed_batch()[::3]
    gaps = [(1, 2, 3, 5, 0, 7, 4, 6)[i % 8] for i in range(len(frames))]
    a, b, off = chains(sora, [m for m, _ in frames], [c for _, c in frames], gaps=gaps)
    for f, (mp, mcs) in enumerate(frames):
        w0, w1 = graph.tx11n(mp, mcs)
        s = off[f] + gaps[f]
        assert s + len(w0) == off[f + 1]
        assert not a[off[f]:s].any() and not b[off[f]:s].any(), f
        assert np.array_equal(a[s:off[f + 1]], w0) and np.array_equal(b[s:off[f + 1]], w1), (mcs, len(mp), gaps[f])


def loopback_capture(rng, s0, s1):
    """test_oracle_vs_refgraph.py's 2x2 recipe: 400 samples of silence, 10 % cross-talk, white noise of sigma 20."""
    n = (len(s0) + 1400) // 28 * 28
    a = np.zeros((n, 2)); b = np.zeros((n, 2))
    a[400:400 + len(s0)] = s0 + 0.1 * s1; b[400:400 + len(s0)] = s1 + 0.1 * s0
    a = np.clip(np.rint(a + rng.normal(0, 20, a.shape)), -32768, 32767).astype(np.int16)
    b = np.clip(np.rint(b + rng.normal(0, 20, b.shape)), -32768, 32767).astype(np.int16)
    return a, b


def test_loopback_through_the_gpu_receiver(sora):
    """MCS 8..10 decode to the exact MPDU (default and other scrambler seeds); MCS 11..14 are refused by the receiver's SIG parser, as the
    reference's own receiver refuses them (PLCP_HEADER_FAIL).  Where oracle/_ref is built, the events equal the reference receiver's."""
    import torch
    from oracle.pyoracle import ReferenceGraph
    g = ReferenceGraph()
    rng = np.random.default_rng(8011)
    plan = [(mcs, ln, sd) for mcs in range(8, 15) for ln, sd in ((60, None), (1000, 0x5D), (333, 0x01))]
    mpdus = [rng.integers(0, 256, ln).astype(np.uint8).tobytes() for _, ln, _ in plan]
    caps = []
    for (mcs, ln, sd), mp in zip(plan, mpdus):
        a, b, _ = chains(sora, [mp], [mcs], None if sd is None else [sd])
        caps.append(loopback_capture(rng, a, b))
    iq0 = np.concatenate([a for a, _ in caps]); iq1 = np.concatenate([b for _, b in caps])
    descs, o = [], 0
    for i, (a, _) in enumerate(caps):
        descs.append((o, len(a), i)); o += len(a)
    rx = sora.Rx11n(len(caps), len(iq0))
    rx.process_dev(torch.from_numpy(iq0).cuda(), torch.from_numpy(iq1).cuda(), descs)
    per = [[] for _ in caps]
    for r in rx.results():
        per[r["capture_id"]].append(r)
    for i, ((mcs, ln, sd), mp) in enumerate(zip(plan, mpdus)):
        ev = per[i]
        assert len(ev) == 1, (mcs, ln, sd, ev)
        if mcs <= 10:
            assert ev[0]["error_code"] == sora.E_FRAME_OK and ev[0]["rate_kbps"] == mcs, (mcs, ln, sd, hex(ev[0]["error_code"]))
            assert ev[0]["length"] == ln + 4 and ev[0]["mpdu"][:ln] == mp, (mcs, ln, sd)
        else:
            assert ev[0]["error_code"] == sora.E_PLCP_HEADER_FAIL, (mcs, ln, sd, hex(ev[0]["error_code"]))
        if g.available():
            ok, why = same_events_11n(ev, g.rx11n(*caps[i]), position="sample_index")
            assert ok, (mcs, ln, sd, why)


def test_unsupported_mcs_is_refused_and_leaves_its_output_untouched(sora, graph):
    import torch
    from sora_amd.capi import _dev_ptr
    for mcs in (7, 15):
        assert sora.tx11n_samples(100, mcs) == 0
        with pytest.raises(sora.SoraError):
            sora.tx11n([bytes(100)], [mcs])
    rng = np.random.default_rng(715)
    frames = [(rng.integers(0, 256, ln).astype(np.uint8).tobytes(), mcs) for ln, mcs in ((100, 9), (100, 7), (57, 14), (100, 15), (1, 8), (0, 9), (4093, 10))]
    room = 4000                                                    # every frame its own 4000-sample range (the valid ones need less)
    blob = np.zeros(sum(len(m) for m, _ in frames) + 4, np.uint8); off = []
    p = 0
    for m, _ in frames:
        off.append(p); blob[p:p + len(m)] = np.frombuffer(m, np.uint8); p += len(m)
    dev = torch.device("cuda", 0)
    t = lambda x, dt: torch.from_numpy(np.asarray(x, dt)).to(dev)
    d_blob, d_off = t(blob, np.uint8), t(off, np.int32)
    d_len, d_mcs = t([len(m) for m, _ in frames], np.int32), t([c for _, c in frames], np.int32)
    d_ooff = t([room * i for i in range(len(frames))], np.int64)
    o0 = torch.full((room * len(frames), 2), 0x5A5A, dtype=torch.int16, device=dev); o1 = o0.clone()
    rc = sora.load().sora_hip_tx11n(_dev_ptr(d_blob), _dev_ptr(d_off), _dev_ptr(d_len), _dev_ptr(d_mcs), None, len(frames),
                                    _dev_ptr(o0), _dev_ptr(o1), _dev_ptr(d_ooff), None)
    assert rc == 0
    torch.cuda.synchronize()
    a, b = o0.cpu().numpy(), o1.cpu().numpy()
    for f, (mp, mcs) in enumerate(frames):
        ra, rb = a[room * f:room * (f + 1)], b[room * f:room * (f + 1)]
        n = sora.tx11n_samples(len(mp), mcs)
        if n == 0:
            assert (ra == 0x5A5A).all() and (rb == 0x5A5A).all(), (mcs, len(mp))
        else:
            w0, w1 = graph.tx11n(mp, mcs)
            assert np.array_equal(ra[:n], w0) and np.array_equal(rb[:n], w1), (mcs, len(mp))
            assert (ra[n:] == 0x5A5A).all() and (rb[n:] == 0x5A5A).all(), (mcs, len(mp))


def test_a_batch_equals_its_frames_one_call_each(sora):
    """512 frames of random MCS, length and scrambler seed in one call = the same frames one call each: no state crosses frames."""
    rng = np.random.default_rng(512)
    mcs = [int(v) for v in rng.integers(8, 15, 512)]
    lens = [int(v) for v in rng.integers(1, 4093, 512)]
    seeds = [int(v) for v in rng.integers(0, 128, 512)]
    mpdus = [rng.integers(0, 256, ln).astype(np.uint8).tobytes() for ln in lens]
    a, b, off = chains(sora, mpdus, mcs, seeds)
    for f in range(512):
        x, y, o = chains(sora, [mpdus[f]], [mcs[f]], [seeds[f]])
        assert np.array_equal(a[off[f]:off[f + 1]], x) and np.array_equal(b[off[f]:off[f + 1]], y), (f, mcs[f], lens[f], seeds[f])
