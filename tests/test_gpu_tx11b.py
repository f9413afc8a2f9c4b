"""GPU 802.11b transmitter (sora_hip_tx11b) against the reference modulator, sample for sample: the 12 recorded frames of
tests/golden/refgraph_11b*.npz with the phase each one started from, the live compiled graph (ref_tx11b) where oracle/_ref is built,
calls chained through last_phase as one reference process chains its frames, frames at any sample offset, unsupported frames next to
valid ones, batch independence, and the loop back through the GPU receiver."""
import numpy as np
import pytest

from test_tx11b_cpu import recorded_frames, ref_tx11b, start_parity

pytestmark = pytest.mark.gpu
RATES = (1000, 2000, 5500, 11000)
# 2560: the FCS's second wave is empty; 2561, 2563: the first four bytes, which the CRC complements, straddle its two waves
LENS = [1, 2, 3, 4, 5, 6, 10, 14, 37, 100, 255, 1000, 1500, 2560, 2561, 2563]


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


def frames_of(sora, mpdus, rates, phase_in=None, gaps=None):
    out, off, ph = sora.tx11b(mpdus, rates, phase_in, gaps=gaps, return_phase=True)
    return out.cpu().numpy(), off, ph


def test_recorded_frames_in_one_batch(sora):
    """All 12 recordings in one call, each from the parity it started with; within a recording, the last_phase frame k leaves
    behind is the one frame k + 1 started from."""
    rec = recorded_frames()
    pin = [start_parity(s) for *_, s in rec]
    out, off, ph = frames_of(sora, [mp for _, _, _, mp, _ in rec], [r for _, _, r, _, _ in rec], pin)
    for f, (name, k, rate, mp, s) in enumerate(rec):
        assert off[f + 1] - off[f] == len(s), (name, k)
        assert np.array_equal(out[off[f]:off[f + 1]], s), (name, k, rate, len(mp))
        if f + 1 < len(rec) and rec[f + 1][0] == name:
            assert ph[f] & 1 == pin[f + 1], (name, k)


def live_batch(rng):
    frames = []
    for rate in RATES:
        for ln in LENS:
            frames.append((rng.integers(0, 256, ln).astype(np.uint8).tobytes(), rate))
    frames += [(rng.integers(0, 256, 4092).astype(np.uint8).tobytes(), r) for r in RATES]
    return frames


def test_mixed_batch_equals_the_live_reference_modulator(sora, graph):
    """Every rate, many lengths (4092 bytes included), both start parities; the reference's own start state is read from its first
    samples, and the last_phase the GPU reports is the one the reference's next frame starts from."""
    rng = np.random.default_rng(1104)
    frames = live_batch(rng)
    want = [ref_tx11b(graph, mp, rate) for mp, rate in frames]        # one reference process, in this order
    pin = [start_parity(w) for w in want]
    assert 0 in pin and 1 in pin
    out, off, ph = frames_of(sora, [m for m, _ in frames], [r for _, r in frames], pin)
    for f, (mp, rate) in enumerate(frames):
        assert off[f + 1] - off[f] == len(want[f]) == sora.tx11b_samples(len(mp), rate)
        assert np.array_equal(out[off[f]:off[f + 1]], want[f]), (rate, len(mp), pin[f])
        if f + 1 < len(frames):
            assert ph[f] & 1 == pin[f + 1], (f, rate, len(mp))


def test_chained_calls_reproduce_a_sequence_of_reference_calls(sora, graph):
    """phase_in of each call = phase_out of the call before: a run of single-frame calls is one reference process."""
    rng = np.random.default_rng(1105)
    seq = [(rng.integers(0, 256, int(ln)).astype(np.uint8).tobytes(), int(r))
           for ln, r in zip(rng.integers(1, 700, 24), rng.choice(RATES, 24))]
    want = [ref_tx11b(graph, mp, rate) for mp, rate in seq]
    phase = start_parity(want[0])
    for f, (mp, rate) in enumerate(seq):
        out, off, ph = frames_of(sora, [mp], [rate], [phase])
        assert np.array_equal(out, want[f]), (f, rate, len(mp), phase)
        phase = ph[0]


def test_frames_at_sample_offsets_that_are_not_multiples_of_eight(sora):
    """The kernel stores eight samples at a time where a frame starts on a 16-byte boundary and two bytes at a time elsewhere: frames
    behind gaps of 1 .. 7 samples come out as they do alone, and the gaps stay untouched."""
    rng = np.random.default_rng(1106)
    frames = live_batch(rng)[::3]
    gaps = [(1, 2, 3, 5, 0, 7, 4, 6, 8, 9)[i % 10] for i in range(len(frames))]
    out, off, _ = frames_of(sora, [m for m, _ in frames], [r for _, r in frames], gaps=gaps)
    for f, (mp, rate) in enumerate(frames):
        alone, _, _ = frames_of(sora, [mp], [rate])
        s = off[f] + gaps[f]
        assert s + len(alone) == off[f + 1]
        assert not out[off[f]:s].any(), f
        assert np.array_equal(out[s:off[f + 1]], alone), (rate, len(mp), gaps[f])


def test_unsupported_frames_are_refused_and_leave_their_output_untouched(sora, graph):
    import torch
    from sora_amd.capi import _dev_ptr
    rng = np.random.default_rng(1107)
    frames = [(rng.integers(0, 256, ln).astype(np.uint8).tobytes(), rate)
              for ln, rate in ((100, 2000), (100, 6000), (57, 11000), (100, 0), (1, 5500), (0, 1000), (4093, 11000), (30, 1000))]
    room = 60000                                                   # every frame its own range (the valid ones need less)
    blob = np.zeros(sum(len(m) for m, _ in frames) + 4, np.uint8); off = []
    p = 0
    for m, _ in frames:
        off.append(p); blob[p:p + len(m)] = np.frombuffer(m, np.uint8); p += len(m)
    want = [ref_tx11b(graph, mp, rate) if sora.tx11b_samples(len(mp), rate) else None for mp, rate in frames]
    pin = [start_parity(w) if w is not None else 0 for w in want]
    dev = torch.device("cuda", 0)
    t = lambda x, dt: torch.from_numpy(np.asarray(x, dt)).to(dev)
    d_blob, d_off = t(blob, np.uint8), t(off, np.int32)
    d_len, d_rate = t([len(m) for m, _ in frames], np.int32), t([r for _, r in frames], np.int32)
    d_pin, d_pout = t(pin, np.uint8), torch.full((len(frames),), 0xEE, dtype=torch.uint8, device=dev)
    d_ooff = t([room * i for i in range(len(frames))], np.int64)
    o = torch.full((room * len(frames), 2), 0x5A, dtype=torch.int8, device=dev)
    rc = sora.load().sora_hip_tx11b(_dev_ptr(d_blob), _dev_ptr(d_off), _dev_ptr(d_len), _dev_ptr(d_rate), _dev_ptr(d_pin), _dev_ptr(d_pout),
                                    len(frames), _dev_ptr(o), _dev_ptr(d_ooff), None)
    assert rc == 0
    torch.cuda.synchronize()
    a, pout = o.cpu().numpy(), d_pout.cpu().numpy()
    for f, (mp, rate) in enumerate(frames):
        r = a[room * f:room * (f + 1)]
        if want[f] is None:
            assert (r == 0x5A).all() and pout[f] == 0xEE, (rate, len(mp))
        else:
            n = len(want[f])
            assert np.array_equal(r[:n], want[f]) and (r[n:] == 0x5A).all() and pout[f] <= 3, (rate, len(mp))


def test_a_batch_equals_its_frames_one_call_each(sora):
    """300 frames of random rate, length and start phase in one call = the same frames one call each: no state crosses frames."""
    rng = np.random.default_rng(300)
    rates = [int(v) for v in rng.choice(RATES, 300)]
    lens = [int(v) for v in rng.integers(1, 4093, 300)]
    pin = [int(v) for v in rng.integers(0, 4, 300)]
    mpdus = [rng.integers(0, 256, ln).astype(np.uint8).tobytes() for ln in lens]
    out, off, ph = frames_of(sora, mpdus, rates, pin)
    for f in range(0, 300, 7):
        x, _, p = frames_of(sora, [mpdus[f]], [rates[f]], [pin[f]])
        assert np.array_equal(out[off[f]:off[f + 1]], x) and p[0] == ph[f], (f, rates[f], lens[f], pin[f])
    # and the order of the batch does not matter
    perm = rng.permutation(300)
    out2, off2, ph2 = frames_of(sora, [mpdus[i] for i in perm], [rates[i] for i in perm], [pin[i] for i in perm])
    for j, i in enumerate(perm):
        assert np.array_equal(out2[off2[j]:off2[j + 1]], out[off[i]:off[i + 1]]) and ph2[j] == ph[i], (i, j)


def test_loopback_through_the_gpu_receiver(sora):
    """GPU frames at every rate through test_oracle_11b's channel into sora_amd.Rx11b: the MPDUs come back with the FCS OK, and the
    receiver reports what the oracle's receiver (oracle/so_rx11b.c) reports for the same captures."""
    import torch
    from oracle.pyoracle import Oracle
    from test_oracle_11b import channel_11b
    rng = np.random.default_rng(1108)
    plan = [(rate, ln) for rate in RATES for ln in (1, 60, 333, 1500)]
    mpdus = [rng.integers(0, 256, ln).astype(np.uint8).tobytes() for _, ln in plan]
    out, off, _ = frames_of(sora, mpdus, [r for r, _ in plan], [f & 1 for f in range(len(plan))])
    # channel seeds: 500 + f, except frame 5, whose capture of seed 505 loses the SFD in the noise (SFD_TIMEOUT in both receivers)
    caps = [channel_11b(out[off[f]:off[f + 1]], 605 if f == 5 else 500 + f) for f in range(len(plan))]
    descs, parts, pos = [], [], 0
    for i, c in enumerate(caps):
        descs.append((pos, len(c), i)); parts.append(c); pos += len(c)
    iq = np.concatenate(parts)
    rx = sora.Rx11b(len(caps), len(iq), max_frames_per_capture=16)
    rx.process_dev(torch.from_numpy(iq).cuda(), descs)
    per = [[] for _ in caps]
    for r in rx.results():
        per[r["capture_id"]].append(r)
    rx.close()
    o = Oracle()
    key = lambda r: (r["error_code"], r["end_sample"], r["mpdu"])
    for i, ((rate, ln), mp) in enumerate(zip(plan, mpdus)):
        ok = [r for r in per[i] if r["error_code"] == sora.E_FRAME_OK]
        assert ok, (rate, ln, [hex(r["error_code"]) for r in per[i]])
        assert ok[0]["rate_kbps"] == rate and ok[0]["length"] == ln + 4 and ok[0]["mpdu"][:ln] == mp, (rate, ln)
        assert [key(r) for r in per[i]] == [key(r) for r in o.rx11b_capture(caps[i])], (rate, ln)
