"""GPU 40 MHz HT 2x2 transmitter in JOINT coding (sora_hip_tx_ht40_joint, k_tx_ht40_joint): sample for sample the integer model
tests/ht40_joint_model.py::frame_int_joint (itself held to the float model of the format by tests/test_ht40_joint_model.py) on both chains, for every MCS at lengths
on both sides of a symbol step, the shortest and the longest frame, any sample offset and seed; nothing written outside accepted frames; frames of a batch
independent.  Then the loop-back: what it sends comes back through the receive handle in joint coding -- the descriptor form, the raw-capture form, and stream mode
cut at random source calls -- and a handle left in per-stream coding does NOT return it: the handle's coding decides, not the frame."""
import numpy as np
import pytest

from oracle import py_ht40 as m
import ht40_joint_model as J
import tx_ht40_model as T

pytestmark = pytest.mark.gpu

GAIN = 250.0 * 128.0 / T.A                                              # the level at which the receiver's own tests are known to decode
SENTINEL = 0x5A5A
FRAME_OK = 1


@pytest.fixture(scope="module")
def env():
    import torch
    import sora_amd
    if sora_amd.device_count() <= 0:
        pytest.skip("no HIP device")
    return torch, sora_amd


def _mpdu(rng, ln):
    return rng.integers(0, 256, ln, dtype=np.uint8).tobytes()


def _step(mcs, n):
    """the longest MPDU (without FCS) of n data symbols in joint coding; one byte more takes n + 1"""
    return (n * J.ndbps(*m.MCS2[mcs]) - 22) // 8 - 4


@pytest.fixture(scope="module")
def batch(env, oracle):
    """one batch for the exactness tests: (frames (mcs, len, seed), MPDUs, model waveforms), the model computed once"""
    rng = np.random.default_rng(6060)
    frames = []
    for mcs in range(8, 15):
        n = 2 + mcs % 3
        for ln in (_step(mcs, n), _step(mcs, n) + 1):
            assert J.nsym_for(ln + 4, *m.MCS2[mcs]) == (n if ln == _step(mcs, n) else n + 1)
            frames.append((mcs, ln, int(rng.integers(1, 128))))
    for k, ln in enumerate((1, 2, 37, 333)):
        frames.append((8 + (3 * k) % 7, ln, int(rng.integers(1, 128))))
    frames.append((13, 1, 0xDD))                                       # bit 7 set: only seven bits count
    frames.append((13, 3996, 0x11))                                    # 32832 field bits: the largest bit field (1026 generator words, 4108 field bytes)
    frames.append((14, 3996, 0x7F))
    frames.append((8, 3996, 0x5D))                                     # 297 data symbols, the longest frame there is
    frames.append((11, 700, 0))                                        # an all-zero seed: the scrambler stays silent
    for mcs, ln in ((9, 2561), (12, 2563)):                            # the first four bytes, which the CRC complements, straddle the FCS's two waves
        frames.append((mcs, ln, int(rng.integers(1, 128))))
    mp = [_mpdu(rng, ln) for _, ln, _ in frames]
    want = [J.frame_int_joint_nofcs(a, mcs, seed, oracle=oracle) for (mcs, _, seed), a in zip(frames, mp)]
    return frames, mp, want


def _run(env, frames, mp, gaps, seeds="given", fill=0):
    """-> (out0, out1 as int16 numpy [total, 2], first samples, sample counts) through the C entry point on sentinel-filled outputs"""
    torch, sora = env
    from sora_amd.capi import _dev_ptr
    n = len(frames)
    lens = [ln for _, ln, _ in frames]
    off = np.zeros(n + 1, np.int64); np.cumsum([(max(ln, 1) + 3) // 4 * 4 for ln in lens], out=off[1:])
    blob = np.zeros(max(int(off[-1]), 4), np.uint8)
    for f in range(n):
        blob[off[f]:off[f] + min(lens[f], len(mp[f]))] = np.frombuffer(mp[f][:lens[f]], np.uint8)
    ns = [sora.tx_ht40_joint_samples(ln, mcs) or 1440 for mcs, ln, _ in frames]   # a refused frame keeps a range of its own, to be found untouched
    first = np.zeros(n, np.int64); pos = 0
    for f in range(n):
        first[f] = pos + gaps[f]; pos = first[f] + ns[f]
    total = pos + 8
    dev = torch.device("cuda")
    d = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)
    o0 = torch.full((total, 2), fill, dtype=torch.int16, device=dev); o1 = torch.full((total, 2), fill, dtype=torch.int16, device=dev)
    d_seed = d([sd for _, _, sd in frames], np.uint8) if seeds == "given" else None
    args = (d(blob, np.uint8), d(off[:-1], np.int32), d(lens, np.int32), d([mcs for mcs, _, _ in frames], np.int32), d(first, np.int64))
    rc = sora.load().sora_hip_tx_ht40_joint(_dev_ptr(args[0]), _dev_ptr(args[1]), _dev_ptr(args[2]), _dev_ptr(args[3]), _dev_ptr(d_seed) if d_seed is not None else None,
                                            n, _dev_ptr(o0), _dev_ptr(o1), _dev_ptr(args[4]), None)
    assert rc == 0, sora.load().sora_hip_last_error()
    torch.cuda.synchronize()
    return o0.cpu().numpy(), o1.cpu().numpy(), first, ns


def _first_difference(got, want):
    bad = np.nonzero((got != want).any(axis=1))[0]
    return None if len(bad) == 0 else (int(bad[0]), len(bad), got[bad[0]].tolist(), want[bad[0]].tolist())


def test_sample_exact_against_the_integer_model(env, batch):
    frames, mp, want = batch
    gaps = [(5 * f + 1) % 11 for f in range(len(frames))]              # first samples at every residue mod 4
    o0, o1, first, ns = _run(env, frames, mp, gaps, fill=SENTINEL)
    assert {int(v) % 4 for v in first} == {0, 1, 2, 3}
    for f, (mcs, ln, seed) in enumerate(frames):
        assert ns[f] == want[f].shape[1], (f, mcs, ln)
        for ch, o in enumerate((o0, o1)):
            got = o[first[f]:first[f] + ns[f]]
            assert _first_difference(got, want[f][ch]) is None, (f, mcs, ln, seed, ch, int(first[f]) % 4, _first_difference(got, want[f][ch]))
    keep = np.ones(len(o0), bool)                                      # ... and nothing outside the frames
    for f in range(len(frames)):
        keep[first[f]:first[f] + ns[f]] = False
    assert keep.sum() >= len(frames) and (o0[keep] == SENTINEL).all() and (o1[keep] == SENTINEL).all()


def test_default_seed_is_0x5d(env, oracle):
    rng = np.random.default_rng(21)
    frames = [(12, 90, 0x5D), (9, 41, 0x5D)]
    mp = [_mpdu(rng, ln) for _, ln, _ in frames]
    a0, a1, first, ns = _run(env, frames, mp, [0, 2], seeds=None)
    b0, b1, _, _ = _run(env, frames, mp, [0, 2], seeds="given")
    assert np.array_equal(a0, b0) and np.array_equal(a1, b1)
    w = J.frame_int_joint_nofcs(mp[0], 12, oracle=oracle)              # the model's default
    assert J.SEED == 0x5D and np.array_equal(a0[:ns[0]], w[0]) and np.array_equal(a1[:ns[0]], w[1])


def test_frames_that_are_not_accepted_leave_their_range_untouched(env, oracle):
    rng = np.random.default_rng(22)
    frames = [(10, 60, 3), (7, 60, 3), (9, 25, 9), (15, 60, 3), (11, 0, 1), (14, 100, 7), (12, 3997, 1), (8, 9, 4)]
    mp = [_mpdu(rng, max(ln, 4)) for _, ln, _ in frames]
    o0, o1, first, ns = _run(env, frames, mp, [3, 0, 1, 6, 0, 2, 0, 5], fill=SENTINEL)
    good = np.zeros(len(o0), bool)
    for f, (mcs, ln, seed) in enumerate(frames):
        if mcs in m.MCS2 and 1 <= ln <= 3996:
            w = J.frame_int_joint_nofcs(mp[f][:ln], mcs, seed, oracle=oracle)
            assert np.array_equal(o0[first[f]:first[f] + ns[f]], w[0]) and np.array_equal(o1[first[f]:first[f] + ns[f]], w[1]), (f, mcs, ln)
            good[first[f]:first[f] + ns[f]] = True
    assert good.sum() == sum(ns[f] for f in (0, 2, 5, 7))
    assert (o0[~good] == SENTINEL).all() and (o1[~good] == SENTINEL).all()


def test_frames_of_a_batch_are_independent(env):
    """the same frame first, in the middle and last of a batch of different frames: identical samples"""
    torch, sora = env
    rng = np.random.default_rng(23)
    a = _mpdu(rng, 611)
    others = [(8 + k % 7, int(rng.integers(1, 900))) for k in range(30)]
    mk = lambda part: [_mpdu(rng, ln) for _, ln in part]
    mps = [a] + mk(others[:15]) + [a] + mk(others[15:]) + [a]
    mcs = [13] + [v for v, _ in others[:15]] + [13] + [v for v, _ in others[15:]] + [13]
    seeds = [0x31] + [1 + k for k in range(15)] + [0x31] + [40 + k for k in range(15)] + [0x31]
    o0, o1, off = sora.tx_ht40_joint(mps, mcs, seeds)
    o0, o1 = o0.cpu().numpy(), o1.cpu().numpy()
    n = sora.tx_ht40_joint_samples(611, 13)
    cut = lambda o, f: o[off[f]:off[f] + n]
    assert off[1] - off[0] == n and np.abs(cut(o0, 0).astype(int)).max() > 1000
    for f in (16, 32):
        assert np.array_equal(cut(o0, 0), cut(o0, f)) and np.array_equal(cut(o1, 0), cut(o1, f)), f


# ------------------------------------------------------------------ loop-back
def _nsoft(specs):
    return sum(2 * (J.nsym_for(ln + 4, *m.MCS2[mcs]) * 108 * m.MCS2[mcs][0] + 64) for mcs, ln in specs)


@pytest.mark.parametrize("cfo_step", [0.0, 37.0])
def test_loopback_through_the_descriptor_call(env, cfo_step):
    """GPU-sent joint frames through py_ht40.channel (2x2 cross-talk, sigma 6, a carrier offset the descriptor names) into sora_ht40_process_dev in joint coding"""
    torch, sora = env
    rng = np.random.default_rng(626 + int(cfo_step))
    flat = [(mcs, ln) for mcs in range(8, 15) for ln in (int(rng.integers(1, 60)), int(rng.integers(100, 1200)))]
    mp = [_mpdu(rng, ln) for _, ln in flat]
    o0, o1, off = sora.tx_ht40_joint(mp, [mcs for mcs, _ in flat], [int(rng.integers(1, 128)) for _ in flat])
    x = np.stack([o.cpu().numpy().astype(float) for o in (o0, o1)])
    x = x[..., 0] + 1j * x[..., 1]
    H = np.array([[1.0 * np.exp(0.3j), 0.35 * np.exp(-1.1j)], [0.3 * np.exp(2.0j), 0.9 * np.exp(-0.4j)]])
    segs, descs, pos = [], [], 0
    for f, (mcs, ln) in enumerate(flat):
        nb, cr = m.MCS2[mcs]
        y = m.channel(x[:, off[f] + 1280:off[f + 1]], H, 6.0, rng, scale=GAIN, cfo_step=cfo_step, lead=64)      # from HT-LTF 1 on: its sample counts from 0
        segs.append(y); descs.append((pos + 64, nb, cr, ln + 4, 0, -int(cfo_step), 0.0, f)); pos += y.shape[1]
    iq = np.concatenate(segs + [np.zeros((2, 256, 2), np.int16)], axis=1)
    rx = sora.RxHt40(len(descs), _nsoft(flat))
    rx.set_coding(sora.HT40_CODING_JOINT)
    rx.process_dev(torch.from_numpy(iq[0].copy()).cuda(), torch.from_numpy(iq[1].copy()).cuda(), descs, None)
    res = rx.results(); rx.close()
    assert len(res) == len(flat)
    for f, r in enumerate(res):
        assert (r["capture_id"], r["stream"], r["error_code"], r["mpdu"]) == (f, 0, FRAME_OK, m.add_fcs(mp[f])), (flat[f], hex(r["error_code"]))


def _captures(env, rng, specs, cfo_step, joint=True, tail=800):
    """specs: per capture a list of (mcs, len).  One batch from the GPU transmitter (joint, or per-stream frames carrying the MPDU on both streams), per frame H with
    random phases x GAIN, a carrier offset, a lead of 300..900 zero samples; per capture `tail` trailing zeros, noise of sigma 8, whole 28-sample bursts.
    -> (iq int16 numpy [2, n, 2], capture descriptors, truth per capture [(mcs, psdu)])"""
    torch, sora = env
    geo = np.random.default_rng(int(rng.integers(1 << 30)))            # channel phases, leads and noise: drawn apart from the payloads, so that two calls with equal
    flat = [(mcs, ln) for cap in specs for mcs, ln in cap]             # seeds place frames of equal extent alike
    mp = [_mpdu(rng, ln) for _, ln in flat]
    if joint:
        o0, o1, off = sora.tx_ht40_joint(mp, [mcs for mcs, _ in flat], [int(rng.integers(1, 128)) for _ in flat])
    else:
        o0, o1, off = sora.tx_ht40(mp, mp, [mcs for mcs, _ in flat])
    x = np.stack([o.cpu().numpy().astype(float) for o in (o0, o1)])
    x = x[..., 0] + 1j * x[..., 1]
    parts, descs, truth, pos, k = [], [], [], 0, 0
    for ci, cap in enumerate(specs):
        segs, want = [], []
        for mcs, ln in cap:
            ph = geo.uniform(0, 2 * np.pi, 4)
            H = np.array([[1.0 * np.exp(1j * ph[0]), 0.3 * np.exp(1j * ph[1])], [0.25 * np.exp(1j * ph[2]), 0.9 * np.exp(1j * ph[3])]])
            segs.append(m.channel(x[:, off[k]:off[k + 1]], H, 0.0, rng, scale=GAIN, cfo_step=cfo_step, lead=int(geo.integers(300, 900))))
            want.append((mcs, m.add_fcs(mp[k]))); k += 1
        y = np.concatenate(segs + [np.zeros((2, tail + 27, 2), np.int16)], axis=1).astype(np.float64)
        y += geo.normal(0, 8.0, y.shape)
        y = np.clip(np.rint(y), -32768, 32767).astype(np.int16)
        n = y.shape[1] // 28 * 28
        parts.append(y[:, :n]); descs.append((pos, n, 100 + ci)); truth.append(want); pos += n
    return np.concatenate(parts, axis=1), descs, truth


def _raw_call(env, iq, descs, coding, nsoft=1 << 22, mf=4):
    torch, sora = env
    rx = sora.RxHt40(64, nsoft)
    rx.set_coding(coding)
    t = rx.process_captures_dev(torch.from_numpy(iq[0].copy()).cuda(), torch.from_numpy(iq[1].copy()).cuda(), descs, max_frames_per_capture=mf)
    res = rx.results(ticket=t)
    rx.close()
    return res


@pytest.mark.parametrize("cfo_step", [0.0, 37.0])
def test_loopback_through_the_raw_capture_receiver_and_the_coding_decides(env, cfo_step):
    """two or three frames per capture, MCS mixed: ONE FRAME_OK row per frame with the sent bytes, rate_kbps = MCS; end_sample as the per-stream form reports it for a
    frame of the same extent; a handle in per-stream coding fed the same captures reports no FRAME_OK row with a sent PSDU"""
    torch, sora = env
    rng = np.random.default_rng(717 + int(cfo_step))
    specs = [[(mcs, int(rng.integers(40, 700))), (8 + (mcs + 3) % 7, int(rng.integers(40, 400)))] + ([(8 + (mcs + 5) % 7, 64)] if mcs % 2 else []) for mcs in range(8, 15)]
    iq, descs, truth = _captures(env, rng, specs, cfo_step)
    res = _raw_call(env, iq, descs, sora.HT40_CODING_JOINT)
    per = {}
    for r in res:
        per.setdefault(r["capture_id"], []).append(r)
    for ci, want in enumerate(truth):
        got = per.get(100 + ci, [])
        assert len(got) == len(want), (cfo_step, ci, [(hex(r["error_code"]), r["rate_kbps"], r["stream"]) for r in got])
        for r, (mcs, psdu) in zip(got, want):
            nb, cr = m.MCS2[mcs]
            assert (r["error_code"], r["rate_kbps"], r["stream"], r["length"], r["mpdu"]) == (FRAME_OK, mcs, 0, len(psdu), psdu), (cfo_step, ci, hex(r["error_code"]), r["rate_kbps"])
            assert r["nsym"] == J.nsym_for(len(psdu), nb, cr) and not r["flags"]
    # the handle's coding decides: the same captures on a per-stream handle
    other = _raw_call(env, iq, descs, sora.HT40_CODING_PER_STREAM)
    sent = {psdu for want in truth for _, psdu in want}
    assert not [r for r in other if r["error_code"] == FRAME_OK and r["mpdu"] in sent]
    # end_sample: a per-stream frame of the same extent (same MCS, the per-stream length whose symbol count is the joint frame's) at the same place in a capture
    # of the same length is reported at the same source position
    mcs, ln = 12, 300
    nb, cr = m.MCS2[mcs]
    nsym = J.nsym_for(ln + 4, nb, cr)
    ln_ps = (nsym * m.ndbps(nb, cr) - 22) // 8 - 4
    assert m.nsym_for([ln_ps + 4], nb, cr) == nsym
    a_iq, a_d, _ = _captures(env, np.random.default_rng(9), [[(mcs, ln)]], cfo_step, joint=True)
    b_iq, b_d, _ = _captures(env, np.random.default_rng(9), [[(mcs, ln_ps)]], cfo_step, joint=False)
    ra = _raw_call(env, a_iq, a_d, sora.HT40_CODING_JOINT); rb = _raw_call(env, b_iq, b_d, sora.HT40_CODING_PER_STREAM)
    assert a_d == b_d and len(ra) == 1 and len(rb) == 2 and ra[0]["error_code"] == rb[0]["error_code"] == rb[1]["error_code"] == FRAME_OK
    assert ra[0]["end_sample"] == rb[0]["end_sample"] == rb[1]["end_sample"] and ra[0]["nsym"] == rb[0]["nsym"] == nsym


def test_stream_mode_cut_at_random_source_calls_yields_the_uncut_rows(env):
    """one stream of six joint frames, cut at random 28-sample source calls (the pattern of tests/test_gpu_stream_ht40.py): exactly the rows of the uncut mode-off
    call in joint coding, every frame once"""
    torch, sora = env
    rng = np.random.default_rng(818)
    spec = [(9, 120), (14, 700), (8, 33), (12, 410), (13, 900), (11, 64)]
    iq, descs, truth = _captures(env, rng, [spec], 21.0, tail=28 * 32)
    n = iq.shape[1]
    key = lambda r: tuple(r[f] for f in ("error_code", "rate_kbps", "stream", "length", "crc32", "end_sample", "mpdu"))
    want = _raw_call(env, iq, [(0, n, 0)], sora.HT40_CODING_JOINT, mf=8)
    assert [(r["error_code"], r["rate_kbps"], r["mpdu"]) for r in want] == [(FRAME_OK, mcs, psdu) for mcs, psdu in truth[0]]
    rx = sora.RxHt40(64, 1 << 22)
    rx.set_coding(sora.HT40_CODING_JOINT)
    assert rx.set_stream_mode(1) == 0 and rx.set_coding() == sora.HT40_CODING_JOINT
    cuts = sorted(int(c) * 28 for c in rng.choice(np.arange(1, n // 28), size=11, replace=False)) + [n]
    base, got = 0, []
    for arrived in cuts:
        piece = iq[:, base:arrived]
        t = rx.process_captures_dev(torch.from_numpy(piece[0].copy()).cuda(), torch.from_numpy(piece[1].copy()).cuda(), [(0, arrived - base, 0)], max_frames_per_capture=8)
        rows = rx.results(ticket=t)
        used = int(rx.stream_consumed(t, 1)[0])
        assert used % 28 == 0 and used <= arrived - base
        for r in rows:
            assert r["end_sample"] <= used and not r["flags"]
            got.append(dict(r, end_sample=r["end_sample"] + base))
        base += used
    rx.close()
    assert [key(r) for r in got] == [key(r) for r in want]
    assert base >= want[-1]["end_sample"]
