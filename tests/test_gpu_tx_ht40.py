"""GPU 40 MHz HT 2x2 transmitter (sora_hip_tx_ht40, k_tx_ht40.hip).  PARITY UNPINNED for the 40 MHz extension; the waveform is held to
the integer model tests/tx_ht40_model.py (itself held to oracle/py_ht40.py::tx_frame by tests/test_tx_ht40_cpu.py): sample for sample on
both chains for every MCS at lengths on both sides of a symbol step, the shortest and the longest frame, any sample offset and seed;
nothing written outside accepted frames; frames of a batch independent; and what it sends comes back through the 40 MHz receiver
(sora_ht40_*), from raw captures with a channel, noise and a carrier offset, and through the descriptor call."""
import numpy as np
import pytest

from oracle import py_ht40 as m
import tx_ht40_model as T

pytestmark = pytest.mark.gpu

GAIN = 250.0 * 128.0 / T.A                                              # the level at which the receiver's own tests are known to decode
SENTINEL = 0x5A5A


@pytest.fixture(scope="module")
def env():
    import torch
    import sora_amd
    if sora_amd.device_count() <= 0:
        pytest.skip("no HIP device")
    return torch, sora_amd


def _mpdus(rng, ln):
    return [rng.integers(0, 256, ln, dtype=np.uint8).tobytes() for _ in range(2)]


def _step(mcs, n):
    """the longest MPDU (without FCS) of n data symbols; one byte more takes n + 1"""
    return (n * m.ndbps(*m.MCS2[mcs]) - 22) // 8 - 4


@pytest.fixture(scope="module")
def batch(env, oracle):
    """one batch for the exactness tests: (frames, model waveforms), the model computed once"""
    rng = np.random.default_rng(4040)
    frames = []                                                         # (mcs, len, (seed0, seed1))
    for mcs in range(8, 15):
        n = 2 + mcs % 3
        for ln in (_step(mcs, n), _step(mcs, n) + 1):
            frames.append((mcs, ln, (int(rng.integers(1, 128)), int(rng.integers(1, 128)))))
    for k, ln in enumerate((1, 2, 37, 333)):
        frames.append((8 + (3 * k) % 7, ln, (int(rng.integers(1, 128)), int(rng.integers(0, 128)))))
    frames.append((13, 1, (0xDD, 0xAB)))                               # bit 7 set: only seven bits count
    frames.append((14, 3996, (0x11, 0x7F)))
    frames.append((8, 3996, (0x5D, 0x2B)))                             # 593 data symbols, the longest frame there is
    frames.append((11, 700, (0, 0x40)))                                # an all-zero seed: the scrambler stays silent
    for mcs, ln in ((9, 2561), (12, 2563)):                            # the first four bytes, which the CRC complements, straddle the FCS's two waves
        frames.append((mcs, ln, (int(rng.integers(1, 128)), int(rng.integers(1, 128)))))
    mp = [_mpdus(rng, ln) for _, ln, _ in frames]
    want = [T.frame_int_nofcs(a, b, mcs, seeds, oracle=oracle) for (mcs, _, seeds), (a, b) in zip(frames, mp)]
    return frames, mp, want


def _run(env, frames, mp, gaps, seeds="given", fill=0):
    """-> (out0, out1 as int16 numpy [total, 2], offsets of the frames' first samples) through the C entry point on sentinel-filled outputs"""
    torch, sora = env
    from sora_amd.capi import _dev_ptr
    n = len(frames)
    lens = [ln for _, ln, _ in frames]
    off = np.zeros(2 * n + 1, np.int64); np.cumsum([(ln + 3) // 4 * 4 for ln in lens for _ in range(2)], out=off[1:])
    blob = np.zeros(max(int(off[-1]), 4), np.uint8)
    for f in range(n):
        for s in range(2):
            blob[off[2 * f + s]:off[2 * f + s] + lens[f]] = np.frombuffer(mp[f][s][:lens[f]], np.uint8)
    ns = [sora.tx_ht40_samples(ln, mcs) or 1440 for mcs, ln, _ in frames]   # a refused frame keeps a range of its own, to be found untouched
    first = np.zeros(n, np.int64); pos = 0
    for f in range(n):
        first[f] = pos + gaps[f]; pos = first[f] + ns[f]
    total = pos + 8
    dev = torch.device("cuda")
    d = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)
    o0 = torch.full((total, 2), fill, dtype=torch.int16, device=dev); o1 = torch.full((total, 2), fill, dtype=torch.int16, device=dev)
    d_seed = d([v for _, _, sd in frames for v in sd], np.uint8) if seeds == "given" else None
    args = (d(blob, np.uint8), d(off[:-1], np.int32), d(lens, np.int32), d([mcs for mcs, _, _ in frames], np.int32), d(first, np.int64))
    rc = sora.load().sora_hip_tx_ht40(_dev_ptr(args[0]), _dev_ptr(args[1]), _dev_ptr(args[2]), _dev_ptr(args[3]), _dev_ptr(d_seed) if d_seed is not None else None,
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
    for f, (mcs, ln, seeds) in enumerate(frames):
        assert ns[f] == want[f].shape[1], (f, mcs, ln)
        for ch, o in enumerate((o0, o1)):
            got = o[first[f]:first[f] + ns[f]]
            assert _first_difference(got, want[f][ch]) is None, (f, mcs, ln, seeds, ch, int(first[f]) % 4, _first_difference(got, want[f][ch]))
    # ... and nothing outside the frames
    keep = np.ones(len(o0), bool)
    for f in range(len(frames)):
        keep[first[f]:first[f] + ns[f]] = False
    assert keep.sum() >= len(frames) and (o0[keep] == SENTINEL).all() and (o1[keep] == SENTINEL).all()


def test_default_seeds_are_0x5d_and_0x2b(env, oracle):
    rng = np.random.default_rng(11)
    frames = [(12, 90, (0x5D, 0x2B)), (9, 41, (0x5D, 0x2B))]
    mp = [_mpdus(rng, ln) for _, ln, _ in frames]
    a0, a1, first, ns = _run(env, frames, mp, [0, 2], seeds=None)
    b0, b1, _, _ = _run(env, frames, mp, [0, 2], seeds="given")
    assert np.array_equal(a0, b0) and np.array_equal(a1, b1)
    w = T.frame_int_nofcs(mp[0][0], mp[0][1], 12, oracle=oracle)
    assert np.array_equal(a0[:ns[0]], w[0]) and np.array_equal(a1[:ns[0]], w[1])


def test_frames_that_are_not_accepted_leave_their_range_untouched(env, oracle):
    rng = np.random.default_rng(12)
    frames = [(10, 60, (3, 5)), (7, 60, (3, 5)), (9, 25, (9, 8)), (15, 60, (3, 5)), (11, 0, (1, 2)), (14, 100, (7, 7)), (12, 3997, (1, 2)), (8, 9, (4, 6))]
    mp = [_mpdus(rng, max(ln, 4)) for _, ln, _ in frames]
    o0, o1, first, ns = _run(env, frames, mp, [3, 0, 1, 6, 0, 2, 0, 5], fill=SENTINEL)
    good = np.zeros(len(o0), bool)
    for f, (mcs, ln, seeds) in enumerate(frames):
        if mcs in m.MCS2 and 1 <= ln <= 3996:
            w = T.frame_int_nofcs(mp[f][0][:ln], mp[f][1][:ln], mcs, seeds, oracle=oracle)
            assert np.array_equal(o0[first[f]:first[f] + ns[f]], w[0]) and np.array_equal(o1[first[f]:first[f] + ns[f]], w[1]), (f, mcs, ln)
            good[first[f]:first[f] + ns[f]] = True
    assert good.sum() == sum(ns[f] for f in (0, 2, 5, 7))
    assert (o0[~good] == SENTINEL).all() and (o1[~good] == SENTINEL).all()


def test_frames_of_a_batch_are_independent(env):
    """the same frame first, in the middle and last of a batch of different frames: identical samples"""
    torch, sora = env
    rng = np.random.default_rng(13)
    a, b = _mpdus(rng, 611)
    others = [(8 + k % 7, int(rng.integers(1, 900))) for k in range(30)]
    m0 = [a] + [rng.integers(0, 256, ln, dtype=np.uint8).tobytes() for _, ln in others[:15]] + [a]
    m0 += [rng.integers(0, 256, ln, dtype=np.uint8).tobytes() for _, ln in others[15:]] + [a]
    m1 = [b if x is a else rng.integers(0, 256, len(x), dtype=np.uint8).tobytes() for x in m0]
    mcs = [13] + [v for v, _ in others[:15]] + [13] + [v for v, _ in others[15:]] + [13]
    seeds = [(0x31, 0x62)] + [(1 + k, 99 - k) for k in range(15)] + [(0x31, 0x62)] + [(40 + k, 3 + k) for k in range(15)] + [(0x31, 0x62)]
    o0, o1, off = sora.tx_ht40(m0, m1, mcs, seeds)
    o0, o1 = o0.cpu().numpy(), o1.cpu().numpy()
    n = sora.tx_ht40_samples(611, 13)
    cut = lambda o, f: o[off[f]:off[f] + n]
    assert off[1] - off[0] == n and np.abs(cut(o0, 0).astype(int)).max() > 1000
    for f in (16, 32):
        assert np.array_equal(cut(o0, 0), cut(o0, f)) and np.array_equal(cut(o1, 0), cut(o1, f)), f


def _loopback_captures(env, rng, specs, cfo_step):
    """specs: per capture a list of (mcs, len).  One tx_ht40 batch, mixed on the GPU: per frame H with random phases x GAIN, a carrier
    offset applied as py_ht40.channel applies it, a lead of 300..900 zero samples; per capture 800 trailing zeros, noise of sigma 8,
    rounded to int16, whole 28-sample bursts.  -> (iq0, iq1 CUDA int16 [n, 2], descs, truth)"""
    torch, sora = env
    flat = [(mcs, ln) for cap in specs for mcs, ln in cap]
    mp = [_mpdus(rng, ln) for _, ln in flat]
    o0, o1, off = sora.tx_ht40([a for a, _ in mp], [b for _, b in mp], [mcs for mcs, _ in flat], [(int(rng.integers(1, 128)), int(rng.integers(1, 128))) for _ in flat])
    x = torch.stack([torch.complex(o[:, 0].double(), o[:, 1].double()) for o in (o0, o1)])
    gen = torch.Generator(device="cuda"); gen.manual_seed(int(rng.integers(1 << 30)))
    parts, descs, truth, pos, k = [], [], [], 0, 0
    for ci, cap in enumerate(specs):
        segs = []; want = []
        for mcs, ln in cap:
            ph = rng.uniform(0, 2 * np.pi, 4)
            H = np.array([[1.0 * np.exp(1j * ph[0]), 0.3 * np.exp(1j * ph[1])], [0.25 * np.exp(1j * ph[2]), 0.9 * np.exp(1j * ph[3])]]) * GAIN
            xf = x[:, off[k]:off[k + 1]]
            y = torch.stack([complex(H[r, 0]) * xf[0] + complex(H[r, 1]) * xf[1] for r in range(2)])
            if cfo_step:
                y = y * torch.exp(1j * 2 * np.pi * cfo_step / 65536.0 * torch.arange(y.shape[1], device="cuda", dtype=torch.float64))[None]
            segs += [torch.zeros((2, int(rng.integers(300, 900))), dtype=torch.complex128, device="cuda"), y]
            want.append((mcs, [m.add_fcs(mp[k][0]), m.add_fcs(mp[k][1])])); k += 1
        y = torch.cat(segs + [torch.zeros((2, 800), dtype=torch.complex128, device="cuda")], dim=1)
        y = torch.view_as_real(y) + 8.0 * torch.randn(y.shape + (2,), generator=gen, device="cuda", dtype=torch.float64)
        y = torch.clamp(torch.round(y), -32768, 32767).to(torch.int16)
        n = y.shape[1] // 28 * 28
        parts.append(y[:, :n]); descs.append((pos, n, 100 + ci)); truth.append(want); pos += n
    iq = torch.cat(parts, dim=1)
    return iq[0].contiguous(), iq[1].contiguous(), descs, truth


@pytest.mark.parametrize("cfo_step", [0.0, 21.0])
def test_loopback_through_the_raw_capture_receiver(env, cfo_step):
    torch, sora = env
    rng = np.random.default_rng(515 + int(cfo_step))
    specs = [[(mcs, int(rng.integers(40, 700))), (8 + (mcs + 3) % 7, int(rng.integers(40, 400)))] + ([(8 + (mcs + 5) % 7, 64)] if mcs % 2 else []) for mcs in range(8, 15)]
    iq0, iq1, descs, truth = _loopback_captures(env, rng, specs, cfo_step)
    nsoft = 2 * sum(2 * (m.nsym_for([ln + 4], *m.MCS2[mcs]) * 108 * m.MCS2[mcs][0] + 64) for cap in specs for mcs, ln in cap)
    rx = sora.RxHt40(64, nsoft)
    t = rx.process_captures_dev(iq0, iq1, descs, max_frames_per_capture=4)
    res = rx.results(ticket=t)
    rx.close()
    per = {}
    for r in res:
        per.setdefault(r["capture_id"], []).append(r)
    for ci, want in enumerate(truth):
        got = per.get(100 + ci, [])
        exp = [(mcs, s, ps[s]) for mcs, ps in want for s in range(2)]
        assert len(got) == len(exp), (cfo_step, ci, [(hex(r["error_code"]), r["rate_kbps"], r["stream"]) for r in got])
        for r, e in zip(got, exp):
            assert (r["error_code"], r["rate_kbps"], r["stream"], r["mpdu"]) == (1, e[0], e[1], e[2]), (cfo_step, ci, hex(r["error_code"]), r["rate_kbps"], r["stream"])


def test_loopback_through_the_descriptor_call(env):
    """sora_ht40_process_dev on the transmitter's two chains as they are (identity channel x GAIN, no noise), HT-LTF 1 at 1280 samples into each frame"""
    torch, sora = env
    rng = np.random.default_rng(616)
    flat = [(mcs, ln) for mcs in range(8, 15) for ln in (int(rng.integers(1, 60)), int(rng.integers(100, 1200)))]
    mp = [_mpdus(rng, ln) for _, ln in flat]
    o0, o1, off = sora.tx_ht40([a for a, _ in mp], [b for _, b in mp], [mcs for mcs, _ in flat], gaps=[64] * len(flat))
    scale = lambda o: torch.clamp(torch.round(torch.cat([o, torch.zeros_like(o[:256])]).double() * GAIN), -32768, 32767).to(torch.int16)
    descs = []
    for f, (mcs, ln) in enumerate(flat):
        nb, cr = m.MCS2[mcs]
        descs.append((off[f] + 64 + 1280, nb, cr, ln + 4, ln + 4, 0, 0.0, f))
    nsoft = sum(2 * (sora.ht40_symbols(d[3], d[4], d[1], d[2]) * 108 * d[1] + 64) for d in descs)
    rx = sora.RxHt40(len(descs), nsoft)
    rx.process_dev(scale(o0), scale(o1), descs, None)
    res = rx.results(); rx.close()
    assert len(res) == 2 * len(flat)
    for r in res:
        f, s = r["capture_id"], r["stream"]
        assert r["error_code"] == 1 and r["mpdu"] == m.add_fcs(mp[f][s]), (flat[f], s, hex(r["error_code"]))
