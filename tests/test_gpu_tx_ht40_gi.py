"""GPU 40 MHz HT 2x2 transmitter with a guard-interval kind per frame (sora_hip_tx_ht40_gi, sora_hip_tx_ht40_joint_gi; k_tx_ht40_gi, k_tx_ht40_joint_gi; DESIGN.md
section 7 g4), held sample for sample on both chains to tests/tx_ht40_gi_model.py (itself held to the existing models by tests/test_ht40_gi_models_cpu.py): both codings,
every MCS at the two lengths either side of a symbol step, N_SYM = 1, 9, 10, 11 (where ceil(9 n / 10) moves against n), the longest frame, first samples at every residue
mod 4 (the 16-byte and the word-by-word emission), kinds 0 and 1 mixed in one call; kind 0 and a null kind array byte-equal to the entry points without a kind; a kind of 2
writes nothing and disturbs nobody."""
import numpy as np
import pytest

from oracle import py_ht40 as m
import tx_ht40_gi_model as TG

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A


@pytest.fixture(scope="module")
def env():
    import torch
    import sora_amd
    if sora_amd.device_count() <= 0:
        pytest.skip("no HIP device")
    return torch, sora_amd


def _step(mcs, n, joint):
    """the longest MPDU (without FCS) of n data symbols in the coding; one byte more takes n + 1"""
    return (n * m.ndbps(*m.MCS2[mcs]) * (2 if joint else 1) - 22) // 8 - 4


def _frames(joint):
    """(mcs, len, seeds, kind): every MCS either side of a symbol step in both kinds, N_SYM 1 / 9 / 10 / 11, the longest frame"""
    rng = np.random.default_rng(1440 + joint)
    seed = (lambda: int(rng.integers(1, 128))) if joint else (lambda: (int(rng.integers(1, 128)), int(rng.integers(1, 128))))
    out = []
    for mcs in range(8, 15):
        n = 2 + mcs % 3
        for k, ln in enumerate((_step(mcs, n, joint), _step(mcs, n, joint) + 1)):
            out.append((mcs, ln, seed(), 1))
            if (mcs + k) % 2:
                out.append((mcs, ln, seed(), 0))                          # long frames between the short ones
    for k, n in enumerate((1, 9, 10, 11)):
        mcs = (9, 11, 12, 14)[k]
        lo = _step(mcs, n - 1, joint) + 1 if n > 1 else 1
        ln = max(1, min(_step(mcs, n, joint), lo + 3))
        out.append((mcs, ln, seed(), 1))
    out.append((8, 3996, seed(), 1))                                      # the longest frame: 593 data symbols per stream (joint: 297)
    return out


def _nsym(mcs, ln, joint):
    nd = m.ndbps(*m.MCS2[mcs]) * (2 if joint else 1)
    return -(-(16 + 8 * (ln + 4) + 6) // nd)


@pytest.fixture(scope="module", params=[False, True], ids=["per_stream", "joint"])
def batch(request, oracle):
    joint = request.param
    frames = _frames(joint)
    rng = np.random.default_rng(77 + joint)
    mp = [[rng.integers(0, 256, ln, dtype=np.uint8).tobytes() for _ in range(1 if joint else 2)] for _, ln, _, _ in frames]
    want = [TG.frame_int_nofcs(p[0] if joint else p, mcs, gi, sd, joint=joint, oracle=oracle) for (mcs, _, sd, gi), p in zip(frames, mp)]
    return joint, frames, mp, want


def _run(env, joint, frames, mp, gaps, kinds="given", fill=SENTINEL, entry="gi"):
    """-> (out0, out1 int16 numpy [total, 2], first samples, sample counts) through the C entry point on sentinel-filled outputs.  kinds: "given" (the frames' own),
    None (a null d_gi); entry "plain": the entry point without a kind"""
    torch, sora = env
    from sora_amd.capi import _dev_ptr
    L = sora.load()
    n = len(frames); per = 1 if joint else 2
    lens = [ln for _, ln, _, _ in frames]
    off = np.zeros(per * n + 1, np.int64); np.cumsum([(ln + 3) // 4 * 4 for ln in lens for _ in range(per)], out=off[1:])
    blob = np.zeros(max(int(off[-1]), 4), np.uint8)
    for f in range(n):
        for s in range(per):
            blob[off[per * f + s]:off[per * f + s] + lens[f]] = np.frombuffer(mp[f][s][:lens[f]], np.uint8)
    samples = sora.tx_ht40_joint_gi_samples if joint else sora.tx_ht40_gi_samples
    ns = [samples(ln, mcs, gi if kinds == "given" else 0) or 1440 for mcs, ln, _, gi in frames]   # a refused frame keeps a range of its own, to be found untouched
    first = np.zeros(n, np.int64); pos = 0
    for f in range(n):
        first[f] = pos + gaps[f]; pos = first[f] + ns[f]
    total = pos + 8
    dev = torch.device("cuda")
    d = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)
    o0 = torch.full((total, 2), fill, dtype=torch.int16, device=dev); o1 = torch.full((total, 2), fill, dtype=torch.int16, device=dev)
    seeds = [sd for _, _, sd, _ in frames] if joint else [v for _, _, sd, _ in frames for v in sd]
    a = (d(blob, np.uint8), d(off[:-1], np.int32), d(lens, np.int32), d([mcs for mcs, _, _, _ in frames], np.int32), d(seeds, np.uint8), d(first, np.int64))
    d_gi = d([gi for _, _, _, gi in frames], np.uint8) if kinds == "given" else None
    if entry == "plain":
        fn = L.sora_hip_tx_ht40_joint if joint else L.sora_hip_tx_ht40
        rc = fn(_dev_ptr(a[0]), _dev_ptr(a[1]), _dev_ptr(a[2]), _dev_ptr(a[3]), _dev_ptr(a[4]), n, _dev_ptr(o0), _dev_ptr(o1), _dev_ptr(a[5]), None)
    else:
        fn = L.sora_hip_tx_ht40_joint_gi if joint else L.sora_hip_tx_ht40_gi
        rc = fn(_dev_ptr(a[0]), _dev_ptr(a[1]), _dev_ptr(a[2]), _dev_ptr(a[3]), _dev_ptr(a[4]), _dev_ptr(d_gi) if d_gi is not None else None, n, _dev_ptr(o0), _dev_ptr(o1),
                _dev_ptr(a[5]), None)
    assert rc == 0, L.sora_hip_last_error()
    torch.cuda.synchronize()
    return o0.cpu().numpy(), o1.cpu().numpy(), first, ns


def _first_difference(got, want):
    bad = np.nonzero((got != want).any(axis=1))[0]
    return None if len(bad) == 0 else (int(bad[0]), len(bad), got[bad[0]].tolist(), want[bad[0]].tolist())


def test_sample_exact_against_the_integer_model(env, batch):
    joint, frames, mp, want = batch
    assert {_nsym(mcs, ln, joint) for mcs, ln, _, gi in frames if gi} >= {1, 9, 10, 11} and {gi for _, _, _, gi in frames} == {0, 1}
    gaps = [(5 * f + 1) % 11 for f in range(len(frames))]
    o0, o1, first, ns = _run(env, joint, frames, mp, gaps)
    # first samples at every residue mod 4, for short frames too: a short frame that starts 16-byte aligned stays aligned for all its symbols (576 bytes each)
    assert {int(first[f]) % 4 for f, fr in enumerate(frames) if fr[3]} == {0, 1, 2, 3}
    for f, (mcs, ln, sd, gi) in enumerate(frames):
        assert ns[f] == want[f].shape[1] == 1600 + (144 if gi else 160) * _nsym(mcs, ln, joint), (f, mcs, ln, gi)
        for ch, o in enumerate((o0, o1)):
            got = o[first[f]:first[f] + ns[f]]
            assert _first_difference(got, want[f][ch]) is None, (joint, f, mcs, ln, sd, gi, ch, int(first[f]) % 4, _first_difference(got, want[f][ch]))
    keep = np.ones(len(o0), bool)                                          # ... and nothing outside the frames
    for f in range(len(frames)):
        keep[first[f]:first[f] + ns[f]] = False
    assert keep.sum() >= len(frames) and (o0[keep] == SENTINEL).all() and (o1[keep] == SENTINEL).all()


def test_kind_0_and_a_null_kind_array_are_the_entry_point_without_a_kind(env, batch):
    joint, frames, mp, _ = batch
    sel = [i for i, fr in enumerate(frames) if fr[1] < 3000][:12]
    fr0 = [frames[i][:3] + (0,) for i in sel]; mp0 = [mp[i] for i in sel]
    gaps = [(3 * f + 2) % 7 for f in range(len(fr0))]
    ref = _run(env, joint, fr0, mp0, gaps, entry="plain")
    zero = _run(env, joint, fr0, mp0, gaps, kinds="given")
    null = _run(env, joint, fr0, mp0, gaps, kinds=None)
    for got in (zero, null):
        assert np.array_equal(got[2], ref[2]) and got[3] == ref[3]
        assert got[0].tobytes() == ref[0].tobytes() and got[1].tobytes() == ref[1].tobytes()


def test_a_kind_of_2_leaves_its_range_untouched_and_its_neighbours_alone(env, batch, oracle):
    joint, frames, mp, want = batch
    torch, sora = env
    samples = sora.tx_ht40_joint_gi_samples if joint else sora.tx_ht40_gi_samples
    assert samples(100, 9, 2) == 0 and samples(100, 9, 255) == 0 and samples(100, 9, 1) > 0 and samples(100, 7, 1) == 0 and samples(3997, 9, 1) == 0
    pick = [i for i, fr in enumerate(frames) if fr[1] < 3000][:5]
    fr = [frames[i] for i in pick]; mq = [mp[i] for i in pick]; wq = [want[i] for i in pick]
    fr[1] = fr[1][:3] + (2,); fr[3] = fr[3][:3] + (255,)
    o0, o1, first, ns = _run(env, joint, fr, mq, [1, 0, 3, 2, 0])
    good = np.zeros(len(o0), bool)
    for f in (0, 2, 4):
        assert np.array_equal(o0[first[f]:first[f] + ns[f]], wq[f][0]) and np.array_equal(o1[first[f]:first[f] + ns[f]], wq[f][1]), f
        good[first[f]:first[f] + ns[f]] = True
    assert ns[1] == ns[3] == 1440 and (o0[~good] == SENTINEL).all() and (o1[~good] == SENTINEL).all()


def test_python_wrappers_mix_kinds(env, batch, oracle):
    joint, frames, mp, want = batch
    torch, sora = env
    pick = [i for i, fr in enumerate(frames) if fr[1] < 3000][:6]
    mcs = [frames[i][0] for i in pick]; gi = [frames[i][3] for i in pick]; seeds = [frames[i][2] for i in pick]
    if joint:
        o0, o1, off = sora.tx_ht40_joint([mp[i][0] for i in pick], mcs, seeds, gi=gi)
    else:
        o0, o1, off = sora.tx_ht40([mp[i][0] for i in pick], [mp[i][1] for i in pick], mcs, seeds, gi=gi)
    o0, o1 = o0.cpu().numpy(), o1.cpu().numpy()
    for k, i in enumerate(pick):
        assert off[k + 1] - off[k] == want[i].shape[1]
        assert np.array_equal(o0[off[k]:off[k + 1]], want[i][0]) and np.array_equal(o1[off[k]:off[k + 1]], want[i][1]), (k, frames[i])
    with pytest.raises(sora.SoraError):
        (sora.tx_ht40_joint([b"ab"], [9], gi=[2]) if joint else sora.tx_ht40([b"ab"], [b"cd"], [9], gi=[2]))
