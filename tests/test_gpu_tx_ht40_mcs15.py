"""The 40 MHz HT 2x2 transmitter behind a gate (sora_hip_tx_ht40_mcs, sora_hip_tx_ht40_joint_mcs; k_tx_ht40_mcs, k_tx_ht40_joint_mcs): with the
gate at 15, MCS 15 frames (64-QAM, rate 5/6: A1 B1 A2 B3 A4 B5, HT-SIG MCS 15) held sample for sample on both chains to tests/ht40_mcs15_model.py's statement of
tests/tx_ht40_gi_model.py -- N_SYM 1 and 2, both sides of a symbol step, 3996 bytes, both codings, both guard intervals, mixed with MCS 8..14 in one call, first samples at
every residue mod 4; with the gate at 14, byte-equal to the _gi entry points, including that MCS 15 then writes nothing; a gate of 13 or 16 is refused.  Then the loop:
tx_ht40(..., mcs_max=15) through a channel chosen so that the models alone decode every frame, into a handle whose gate is 15 -- FRAME_OK and the sent bytes."""
import numpy as np
import pytest

from oracle import ht40_data_model as dm
from oracle import py_ht40 as m
import ht40_mcs15_model as M
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


def _nd(mcs, joint):
    with M.rate56():
        return m.ndbps(*m.MCS2[mcs]) * (2 if joint else 1)


def _step(mcs, n, joint):
    """the longest MPDU (without FCS) of n data symbols in the coding; one byte more takes n + 1"""
    return (n * _nd(mcs, joint) - 22) // 8 - 4


def _nsym(mcs, ln, joint):
    return -(-(16 + 8 * (ln + 4) + 6) // _nd(mcs, joint))


def _frames(joint):
    """(mcs, len, seeds, kind): MCS 15 at one byte, at both sides of the steps 1 -> 2 and 2 -> 3 symbols in both kinds, at 3996 bytes, with MCS 8..14 between them"""
    rng = np.random.default_rng(1550 + joint)
    seed = (lambda: int(rng.integers(1, 128))) if joint else (lambda: (int(rng.integers(1, 128)), int(rng.integers(1, 128))))
    out = [(15, 1, seed(), 0)]
    for k, n in enumerate((1, 2)):
        for j, ln in enumerate((_step(15, n, joint), _step(15, n, joint) + 1)):
            out.append((15, ln, seed(), (k + j) & 1))
            out.append((15, ln, seed(), (k + j + 1) & 1))
            out.append((8 + (3 * k + 2 * j + joint) % 7, 30 + 7 * k + j, seed(), j))
    out.append((15, 3996, seed(), 1))
    out.append((14, 200, seed(), 0))
    out.append((15, 3996, seed(), 0))
    return out


@pytest.fixture(scope="module", params=[False, True], ids=["per_stream", "joint"])
def batch(request, oracle):
    joint = request.param
    frames = _frames(joint)
    rng = np.random.default_rng(78 + joint)
    mp = [[rng.integers(0, 256, ln, dtype=np.uint8).tobytes() for _ in range(1 if joint else 2)] for _, ln, _, _ in frames]
    with M.rate56():
        want = [TG.frame_int_nofcs(p[0] if joint else p, mcs, gi, sd, joint=joint, oracle=oracle) for (mcs, _, sd, gi), p in zip(frames, mp)]
    return joint, frames, mp, want


def _run(env, joint, frames, mp, gaps, gate, entry="mcs", expect=0):
    """-> (out0, out1 int16 numpy [total, 2], first samples, sample counts at this gate) through the C entry point on sentinel-filled outputs; entry "gi": the _gi entry point"""
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
    samples = L.sora_hip_tx_ht40_joint_mcs_samples if joint else L.sora_hip_tx_ht40_mcs_samples
    room = [int(samples(ln, mcs, gi, 15)) for mcs, ln, _, gi in frames]            # every frame keeps the range it has at gate 15: a refused one is found untouched
    ns = [int(samples(ln, mcs, gi, gate)) for mcs, ln, _, gi in frames]
    first = np.zeros(n, np.int64); pos = 0
    for f in range(n):
        first[f] = pos + gaps[f]; pos = first[f] + room[f]
    total = pos + 8
    dev = torch.device("cuda")
    d = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)
    o0 = torch.full((total, 2), SENTINEL, dtype=torch.int16, device=dev); o1 = torch.full((total, 2), SENTINEL, dtype=torch.int16, device=dev)
    seeds = [sd for _, _, sd, _ in frames] if joint else [v for _, _, sd, _ in frames for v in sd]
    a = (d(blob, np.uint8), d(off[:-1], np.int32), d(lens, np.int32), d([mcs for mcs, _, _, _ in frames], np.int32), d(seeds, np.uint8), d(first, np.int64))
    d_gi = d([gi for _, _, _, gi in frames], np.uint8)
    if entry == "gi":
        fn = L.sora_hip_tx_ht40_joint_gi if joint else L.sora_hip_tx_ht40_gi
        rc = fn(_dev_ptr(a[0]), _dev_ptr(a[1]), _dev_ptr(a[2]), _dev_ptr(a[3]), _dev_ptr(a[4]), _dev_ptr(d_gi), n, _dev_ptr(o0), _dev_ptr(o1), _dev_ptr(a[5]), None)
    else:
        fn = L.sora_hip_tx_ht40_joint_mcs if joint else L.sora_hip_tx_ht40_mcs
        rc = fn(_dev_ptr(a[0]), _dev_ptr(a[1]), _dev_ptr(a[2]), _dev_ptr(a[3]), _dev_ptr(a[4]), _dev_ptr(d_gi), n, _dev_ptr(o0), _dev_ptr(o1), _dev_ptr(a[5]), int(gate), None)
    assert rc == expect, (rc, L.sora_hip_last_error())
    torch.cuda.synchronize()
    return o0.cpu().numpy(), o1.cpu().numpy(), first, ns


def _first_difference(got, want):
    bad = np.nonzero((got != want).any(axis=1))[0]
    return None if len(bad) == 0 else (int(bad[0]), len(bad), got[bad[0]].tolist(), want[bad[0]].tolist())


def test_sample_exact_against_the_integer_model(env, batch):
    joint, frames, mp, want = batch
    assert {_nsym(mcs, ln, joint) for mcs, ln, _, _ in frames if mcs == 15} >= {1, 2, 3} and {gi for mcs, _, _, gi in frames if mcs == 15} == {0, 1}
    assert {mcs for mcs, _, _, _ in frames} >= {15, 14} and len({mcs for mcs, _, _, _ in frames}) >= 4
    gaps = [(5 * f + 1) % 11 for f in range(len(frames))]
    o0, o1, first, ns = _run(env, joint, frames, mp, gaps, 15)
    assert {int(first[f]) % 4 for f, fr in enumerate(frames) if fr[0] == 15} == {0, 1, 2, 3}
    for f, (mcs, ln, sd, gi) in enumerate(frames):
        assert ns[f] == want[f].shape[1] == 1600 + (144 if gi else 160) * _nsym(mcs, ln, joint), (f, mcs, ln, gi)
        for ch, o in enumerate((o0, o1)):
            got = o[first[f]:first[f] + ns[f]]
            assert _first_difference(got, want[f][ch]) is None, (joint, f, mcs, ln, sd, gi, ch, int(first[f]) % 4, _first_difference(got, want[f][ch]))
    keep = np.ones(len(o0), bool)                                          # ... and nothing outside the frames
    for f in range(len(frames)):
        keep[first[f]:first[f] + ns[f]] = False
    assert np.all(o0[keep].view(np.uint16) == SENTINEL) and np.all(o1[keep].view(np.uint16) == SENTINEL)


def test_the_gate_at_14_is_the_gi_entry_point_and_mcs15_writes_nothing(env, batch):
    joint, frames, mp, want = batch
    gaps = [(3 * f + 2) % 7 for f in range(len(frames))]
    a0, a1, first, ns = _run(env, joint, frames, mp, gaps, 14)
    b0, b1, _, _ = _run(env, joint, frames, mp, gaps, 14, entry="gi")
    assert np.array_equal(a0, b0) and np.array_equal(a1, b1)
    torch, sora = env
    for f, (mcs, ln, sd, gi) in enumerate(frames):
        rng_ = slice(first[f], first[f] + want[f].shape[1])
        if mcs == 15:
            assert ns[f] == 0 and np.all(a0[rng_].view(np.uint16) == SENTINEL) and np.all(a1[rng_].view(np.uint16) == SENTINEL), f
        else:
            assert ns[f] == want[f].shape[1] == (sora.tx_ht40_joint_gi_samples if joint else sora.tx_ht40_gi_samples)(ln, mcs, gi)
            assert _first_difference(a0[rng_], want[f][0]) is None and _first_difference(a1[rng_], want[f][1]) is None, f


@pytest.mark.parametrize("gate", [13, 16, 0, -1])
def test_any_other_gate_is_refused(env, batch, gate):
    joint, frames, mp, want = batch
    o0, o1, _, ns = _run(env, joint, frames[:4], mp[:4], [0, 1, 2, 3], gate, expect=-1)
    assert np.all(o0.view(np.uint16) == SENTINEL) and np.all(o1.view(np.uint16) == SENTINEL) and ns == [0] * 4


def test_python_wrappers(env, batch):
    joint, frames, mp, want = batch
    torch, sora = env
    mcs = [f[0] for f in frames]; gi = [f[3] for f in frames]; sd = [f[2] for f in frames]
    if joint:
        o0, o1, off = sora.tx_ht40_joint([p[0] for p in mp], mcs, sd, gi=gi, mcs_max=15)
    else:
        o0, o1, off = sora.tx_ht40([p[0] for p in mp], [p[1] for p in mp], mcs, sd, gi=gi, mcs_max=15)
    h0, h1 = o0.cpu().numpy(), o1.cpu().numpy()
    for f in range(len(frames)):
        assert off[f + 1] - off[f] == want[f].shape[1] == sora.tx_ht40_samples(frames[f][1], mcs[f], 15, gi[f], joint=joint)
        assert np.array_equal(h0[off[f]:off[f + 1]], want[f][0]) and np.array_equal(h1[off[f]:off[f + 1]], want[f][1]), f
    for kw in ({}, {"mcs_max": 14}, {"mcs_max": 16}, {"gi": [1]}):           # the defaults keep refusing MCS 15, before any launch
        with pytest.raises(sora.SoraError):
            if joint:
                sora.tx_ht40_joint([b"\x01\x02"], [15], **kw)
            else:
                sora.tx_ht40([b"\x01\x02"], [b"\x03\x04"], [15], **kw)
    assert sora.tx_ht40_samples(100, 15) == 0 and sora.tx_ht40_samples(100, 15, 14, 1, joint=joint) == 0 and sora.tx_ht40_samples(100, 15, 16) == 0
    assert sora.tx_ht40_samples(100, 14, 15) == sora.tx_ht40_samples(100, 14) and sora.tx_ht40_samples(3997, 15, 15) == 0 == sora.tx_ht40_samples(0, 15, 15)


# ------------------------------------------------------------------ the loop
H_LOOP = np.array([[0.9 * np.exp(0.4j), 0.2 * np.exp(-1.0j)], [0.15 * np.exp(2.1j), 0.8 * np.exp(-0.3j)]])
GAIN = 250.0 * 128.0 / 16384                                               # the level of tests/test_gpu_tx_ht40.py's loop-back (16384: the transmitter's LTF carrier)


def _mix(frames_iq, leads, rng, sigma):
    """int16 [2, n, 2] frames -> one capture per chain (int16 [N, 2], N a multiple of 28): per frame `lead` zeros, H_LOOP x GAIN; 800 trailing zeros; white noise"""
    parts = []
    for x, lead in zip(frames_iq, leads):
        c = x[:, :, 0].astype(np.float64) + 1j * x[:, :, 1]
        parts += [np.zeros((2, lead), complex), (H_LOOP * GAIN) @ c]
    y = np.concatenate(parts + [np.zeros((2, 800), complex)], axis=1)
    y = np.stack([y.real, y.imag], axis=2) + rng.normal(0, sigma, y.shape + (2,))
    y = np.clip(np.rint(y), -32768, 32767).astype(np.int16)
    n = y.shape[1] // 28 * 28
    return y[0, :n].copy(), y[1, :n].copy()


@pytest.mark.parametrize("joint", [False, True], ids=["per-stream", "joint"])
def test_loopback_into_a_gate_15_handle(env, oracle, joint):
    torch, sora = env
    rng = np.random.default_rng(1590 + joint)
    specs = [(15, 1, 0), (15, _step(15, 1, joint) + 1, 0), (14, 90, 0), (15, 300, 0), (9, 50, 0), (15, 1200, 0)]       # (mcs, len, gi)
    mp = [[rng.integers(0, 256, ln, dtype=np.uint8).tobytes() for _ in range(1 if joint else 2)] for _, ln, _ in specs]
    mcs = [s[0] for s in specs]; gi = [s[2] for s in specs]
    if joint:
        o0, o1, off = sora.tx_ht40_joint([p[0] for p in mp], mcs, gi=gi, mcs_max=15)
    else:
        o0, o1, off = sora.tx_ht40([p[0] for p in mp], [p[1] for p in mp], mcs, gi=gi, mcs_max=15)
    h = np.stack([o0.cpu().numpy(), o1.cpu().numpy()])
    sent = [h[:, off[f]:off[f + 1]] for f in range(len(specs))]
    with M.rate56():                                                       # (the transmitter's frames are the model's: the models below read what the handle reads)
        for f, (q, _, g) in enumerate(specs):
            assert np.array_equal(sent[f], TG.frame_int_nofcs(mp[f][0] if joint else mp[f], q, g, None, joint=joint, oracle=oracle)), f
    leads = [int(rng.integers(640, 900)) // 4 * 4 for _ in specs]                  # (more than the 512 samples carrier sense looks back over)
    c0, c1 = _mix(sent, leads, rng, 8.0)                                   # (the floor of tests/test_gpu_tx_ht40.py's loop-back; at 4 - 6 LSB carrier sense fires on a frame's own first samples)
    # the models alone, first: the front end at gate 15 records every frame, and each decodes FRAME_OK with the sent bytes (zero-forcing weights of the model's own)
    ev = M.front(c0, c1, mcs_max=15, joint=joint)
    assert [(e["error_code"], e["mcs"], e["ht_len"]) for e in ev] == [(0, q, ln + 4) for q, ln, _ in specs], ev
    iq = np.stack([c0, c1])
    for f, e in enumerate(ev):
        d = M.descriptor(0, e, 0.0, joint, f)
        r = M.model(iq, d[0], d[1], d[2], d[3] if joint else (d[3], d[4]), d[5], dm.zf_weights(iq, d[0], d[5]), joint=joint)
        assert all(s.error_code == 1 for s in r.streams) and [s.psdu for s in r.streams] == [m.add_fcs(p) for p in mp[f]], f
    # ... then the handle
    rx = sora.RxHt40(16, 1 << 20)
    rx.set_coding(int(joint)); assert rx.set_mcs_max(15) == 14
    t = rx.process_captures_dev(torch.from_numpy(c0).cuda(), torch.from_numpy(c1).cuda(), [(0, len(c0), 5)], max_frames_per_capture=8)
    res = rx.results(ticket=t)
    found = rx.found(0, ticket=t)
    rx.close()
    assert [{k: r[k] for k in ("a20", "mcs", "ht_len", "nsym", "cfo", "end_sample", "error_code")} for r in found] == \
           [{k: e[k] for k in ("a20", "mcs", "ht_len", "nsym", "cfo", "end_sample", "error_code")} for e in ev]
    jpf = 1 if joint else 2
    exp = [(q, s, m.add_fcs(mp[f][s])) for f, (q, _, _) in enumerate(specs) for s in range(jpf)]
    assert len(res) == len(exp), [(hex(r["error_code"]), r["rate_kbps"]) for r in res]
    for r, e in zip(res, exp):
        assert (r["error_code"], r["rate_kbps"], r["stream"], r["mpdu"]) == (1, e[0], e[1], e[2]), (hex(r["error_code"]), r["rate_kbps"], r["stream"])
