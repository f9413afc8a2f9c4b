"""The survivor ring's position and the window trace-back of the 16-lane trellis layout (dev_vit16.h), through the stage calls.

k_viterbi16 / k_viterbi16_11n and k_viterbi16w / k_viterbi16w_11n (sora_hip_viterbi11a_ws, sora_hip_viterbi11n_ws, as tests/test_gpu_trellis_stage.py
calls them) on frames of 150 .. 161 bytes: at rate 3/4 that is 1222 .. 1310 steps, more than four turns of the 37-block ring (window 256 + 24) and
more than four of the 31-block one (192 + 36), with every (8 L + 22) mod 24 phase of the frame's last trace-back -- the ring position is a byte
offset that wraps by an unsigned minimum, and a whole window's bytes leave the trace-back as dwords built in registers while a frame's last, partial
window, an output that is not dword-aligned (output stride 173) and the window-parallel form's units go through the byte path.  All three code rates; batches of 1, 7, 8, 9 and 17 jobs (a lone row, a
partial wave, exactly one wave, a wave plus one, two waves plus one) and one wave that mixes lengths 150 and 161, so that its lanes finish at
different ring positions.  Soft values come from a seeded generator -- noisy codewords and pure noise -- and one stream is all-equal, so that every
comparison ties.  Every decoded byte of every job (length + 2) must be Oracle.viterbi_frame's / viterbi_frame_ex(.., 192, 36)'s."""
import numpy as np
import pytest

import trellis_streams as ts

pytestmark = pytest.mark.gpu

W = 1                                   # SORA_TRELLIS_WINDOWED
KERNELS = [("11a", 16, "k_viterbi16"), ("11a", W, "k_viterbi16w"), ("11n", 16, "k_viterbi16_11n"), ("11n", W, "k_viterbi16w_11n")]
LENGTHS = tuple(range(150, 162))
BATCHES = (1, 7, 8, 9, 17)
OUT_STRIDES = (176, 173)                # room for a 161-byte frame's 163 bytes: every job's bytes dword-aligned / at every alignment in one wave
_WANT = {}                              # (cr, sched) -> [(jobs, expected bytes)] per batch, computed once


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def sora():
    import sora_amd
    sora_amd.load()
    assert sora_amd.device_count() > 0
    return sora_amd


def stream(rng, L, cr, kind):
    if kind == "equal":
        return np.full(ts.nsoft_for(L, cr), 3, np.uint8)
    n = ts.nsoft_for(L, cr, 48 * (kind % 2))
    if kind % 3 == 2:                                                          # pure noise
        return rng.integers(0, 8, n).astype(np.uint8)
    s = ts.codeword(rng, n, cr).astype(np.int64)                               # a codeword, every value pushed up to three levels towards the other side
    s = np.where(s == 7, 7 - rng.integers(0, 4, n), rng.integers(0, 4, n))
    return s.astype(np.uint8)


def batches(cr):
    """[(name, jobs)]: the five batch sizes with the lengths 150 .. 161 in turn (all twelve occur), the all-equal stream, and the mixed wave"""
    rng = np.random.default_rng(7000 + cr)
    out, k = [], 0
    for n in BATCHES:
        jobs = []
        for _ in range(n):
            L = LENGTHS[k % len(LENGTHS)]
            jobs.append((stream(rng, L, cr, k), L))
            k += 1
        out.append(("batch of %d" % n, jobs))
    out[-1][1][5] = (stream(rng, 157, cr, "equal"), 157)
    out.append(("lengths 150 and 161 in one wave", [(stream(rng, L, cr, i), L) for i, L in enumerate((150, 161) * 4)]))
    return out


def expected(oracle, cr, sched):
    if (cr, sched) not in _WANT:
        win, look = ts.SCHEDULES[sched]
        f = (lambda s, L: oracle.viterbi_frame(s, cr, L)) if sched == "11a" else (lambda s, L: oracle.viterbi_frame_ex(s, cr, L, win, look))
        _WANT[(cr, sched)] = [(name, jobs, [f(s, L) for s, L in jobs]) for name, jobs in batches(cr)]
        assert all(len(w) == L + 2 for _, jobs, want in _WANT[(cr, sched)] for w, (_, L) in zip(want, jobs))
    return _WANT[(cr, sched)]


def run(sora, torch, jobs, cr, sched, lanes, out_stride):
    buf, offs, ns, lens = ts.layout(jobs)
    d = torch.from_numpy(buf).cuda()
    args = (torch.from_numpy(offs.astype(np.int32)).cuda(), torch.from_numpy(ns.astype(np.int32)).cuda(), torch.from_numpy(lens.astype(np.int16)).cuda())
    wsb = (sora.viterbi11a_workspace_bytes if sched == "11a" else sora.viterbi11n_workspace_bytes)(d.numel(), len(jobs))
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    call = sora.viterbi11a_ws if sched == "11a" else sora.viterbi11n_ws
    out = call(d, *args, cr, ws, out_stride=out_stride, lanes_per_pair=lanes)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("cr", (0, 1, 2))
@pytest.mark.parametrize("kernel", KERNELS, ids=[k[2] for k in KERNELS])
def test_ring_turns_and_last_window_phases(sora, torch_cuda, oracle, kernel, cr):
    sched, lanes, name = kernel
    assert {L for _, jobs, _ in expected(oracle, cr, sched) for _, L in jobs} == set(LENGTHS)
    for what, jobs, want in expected(oracle, cr, sched):
        for stride in OUT_STRIDES:
            got = run(sora, torch_cuda, jobs, cr, sched, lanes, stride)
            for i, w in enumerate(want):
                g = got[i, :len(w)]
                if not np.array_equal(g, w):
                    bad = np.nonzero(g != w)[0]
                    pytest.fail("%s, rate %d, %s, output stride %d: job %d (length %d) differs from the oracle at byte %d (%d bytes differ)"
                                % (name, cr, what, stride, i, len(w) - 2, bad[0], len(bad)))
