"""k_viterbi56_11n alone, through its stage entry point (sora_hip_viterbi56_11n, sora_amd.viterbi56_11n), bit for bit against tests/viterbi56_model.py: the K=7
decoder at code rate 5/6 (A1 B1 A2 B3 A4 B5) under the 192 / 36 window schedule.  Every decoded byte of every job is compared, and every byte of a job's output row
behind them must still be zero.  The model's bytes are computed once per module.

Shapes (tr_end = 8 length + 22 steps; the schedule is looked at after every 5-step group, a window is due from step ob + 234 on):
  lengths 1..5        every residue of tr_end mod 5
  26, 27              the largest length with tr_end < 234 and the one above it (one trace-back / a window and then the frame's end one group later)
  51, 98              a window's threshold and the frame's end inside the same group (426..430 and 806..810), with their neighbours 50, 52, 97, 99
  60..100             two to four windows
  4000                many ring wraps and 120-step periods
  pairs               the A side ends first / the B side ends first / equal; an odd job count; a single job
Streams: uniform random; clean codewords; constant 0, 7, 3 / 4 ties and alternating values, and streams of tests/golden/trellis_adversarial.npz cut to whole 6-value
groups; random 0 / 7 values (the largest branch metrics: the 8-bit metrics wrap).  Layouts: unaligned offsets, junk in the bytes' high bits, a stream that ends exactly
at soft_span_bytes, streams that end before their frame does and streams with a ragged tail."""
import os

import numpy as np
import pytest

import viterbi56_model as vm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT_STRIDE = 4112                       # room for a 4000-byte frame's 4002 bytes
LENGTHS = (1, 2, 3, 4, 5, 26, 27, 50, 51, 52, 60, 74, 75, 97, 98, 99, 100)


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


def random_job(rng, L, extra=0):
    return rng.integers(0, 8, vm.nsoft_of(L) + 6 * extra).astype(np.uint8), L


def clean_job(rng, L, extra=0):
    return vm.clean_stream(rng.integers(0, 256, L + 2, dtype=np.uint8).tobytes(), extra_groups=extra), L


def wrap_job(rng, L):
    return (rng.integers(0, 2, vm.nsoft_of(L) + 12) * 7).astype(np.uint8), L


def constant_jobs(L):
    n = vm.nsoft_of(L)
    alt = np.zeros(n, np.uint8); alt[1::2] = 7
    ties = np.full(n, 3, np.uint8); ties[1::2] = 4
    return [(np.full(n, 0, np.uint8), L), (np.full(n, 7, np.uint8), L), (alt, L), (ties, L), (np.full(n, 3, np.uint8), L), (np.full(n, 4, np.uint8), L)]


def golden_jobs(limit=1400):
    """streams of the recorded adversarial set (ties, wrap, bursts, lengths: rate 3/4's), each cut to whole 6-value groups and given the longest frame it holds"""
    z = np.load(os.path.join(ROOT, "tests", "golden", "trellis_adversarial.npz"))
    soft, nsoft = z["soft_2"], z["nsoft_2"]
    offs = np.concatenate([[0], np.cumsum(nsoft)])
    jobs = []
    for i in range(len(nsoft)):
        n = int(nsoft[i]) // 6 * 6
        L = (n // 6 * 5 - 22) // 8
        if 1 <= L <= limit:
            jobs.append((soft[offs[i]:offs[i] + n].copy(), L))
    return jobs


class Cases:
    def __init__(self):
        rng = np.random.default_rng(56)
        self.lengths = [random_job(rng, L, extra=L % 3) for L in LENGTHS] + [clean_job(rng, L, extra=(L + 1) % 3) for L in LENGTHS]
        # pairs: (short, long), (long, short), (equal, equal), and an odd tail
        self.pairs = [random_job(rng, 5), clean_job(rng, 100), wrap_job(rng, 98), random_job(rng, 3), clean_job(rng, 51), random_job(rng, 51), random_job(rng, 27),
                      clean_job(rng, 26), wrap_job(rng, 60)]
        self.adversarial = constant_jobs(40) + constant_jobs(99) + [wrap_job(rng, L) for L in (75, 300, 700)] + golden_jobs()
        self.long = [random_job(rng, 4000), clean_job(rng, 4000), wrap_job(rng, 1500)]
        # streams that end before their frame does (whole windows only, nothing at the end), beside whole ones; ragged tails (1..5 values short of a group)
        s, L = random_job(rng, 100)
        t, _ = clean_job(rng, 100)
        self.cut = [(s[:6 * 50], L), (t, L), (s, L), (t[:6 * 90 + 3], L), (s[:len(s) - 1], L), (s[:5], L), (t[:6], L)]

    def all(self):
        return self.lengths + self.pairs + self.adversarial + self.long + self.cut


@pytest.fixture(scope="module")
def cases():
    c = Cases()
    c.want = {id(j[0]): vm.viterbi_frame(j[0], vm.CR_56, j[1]) for j in c.all()}
    for s, L in c.lengths + c.pairs + c.adversarial + c.long:
        assert len(c.want[id(s)]) == L + 2                                   # a whole frame each
    return c


def run(sora, torch, jobs, align=0, gap=0, slack=0, junk=None):
    """one stage call over `jobs`, their streams back to back from byte `align` with `gap` bytes between them and `slack` bytes behind the last -> [n, OUT_STRIDE]"""
    offs, o = [], align
    for s, _ in jobs:
        offs.append(o); o += len(s) + gap
    buf = np.full(o - gap + slack, 0xA5, np.uint8)                           # (what lies between the streams is no soft value)
    for (s, _), off in zip(jobs, offs):
        buf[off:off + len(s)] = s
    if junk is not None:
        buf |= (junk.integers(0, 32, len(buf)) << 3).astype(np.uint8)
    d = torch.from_numpy(buf).cuda()
    out = sora.viterbi56_11n(d, torch.tensor(offs, dtype=torch.int32).cuda(), torch.tensor([len(s) for s, _ in jobs], dtype=torch.int32).cuda(),
                             torch.tensor([L for _, L in jobs], dtype=torch.int16).cuda(), out_stride=OUT_STRIDE)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def check(got, jobs, cases, what):
    for i, (s, L) in enumerate(jobs):
        w = cases.want[id(s)]
        g = got[i, :len(w)]
        if not np.array_equal(g, w):
            bad = np.nonzero(g != w)[0]
            pytest.fail("%s: job %d of %d (length %d, %d soft values) differs from the model at byte %d (%d of %d bytes differ)"
                        % (what, i, len(jobs), L, len(s), bad[0], len(bad), len(w)))
        assert not got[i, len(w):].any(), "%s: job %d (length %d): bytes behind the model's %d were written" % (what, i, L, len(w))


def test_lengths_at_the_schedules_corners(sora, torch_cuda, cases):
    check(run(sora, torch_cuda, cases.lengths, slack=64), cases.lengths, cases, "lengths")


def test_pairs_whose_sides_end_apart_and_an_odd_count(sora, torch_cuda, cases):
    assert len(cases.pairs) % 2 == 1
    check(run(sora, torch_cuda, cases.pairs, slack=64), cases.pairs, cases, "pairs")
    rev = cases.pairs[::-1]
    check(run(sora, torch_cuda, rev, slack=64), rev, cases, "pairs reversed")


@pytest.mark.parametrize("k", range(4))
def test_a_single_job(sora, torch_cuda, cases, k):
    jobs = [(cases.lengths + cases.pairs)[(1, 6, 20, 35)[k]]]
    check(run(sora, torch_cuda, jobs, slack=k), jobs, cases, "n = 1")


def test_adversarial_streams_and_metric_wrap(sora, torch_cuda, cases):
    assert len(cases.adversarial) >= 20
    check(run(sora, torch_cuda, cases.adversarial, slack=64), cases.adversarial, cases, "adversarial")


def test_four_thousand_bytes(sora, torch_cuda, cases):
    check(run(sora, torch_cuda, cases.long, slack=64), cases.long, cases, "long")


def test_unaligned_offsets_and_junk_above_the_low_three_bits(sora, torch_cuda, cases):
    jobs = cases.lengths + cases.pairs
    check(run(sora, torch_cuda, jobs, align=1, gap=3, slack=5), jobs, cases, "align 1, gap 3")
    check(run(sora, torch_cuda, jobs, align=7, gap=1, slack=64, junk=np.random.default_rng(7)), jobs, cases, "junk in the high bits")


def test_a_stream_that_ends_exactly_at_the_span(sora, torch_cuda, cases):
    """no slack behind the last stream, which is the longer side of its pair, then the shorter, then alone"""
    for jobs in ([cases.pairs[0], cases.pairs[1]], [cases.pairs[1], cases.pairs[0]], [cases.lengths[3]], cases.lengths[:5]):
        check(run(sora, torch_cuda, jobs, slack=0), jobs, cases, "no slack")


def test_streams_that_end_before_their_frame_and_ragged_tails(sora, torch_cuda, cases):
    check(run(sora, torch_cuda, cases.cut, slack=0), cases.cut, cases, "cut streams")
    rev = cases.cut[::-1]
    check(run(sora, torch_cuda, rev, slack=9), rev, cases, "cut streams reversed")


def test_arguments(sora, torch_cuda, cases):
    import ctypes
    L = sora.load()
    p = ctypes.c_void_p(256)
    assert L.sora_hip_viterbi56_11n(None, 64, p, p, p, p, p, 1, None) == -1 and b"sora_hip_viterbi56_11n" in L.sora_hip_last_error()
    assert L.sora_hip_viterbi56_11n(p, 64, p, p, p, p, p, 0, None) == 0                      # nothing to do
    assert L.sora_hip_viterbi56_11n(p, 0, p, p, p, p, p, 1, None) == -1
    assert L.sora_hip_viterbi56_11n(p, 1 << 32, p, p, p, p, p, 1, None) == -6
    assert L.sora_hip_viterbi56_11n(p, 64, p, p, p, p, p, 1 << 31, None) == -6
