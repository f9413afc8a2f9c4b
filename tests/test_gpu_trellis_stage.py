"""Every trellis kernel through its stage call, bit-exact against the oracle on adversarial soft streams (tests/trellis_streams.py).

Six kernels -- k_viterbi, k_viterbi16, k_viterbi16w + k_win_redo (sora_hip_viterbi11a_ws: T11aViterbi<..,256,24>, three bits per value after k_soft_pack3)
and k_viterbi11n, k_viterbi16_11n, k_viterbi16w_11n + k_win_redo_11n (sora_hip_viterbi11n_ws: T11aViterbi<..,192,36>, one byte per value) -- times three
code rates times the families: ties, metric wrap, bursts across unit boundaries, lengths at the schedule's corners, batch geometry and format junk.
Every decoded byte of every job (length + 2) is compared with Oracle.viterbi_frame / viterbi_frame_ex(.., 192, 36), computed once per module.
The window-parallel kernels' proof record (sora_hip_viterbi_window_stats) must show no failed boundary on noiseless codewords, and both failed and
held boundaries where bursts end at verify points."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import trellis_streams as ts

pytestmark = pytest.mark.gpu

W = 1                                   # SORA_TRELLIS_WINDOWED
KERNELS = [("11a", 64, "k_viterbi"), ("11a", 16, "k_viterbi16"), ("11a", W, "k_viterbi16w+k_win_redo"),
           ("11n", 64, "k_viterbi11n"), ("11n", 16, "k_viterbi16_11n"), ("11n", W, "k_viterbi16w_11n+k_win_redo_11n")]
KIDS = [k[2] for k in KERNELS]
RATES = (0, 1, 2)
OUT_STRIDE = 4112                       # room for a 4095-byte frame's 4097 bytes
STATS = {}                              # (family, kernel, rate) -> proof record, printed at the end of the module


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


class Expected:
    """the oracle's bytes for each (family, rate, schedule), computed on first use"""
    def __init__(self, oracle):
        self.o, self.cache = oracle, {}
        self.o.viterbi_frame(np.zeros(64, np.uint8), 0, 1)         # (its tables are set up once, before any thread runs it)

    def __call__(self, key, jobs, cr, sched):
        k = (key, cr, sched)
        if k not in self.cache:
            win, look = ts.SCHEDULES[sched]
            f = (lambda j: self.o.viterbi_frame(j[0], cr, j[1])) if sched == "11a" else (lambda j: self.o.viterbi_frame_ex(j[0], cr, j[1], win, look))
            with ThreadPoolExecutor(8) as ex:
                self.cache[k] = list(ex.map(f, jobs, chunksize=64))
            assert all(len(w) == L + 2 for w, (_, L) in zip(self.cache[k], jobs))
        return self.cache[k]


@pytest.fixture(scope="module")
def expected(oracle):
    yield Expected(oracle)
    for k in sorted(STATS):
        print("proof record %-8s %-32s rate %d: boundaries %d, failed %d, decoded again %d, units %d" % (k + STATS[k]))


def run(sora, torch, jobs, cr, sched, lanes, order="forward", align=0, gap=0, junk=None):
    """one stage call over `jobs` -> (decoded bytes [n, OUT_STRIDE], proof record or None)"""
    buf, offs, ns, lens = ts.layout(jobs, order, align, gap)
    if junk is not None:
        buf |= (junk.integers(0, 32, len(buf)) << 3).astype(np.uint8)
    d = torch.from_numpy(buf).cuda()
    n = len(jobs)
    args = (torch.from_numpy(offs.astype(np.int32)).cuda(), torch.from_numpy(ns.astype(np.int32)).cuda(), torch.from_numpy(lens.astype(np.int16)).cuda())
    wsb = (sora.viterbi11a_workspace_bytes if sched == "11a" else sora.viterbi11n_workspace_bytes)(d.numel(), n)
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    call = sora.viterbi11a_ws if sched == "11a" else sora.viterbi11n_ws
    out = call(d, *args, cr, ws, out_stride=OUT_STRIDE, lanes_per_pair=lanes)
    stats = sora.viterbi_window_stats(ws) if lanes == W else None
    torch.cuda.synchronize()
    return out.cpu().numpy(), stats


def check(got, want, kernel, family, cr, jobs=None):
    for i, w in enumerate(want):
        g = got[i, :len(w)]
        if not np.array_equal(g, w):
            bad = np.nonzero(g != w)[0]
            pytest.fail("%s, family %s, rate %d: job %d of %d (length %d) differs from the oracle at byte %d (%d bytes differ)"
                        % (kernel, family, cr, i, len(want), len(w) - 2, bad[0], len(bad)))


def record(family, kernel, cr, stats):
    if stats is not None:
        prev = STATS.get((family, kernel, cr), (0, 0, 0, 0))
        STATS[(family, kernel, cr)] = tuple(a + b for a, b in zip(prev, stats))


@pytest.mark.parametrize("cr", RATES)
@pytest.mark.parametrize("kernel", KERNELS, ids=KIDS)
def test_ties_and_metric_wrap(sora, torch_cuda, expected, kernel, cr):
    """families 1 and 2: not codewords -- bytes only (the proof may fail anywhere; what fails is decoded again)"""
    sched, lanes, name = kernel
    for fam, jobs in (("ties", ts.ties(cr)), ("wrap", ts.wrap(cr))):
        got, st = run(sora, torch_cuda, jobs, cr, sched, lanes)
        check(got, expected(fam, jobs, cr, sched), name, fam, cr)
        record(fam, name, cr, st)


@pytest.mark.parametrize("cr", RATES)
@pytest.mark.parametrize("kernel", KERNELS, ids=KIDS)
def test_bursts_across_unit_boundaries(sora, torch_cuda, expected, kernel, cr):
    """family 3: a burst longer than the warm-up ends just before, at or just after a verify point, in calls whose unit plans put the verify
    points there (1 job: units of one window; 64 jobs: one window; 4096 jobs: several windows, beside short fillers).  The windowed kernels'
    record must show failed AND held boundaries, and the bytes must still be the oracle's."""
    sched, lanes, name = kernel
    for njobs, nburst in ((1, 1), (64, 64), (4096, 96)):
        jobs, where = ts.bursts(cr, sched, njobs, nburst, seed=3 + njobs)
        if njobs > nburst:
            jobs = jobs + ts.batch(cr, njobs - nburst, seed=9)
            jobs = [(s, min(L, 63)) if i >= nburst and L > 63 else (s, L) for i, (s, L) in enumerate(jobs)]
        got, st = run(sora, torch_cuda, jobs, cr, sched, lanes)
        check(got, expected("bursts%d" % njobs, jobs, cr, sched), name, "bursts (%d jobs)" % njobs, cr)
        record("bursts%d" % njobs, name, cr, st)
        if st is not None and njobs > 1:
            boundaries, failed, again, units = st
            assert units > njobs and boundaries == units - njobs
            assert 0 < failed < boundaries and 0 < again <= nburst, (name, cr, njobs, st)


@pytest.mark.parametrize("cr", RATES)
@pytest.mark.parametrize("kernel", KERNELS, ids=KIDS)
def test_lengths_at_schedule_corners(sora, torch_cuda, expected, kernel, cr):
    """family 4: every length 1..100, every residue of the step count modulo the window and 24 / 36 near 1000, 2304 and 4095 bytes, surplus
    symbols; noiseless codewords, so the window-parallel proof must hold at every boundary"""
    sched, lanes, name = kernel
    jobs = ts.lengths(cr, sched)
    for order in ("forward", "shuffle"):
        got, st = run(sora, torch_cuda, jobs, cr, sched, lanes, order=order)
        check(got, expected("lengths", jobs, cr, sched), name, "lengths (%s)" % order, cr)
        record("lengths", name, cr, st)
        if st is not None:
            assert st[1] == 0 and st[2] == 0 and st[3] >= len(jobs), (name, cr, st)


@pytest.mark.parametrize("cr", RATES)
@pytest.mark.parametrize("kernel", KERNELS, ids=KIDS)
def test_batch_geometry(sora, torch_cuda, expected, kernel, cr):
    """family 5: job counts around the wave (8 jobs), pair and 16-lane row sizes and the unit target, mixed lengths, the streams back to back
    in forward, reverse or shuffled offset order"""
    sched, lanes, name = kernel
    for k, n in enumerate(ts.BATCH_COUNTS):
        jobs = ts.batch(cr, n)
        order = ("forward", "reverse", "shuffle")[k % 3]
        got, st = run(sora, torch_cuda, jobs, cr, sched, lanes, order=order)
        check(got, expected("batch%d" % n, jobs, cr, sched), name, "batch of %d (%s)" % (n, order), cr)
        record("batch", name, cr, st)
        if st is not None:
            assert st[1] == 0 and st[2] == 0, (name, cr, n, st)


@pytest.mark.parametrize("cr", RATES)
@pytest.mark.parametrize("kernel", KERNELS, ids=KIDS)
def test_format_junk(sora, torch_cuda, expected, kernel, cr):
    """family 6: junk in the upper five bits of every byte (only the low three are soft values), jobs at every byte alignment -- odd offsets
    for the 802.11a stage's packer, every offset modulo 16 for the 802.11n kernels that read the bytes themselves"""
    sched, lanes, name = kernel
    jobs = ts.lengths(cr, sched)[:100] + ts.batch(cr, 17, seed=11)
    want = expected("junk", jobs, cr, sched)
    rng = np.random.default_rng(100 + cr)
    for align in ((1, 3) if sched == "11a" else (0, 1, 2, 3, 5, 8, 13)):
        got, st = run(sora, torch_cuda, jobs, cr, sched, lanes, align=align, gap=7 if sched == "11n" else 3, junk=rng)
        check(got, want, name, "format junk (first job at byte %d)" % align, cr)
        record("junk", name, cr, st)
        if st is not None:
            assert st[1] == 0 and st[2] == 0, (name, cr, align, st)


def test_stage_refuses_bad_arguments(sora, torch_cuda):
    torch = torch_cuda
    soft = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    args = (torch.zeros(1, dtype=torch.int32, device="cuda"), torch.full((1,), 2000, dtype=torch.int32, device="cuda"), torch.ones(1, dtype=torch.int16, device="cuda"))
    for call, wsb in ((sora.viterbi11a_ws, sora.viterbi11a_workspace_bytes), (sora.viterbi11n_ws, sora.viterbi11n_workspace_bytes)):
        ws = torch.empty(wsb(soft.numel(), 1), dtype=torch.uint8, device="cuda")
        for bad in (2, 8, 32, 65):
            with pytest.raises(sora.SoraError):
                call(soft, *args, 0, ws, lanes_per_pair=bad)
        with pytest.raises(sora.SoraError):
            call(soft, *args, 3, ws)
        with pytest.raises(sora.SoraError):
            call(soft, *args, 0, ws[:wsb(soft.numel(), 1) - 16])
    assert sora.viterbi11n_workspace_bytes(4096, 16385) > sora.viterbi11n_workspace_bytes(4096, 1)
