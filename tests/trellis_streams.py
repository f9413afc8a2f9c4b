"""Adversarial soft streams for the K=7 trellis (T11aViterbi<..,256,24> and <..,192,36>) and the unit plan of the window-parallel form.

Shared by tests/test_trellis_pin_cpu.py (oracle against the reference), tests/golden/make_golden.py (the recorded subset) and
tests/test_gpu_trellis_stage.py (every trellis kernel against the oracle).  A job is (soft, length): soft values 0..7, one per byte,
a whole number of puncture groups, and enough of them for the frame's length + 2 decoded bytes.  Soft value 7 is a confident 1.

The families (numbers as in the test's docstrings):
  1 ties    constant streams of every value, runs of the mid values 3 / 4 between codeword stretches (LSB tie-breaks, unsigned minimum)
  2 wrap    maximally confident contradictory values 0 / 7 for thousands of steps (the largest branch metrics: 8-bit metrics wrap)
  3 bursts  a clean codeword with a noise or inversion burst, longer than the warm-up, that ends just before, at or after a unit's verify point
  4 lengths every length 1..100, every residue of the frame's step count modulo the window and 24 / 36 near 1000, 2304 and 4095 bytes,
            one or two surplus symbols
  5 batches job counts around the wave and pair sizes, mixed lengths (whole waves of the window-parallel kernel empty)
"""
import math

import numpy as np

GB = (2, 3, 4)                  # soft values per puncture group, code rate 1/2, 2/3, 3/4
GS = (1, 2, 3)                  # trellis steps per group
SCHEDULES = {"11a": (256, 24), "11n": (192, 36)}
WARM = 144                      # sora_amd/csrc/rx_types.h kWinWarm
TARGET = 16384                  # the receive path's unit target (kWinUnitsTarget)
MAX_UNITS = 80                  # dev_winplan.h kWinMaxUnits
SYMBOL = {"11a": 48, "11n": 108}   # soft values of a surplus symbol (both a multiple of every group size)


# ---- the unit plan (sora_amd/csrc/dev_winplan.h, restated)
def win_events(length, cr, win, look):
    g = GS[cr]
    tr_end = length * 8 + 22
    top = (tr_end - 1) // g * g
    thr = win + look + 6
    return ((top - thr) // win + 1 if top >= thr else 0) + 1


def units_per_frame(njobs):
    return min(max(TARGET // max(njobs, 1), 1), MAX_UNITS)


def win_per_unit(nev, q):
    m = max((nev + q - 1) // q, 1)
    return (m + 2) // 3 * 3 if m >= 2 else m


def verify_points(length, cr, njobs, sched):
    """the steps at which units 1, 2, ... of a frame in a call of njobs jobs are proven (floor24(WIN k0))"""
    win, look = SCHEDULES[sched]
    nev = win_events(length, cr, win, look)
    m = win_per_unit(nev, units_per_frame(njobs))
    nun = (nev + m - 1) // m
    return [win * u * m // 24 * 24 for u in range(1, nun)]


# ---- streams
def nsoft_for(length, cr, surplus=0):
    """whole puncture groups up to the frame's last step (8 length + 22), + `surplus` soft values"""
    return -(-(length * 8 + 22) // GS[cr]) * GB[cr] + surplus


def codeword(rng, nsoft, cr):
    """a noiseless codeword of random bits, as soft values 0 / 7"""
    ng = nsoft // GB[cr]
    x = np.concatenate([np.zeros(6, np.uint8), rng.integers(0, 2, ng * GS[cr]).astype(np.uint8)])
    d = lambda k: x[6 - k:len(x) - k]
    a = d(0) ^ d(2) ^ d(3) ^ d(5) ^ d(6)                      # 133 (conv_enc.hpp:6-14)
    b = d(0) ^ d(1) ^ d(2) ^ d(3) ^ d(6)                      # 171
    if cr == 0:
        c = np.stack([a, b], 1)
    elif cr == 1:
        c = np.stack([a[0::2], b[0::2], a[1::2]], 1)
    else:
        c = np.stack([a[0::3], b[0::3], a[1::3], b[2::3]], 1)
    return (c.reshape(-1) * 7).astype(np.uint8)


def steps_to_soft(t, cr):
    """the first soft value of the group that holds trellis step t"""
    return t // GS[cr] * GB[cr]


def ties(cr, seed=1):
    rng = np.random.default_rng(seed * 10 + cr)
    jobs = []
    for v in range(8):
        for L in (40, 700):
            jobs.append((np.full(nsoft_for(L, cr), v, np.uint8), L))
    for i, L in enumerate((300, 1200, 2000)):
        for mid in (3, 4, "alt"):
            s = codeword(rng, nsoft_for(L, cr, 48), cr)
            pos = 60
            while pos < len(s) - 40:
                n = int(rng.integers(20, 600))
                seg = np.full(min(n, len(s) - pos), mid if mid != "alt" else 3, np.uint8)
                if mid == "alt":
                    seg[1::2] = 4
                s[pos:pos + len(seg)] = seg
                pos += len(seg) + int(rng.integers(30, 500))
            jobs.append((s, L))
    return jobs


def wrap(cr, seed=2):
    rng = np.random.default_rng(seed * 10 + cr)
    return [((rng.integers(0, 2, nsoft_for(L, cr, 48)) * 7).astype(np.uint8), L) for L in (600, 1500, 2000, 3000)]


BURST_ENDS = (-8, 0, 8, 64)     # where a burst ends, in steps from the verify point
BURST_LEN = (160, 240)          # burst length in steps (> WARM)


def bursts(cr, sched, njobs, nburst, length=1000, seed=3):
    """nburst frames of `length` bytes, each a codeword with ONE burst at one of its verify points (a different unit from frame to frame,
    later ones included); for a call of njobs jobs.  Returns (jobs, where): where[i] = (verify point, burst end offset, kind)."""
    rng = np.random.default_rng(seed * 100 + cr * 10 + len(sched))
    vps = verify_points(length, cr, njobs, sched)
    assert vps, "the frame has a single unit in this plan"
    jobs, where = [], []
    for i in range(nburst):
        s = codeword(rng, nsoft_for(length, cr, 48), cr)
        b = vps[(i * 5 + 1) % len(vps)] if i % 3 else vps[-1 - i % len(vps)]
        end = b + BURST_ENDS[i % len(BURST_ENDS)]
        blen = BURST_LEN[(i // len(BURST_ENDS)) % len(BURST_LEN)]
        lo, hi = steps_to_soft(max(end - blen, 0), cr), steps_to_soft(end, cr)
        kind = "noise" if (i // 2) % 2 == 0 else "invert"
        s[lo:hi] = rng.integers(0, 8, hi - lo) if kind == "noise" else 7 - s[lo:hi]
        jobs.append((s, length))
        where.append((b, end - b, kind))
    return jobs, where


def lengths(cr, sched, seed=4):
    """every length 1..100 (0, 1 or 2 surplus symbols); 32 consecutive lengths below 1000, 2304 and 4095 bytes (every residue of the
    frame's 8 L + 22 steps modulo 256 / 192 and 24 / 36), each with 0..2 surplus symbols; and at 1000 bytes every residue of the soft
    stream's step count modulo the window."""
    rng = np.random.default_rng(seed * 10 + cr)
    sym = SYMBOL[sched]
    jobs = [(codeword(rng, nsoft_for(L, cr, sym * (L % 3)), cr), L) for L in range(1, 101)]
    for L0 in (1000, 2304, 4095):
        jobs += [(codeword(rng, nsoft_for(L0 - d, cr, sym * (d % 3)), cr), L0 - d) for d in range(32)]
    win = SCHEDULES[sched][0]
    jobs += [(codeword(rng, nsoft_for(1000, cr, GB[cr] * e), cr), 1000) for e in range(win // math.gcd(GS[cr], win))]
    return jobs


BATCH_COUNTS = (1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 4095, 4096, 16385)


def batch(cr, n, seed=5):
    """n codeword jobs of mixed lengths: short frames next to long ones (every 13th is 1500 bytes and every 101st 2304; beyond 1000 jobs every
    211th is 1500 bytes)"""
    rng = np.random.default_rng(seed * 100000 + n * 10 + cr)
    jobs = []
    every = 13 if n < 1000 else 211
    for i in range(n):
        L = 2304 if i % 101 == 50 else 1500 if i % every == 6 else int(rng.integers(1, 64))
        jobs.append((codeword(rng, nsoft_for(L, cr, 48 * (i % 3)), cr), L))
    return jobs


def layout(jobs, order="forward", align=0, gap=0):
    """the jobs' streams back to back in one buffer (`gap` bytes between them, the first at byte `align`), in forward, reverse or shuffled
    offset order -> (buffer, offsets, nsoft, lengths), the job order unchanged"""
    n = len(jobs)
    place = list(range(n))
    if order == "reverse":
        place = place[::-1]
    elif order == "shuffle":
        place = list(np.random.default_rng(n).permutation(n))
    offs = [0] * n
    o = align
    for j in place:
        offs[j] = o
        o += len(jobs[j][0]) + gap
    buf = np.zeros(o + 64, np.uint8)
    for (s, _), off in zip(jobs, offs):
        buf[off:off + len(s)] = s
    return buf, np.array(offs, np.int64), np.array([len(s) for s, _ in jobs], np.int64), np.array([L for _, L in jobs], np.int64)
