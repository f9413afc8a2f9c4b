"""The carrier-sense streams that tests/test_11n_stage_model_cpu.py counts branches on and tests/test_gpu_11n_rx_stages.py runs on the GPU: the same lists, so that the GPU
test cannot pass by never reaching a branch.  Built from the reference modulator's recorded frames (tests/golden/refgraph_11n.npz: what ReferenceGraph.tx11n wrote) with the
L-STF cut or repeated, behind leads of every length mod 8 at 40 MHz, and from random streams at the rails and near silence.  Every stream is a pair of int16 [4 n, 2] arrays
at 20 MHz (behind TDownSample2).  TEST INFRASTRUCTURE."""
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "refgraph_11n.npz")
FRAME_BURSTS = 400                       # a recorded frame's worth of 20 MHz bursts (tx1: 2880 samples at 40 MHz = 360 bursts), and then some


def _noise(rng, n, sigma):
    return rng.normal(0, sigma, n) + 1j * rng.normal(0, sigma, n)


def _i16(c):
    return np.stack([np.clip(np.rint(c.real), -32768, 32767), np.clip(np.rint(c.imag), -32768, 32767)], axis=1).astype(np.int16)


def capture40(rng, frames, leads, sigma=20.0, tail=400, stf=None, gain=1.0):
    """two chains at 40 MHz: frames [(s0, s1)] each behind its lead of noise; stf: None, or the number of 40 MHz L-STF samples to keep (< 320: cut from the front) or to
    have (> 320: the first 16-sample period repeated in front)"""
    seg0, seg1 = [], []
    for (s0, s1), lead in zip(frames, leads):
        c0 = gain * (s0[:, 0] + 1j * s0[:, 1]); c1 = gain * (s1[:, 0] + 1j * s1[:, 1])
        if stf is not None and stf < 320:
            c0 = c0[320 - stf:]; c1 = c1[320 - stf:]
        elif stf is not None:
            k = (stf - 320 + 31) // 32
            c0 = np.concatenate([np.tile(c0[:32], k), c0]); c1 = np.concatenate([np.tile(c1[:32], k), c1])
        seg0 += [np.zeros(lead, complex), c0]; seg1 += [np.zeros(lead, complex), c1]
    a = np.concatenate(seg0 + [np.zeros(tail, complex)]); b = np.concatenate(seg1 + [np.zeros(tail, complex)])
    n = (len(a) + 27) // 28 * 28
    a = np.concatenate([a, np.zeros(n - len(a), complex)]) + _noise(rng, n, sigma); b = np.concatenate([b, np.zeros(n - len(b), complex)]) + _noise(rng, n, sigma)
    return _i16(a), _i16(b)


def down2(x):
    """TDownSample2 over whole bursts: the even samples"""
    n = len(x) // 8 * 8
    return np.ascontiguousarray(x[:n:2])


def built_streams():
    """-> [(name, x0, x1)] at 20 MHz"""
    z = np.load(GOLD)
    f = [(z["tx%d_0" % i], z["tx%d_1" % i]) for i in range(4)]
    rng = np.random.default_rng(1106)
    out = []
    for r in range(16):                                                      # one frame behind leads of every length mod 8 (twice over): the deciding lane moves
        a, b = capture40(rng, [f[r % 3]], [600 + 37 * r + (r % 8) - (37 * r) % 8], sigma=[20.0, 60.0][r & 1])
        out.append(("lead%d" % r, down2(a), down2(b)))
    for r in range(8):                                                       # a second frame behind the first: the ring has slipped when it comes
        a, b = capture40(rng, [f[0], f[1]], [300 + r, 500 + 3 * r])
        out.append(("two%d" % r, down2(a), down2(b)))
    for r, keep in enumerate((120, 160, 192, 200)):                          # an L-STF of 60 .. 100 samples at 20 MHz: a fake plateau
        a, b = capture40(rng, [f[1]], [500 + r], stf=keep)
        out.append(("short%d" % keep, down2(a), down2(b)))
    for r, have in enumerate((416, 480, 640, 960)):                          # an L-STF of 208 .. 480 samples at 20 MHz: too many peaks
        a, b = capture40(rng, [f[2]], [500 + r], stf=have)
        out.append(("long%d" % have, down2(a), down2(b)))
    a, b = capture40(rng, [f[0]], [3 + 28 * 0], tail=200)                    # the frame inside the first 64 samples' LLONG_MAX ring
    out.append(("early", down2(a), down2(b)))
    for k in range(3):                                                       # at +-32767; at the int16 rails, where the squared norm itself wraps; and mixed with a frame
        n = 4 * (150 + 50 * k)
        out.append(("full%d" % k, (rng.choice([-32767, 32767], (n, 2))).astype(np.int16), (rng.choice([-32767, 32767], (n, 2))).astype(np.int16)))
        out.append(("rail%d" % k, (rng.choice([-32768, 32767], (n, 2))).astype(np.int16), (rng.choice([-32768, -32768, 32767], (n, 2))).astype(np.int16)))
    a, b = capture40(rng, [f[1]], [700], gain=60.0, sigma=3000.0)            # a frame driven into the rails
    out.append(("overdriven", down2(a), down2(b)))
    out.append(("allmin", np.full((4 * 120, 2), -32768, np.int16), np.full((4 * 120, 2), -32768, np.int16)))
    for k in range(3):                                                       # |x| <= 3: every >> 5 term is 0
        n = 4 * (100 + 77 * k)
        out.append(("silent%d" % k, rng.integers(-3, 4, (n, 2)).astype(np.int16), rng.integers(-3, 4, (n, 2)).astype(np.int16)))
    for k in range(4):                                                       # plain noise at four levels, with steps of level (rises without a plateau)
        n = 4 * (200 + 111 * k)
        lvl = np.repeat(rng.choice([5.0, 40.0, 400.0, 4000.0], n // 40 + 1), 40)[:n]
        out.append(("steps%d" % k, _i16(_noise(rng, n, 1.0) * lvl), _i16(_noise(rng, n, 1.0) * lvl)))
    return out


def lengths_streams(rng, tile_bursts=64):
    """-> [(x0, x1)] of 0, 1, 2, 15 .. 1000 bursts and the tile size +- 1: noise with a step of level in the last third, so that short streams see rises too"""
    out = []
    for nb in (0, 1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1000, tile_bursts - 1, tile_bursts, tile_bursts + 1, 2 * tile_bursts - 1, 2 * tile_bursts + 1):
        n = 4 * nb
        lvl = np.where(np.arange(n) >= 2 * n // 3, 900.0, 30.0)
        out.append((_i16(_noise(rng, n, 1.0) * lvl), _i16(_noise(rng, n, 1.0) * lvl)))
    return out
