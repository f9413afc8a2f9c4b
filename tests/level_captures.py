"""Capture families at the levels where saturating and wrapping integer arithmetic part ways: overdriven up to a square wave, DC-shifted,
near-silent, and the int16 rails themselves -- for the 802.11a (40 and 44 MHz), 802.11b and 802.11n 2x2 receive chains.

Every capture is built with integer arithmetic only (gain = multiply and arithmetic shift, integer DC, noise from Generator.integers, phases by
multiples of 90 degrees), so any machine regenerates it bit for bit; tests/golden/refgraph_levels.npz (make_golden.py levels) holds a sha256 of each
capture and the events the compiled reference graphs reported for it.  A regeneration mismatch is reported as such by recorded().

Waveforms: 802.11a from Oracle.tx_capture (sample-exact to the reference modulator, tests/test_oracle_vs_refgraph.py); 802.11b and 802.11n from the
reference modulator's recorded output (refgraph_11b.npz, refgraph_11b_cck.npz, refgraph_11n.npz, refmod_11n_mcs11_14.npz).

What the reference graphs make of the families, counted on the reference alone by `make_golden.py levels` (a frame: FRAME_OK or CRC32_FAIL;
tests/test_oracle_levels.py asserts the floors on the recorded events):
  11a    overdriven  64 captures,  45 with a frame,   6 without an event; events 0x1: 50, 0x80000005: 39, 0x80000006: 25
  11a    offset      32 captures,  32 with a frame,   0 without an event; events 0x1: 57, 0x80000006: 8
  11a    silent      96 captures,  40 with a frame,  56 without an event; events 0x1: 79
  11a    rails       16 captures,  10 with a frame,   5 without an event; events 0x1: 16, 0x80000005: 3, 0x80000006: 2
  11a    stream       1 captures,   1 with a frame,   0 without an event; events 0x1: 12
  11a44  overdriven  64 captures,  46 with a frame,  10 without an event; events 0x1: 55, 0x80000005: 19, 0x80000006: 23
  11a44  offset      32 captures,  32 with a frame,   0 without an event; events 0x1: 54, 0x80000005: 3, 0x80000006: 7
  11a44  silent      96 captures,  32 with a frame,  64 without an event; events 0x1: 63
  11a44  rails       16 captures,  10 with a frame,   6 without an event; events 0x1: 17, 0x80000005: 1, 0x80000006: 2
  11a44  stream       1 captures,   1 with a frame,   0 without an event; events 0x1: 12
  11b    overdriven  42 captures,  21 with a frame,   0 without an event; events 0x1: 11, 0x80000004: 3, 0x80000006: 13, 0x80000008: 16, 0x80000009: 1041
  11b    offset      18 captures,  18 with a frame,   0 without an event; events 0x1: 21, 0x80000006: 2, 0x80000008: 2, 0x80000009: 35
  11b    silent      80 captures,  40 with a frame,  40 without an event; events 0x1: 55
  11b    rails       16 captures,  10 with a frame,   0 without an event; events 0x1: 12, 0x80000006: 1, 0x80000009: 75
  11b    stream       1 captures,   1 with a frame,   0 without an event; events 0x1: 8, 0x80000006: 2, 0x80000009: 26
  11n    overdriven  96 captures,  74 with a frame,   1 without an event; events 0x1: 96, 0x80000005: 82, 0x80000006: 13
  11n    offset      45 captures,  29 with a frame,   8 without an event; events 0x1: 42, 0x80000005: 29
  11n    silent     104 captures,  41 with a frame,  33 without an event; events 0x1: 58, 0x80000005: 74, 0x80000006: 3
  11n    rails       16 captures,   8 with a frame,   7 without an event; events 0x1: 10, 0x80000005: 5, 0x80000006: 4
  11n    stream       1 captures,   1 with a frame,   0 without an event; events 0x1: 9, 0x80000005: 6
Thresholds, measured on the reference alone (gain = what scale() applies to the modulator's output, peak 26112 for 802.11a):
  802.11a  at 40 MHz every frame is found down to gain 7/16 and none from 13/32 down; behind the 44 -> 40 MHz resampler down to 15/32, none from 7/16 down.
           From gain 3 up FRAME_OK, PLCP_HEADER_FAIL and CRC32_FAIL occur side by side.  Under a DC of 30000 on either component every capture still yields a frame.
  802.11b  frames are found down to gain 3/64 and none from 1/32 down; under a DC of 25000 every capture still yields one.  Overdrive raises SYNC_TIMEOUT (0x80000009) events by
           the dozen (up to 76 in one capture), which is what MAX_EVENTS["11b"] is sized for.
  802.11n  TCCA11n compares an auto-correlation with an energy, so it has no absolute threshold: frames decode down to gain 1/32 (peak about 270 LSB), gains
           1/64 .. 1/256 still raise events but only header failures, and from 1/512 down (peak 17 LSB) nothing is reported.  A DC of up to 1000 on both
           components of both chains still yields frames; 1500 silences the graph unless it steps in after carrier sense (DC_11N ends there).
"""
import hashlib
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = os.path.join(GOLD, "refgraph_levels.npz")
MAX_EVENTS = {"11a": 32, "11a44": 32, "11b": 128, "11n": 32}   # per capture, for the references and the handles' max_frames_per_capture alike: no recorded list reaches it
CHAINS = ("11a", "11a44", "11b", "11n")
FAMILIES = ("overdriven", "offset", "silent", "rails", "stream")
RATES_11A = (6000, 9000, 12000, 18000, 24000, 36000, 48000, 54000)
E_OK, E_PLCP, E_CRC = 0x1, 0x80000005, 0x80000006

OVER_11A = ((5, 2), (3, 1), (2, 0), (3, 0), (4, 0), (8, 0), (30, 0), (128, 0))          # gain = num / 2^shift; x128 turns every non-zero sample into a rail
SILENT_11A = ((3, 2), (5, 3), (1, 1), (15, 5), (7, 4), (13, 5), (3, 3), (11, 5), (1, 2), (1, 4), (1, 8), (1, 13))
DC_11A = (2000, 8000, 20000, 30000)
OVER_11B = ((3, 1), (2, 0), (3, 0), (4, 0), (8, 0), (30, 0), (128, 0))
SILENT_11B = ((1, 2), (1, 3), (3, 5), (1, 4), (3, 6), (1, 5), (1, 6), (1, 7), (1, 10), (1, 13))
DC_11B = (3000, 10000, 25000)
OVER_11N = ((2, 0), (3, 0), (4, 0), (6, 0), (8, 0), (10, 0), (12, 0), (16, 0), (20, 0), (30, 0), (60, 0), (256, 0))
SILENT_11N = ((1, 0), (1, 1), (1, 2), (1, 3), (1, 4), (1, 5), (1, 6), (1, 7), (1, 8), (1, 9), (1, 10), (1, 12), (1, 13))
DC_11N = (100, 300, 600, 1000, 1500)
STREAM_OF = (("silent", 0), ("overdriven", 1), ("offset", 2), ("silent", 9), ("overdriven", 13), ("offset", 7), ("rails", 12), ("silent", 3))   # the stream capture: these, back to back


class Cap:
    """one capture: name, family, iq (int16 [n,2]; the 802.11n chain: a pair of them)"""
    def __init__(self, name, family, iq):
        self.name, self.family, self.iq = name, family, iq

    def sha(self):
        h = hashlib.sha256()
        for x in (self.iq if isinstance(self.iq, tuple) else (self.iq,)):
            assert x.dtype == np.int16 and x.ndim == 2 and x.shape[1] == 2 and len(x) % 28 == 0
            h.update(np.ascontiguousarray(x).tobytes())
        return h.digest()


# ------------------------------------------------------------------ integer signal operations
def _rng(chain, k):
    return np.random.default_rng([20261017, CHAINS.index(chain), k])


def _clip(y):
    return np.clip(y, -32768, 32767).astype(np.int16)


def scale(x, num, shift):
    """gain num / 2^shift: multiply, arithmetic shift (floor), clip"""
    return _clip((x.astype(np.int32) * num) >> shift)


def add_dc(x, di, dq, start=0):
    y = x.astype(np.int32); y[start:, 0] += di; y[start:, 1] += dq
    return _clip(y)


def add_noise(x, rng, amp):
    return _clip(x.astype(np.int32) + rng.integers(-amp, amp + 1, size=x.shape)) if amp else x


def rot90(x, k):
    """x * j^k, exact (a rail of -32768 clips to 32767 when negated)"""
    y = x.astype(np.int32)
    for _ in range(k % 4):
        y = np.stack([-y[:, 1], y[:, 0]], 1)
    return _clip(y)


_ROTOR = {}


def spin(x, step):
    """a carrier offset without a sine: x[n] z[n] >> 30 with the integer rotor z[0] = 2^30, z[n + 1] = z[n] (c + j step) >> 30, c = 2^30 - step^2 / 2^31 (the cosine to
    second order, so the rotor keeps its length), i.e. step / 2^30 rad per sample"""
    if not step:
        return x
    if len(_ROTOR.get(step, ())) < len(x):                                  # (grown to the longest frame asked for; a longer one begins as the shorter one did)
        re, im, z, c = 1 << 30, 0, [], (1 << 30) - (step * step >> 31)
        for _ in range(max(len(x), 1 << 14)):
            z.append((re, im)); re, im = (re * c - im * step) >> 30, (im * c + re * step) >> 30
        _ROTOR[step] = np.array(z, np.int64)
    z = _ROTOR[step][:len(x)]; y = x.astype(np.int64)
    return _clip(np.stack([(y[:, 0] * z[:, 0] - y[:, 1] * z[:, 1]) >> 30, (y[:, 0] * z[:, 1] + y[:, 1] * z[:, 0]) >> 30], 1))


def whole(x, q=28):
    n = -(-len(x) // q) * q
    return np.ascontiguousarray(np.concatenate([x, np.zeros((n - len(x), 2), np.int16)]) if n != len(x) else x)


def zeros(n):
    return np.zeros((n, 2), np.int16)


def up44(x40):
    """a 44 MHz capture of the same signal: linear interpolation in integers (x[i] (11 - f) + x[i + 1] f + 5) // 11 at position k 10/11 = i + f/11"""
    n = len(x40) * 11 // 10 // 28 * 28
    p = np.arange(n, dtype=np.int64) * 10
    i = np.minimum(p // 11, len(x40) - 2); f = (p - 11 * i)[:, None]
    x = x40.astype(np.int64)
    return _clip((x[i] * (11 - f) + x[i + 1] * f + 5) // 11)


class _Set:
    """The captures of one chain in the making.  wave(rng, k) -> the k-th clean capture (one array, or a pair for the two-chain graph); every capture draws from a
    generator of its own, seeded by the chain and its place in the set, and a clean capture is drawn before anything else."""
    def __init__(self, chain, wave):
        self.chain, self.wave, self.pair, self.out = chain, wave, chain == "11n", []

    def each(self, f, x):
        """f on every chain of a capture"""
        return tuple(f(c) for c in x) if self.pair else f(x)

    def emit(self, name, family, make, clean=True):
        """make(rng, x) -> the capture, x the clean capture of this place (None where clean is False: the place is counted all the same)"""
        k = len(self.out); rng = _rng(self.chain, k)
        x = make(rng, self.wave(rng, k) if clean else None)
        self.out.append(Cap("%s/%s" % (family, name), family, self.each(whole, x)))

    def of(self, family):
        return [c for c in self.out if c.family == family]


def _overdriven(s, gains, per_gain):
    """through the onset of clipping up to a square wave, bare and under noise of +-300 and +-3000"""
    for num, sh in gains:
        for v in range(per_gain):
            def make(rng, x, num=num, sh=sh, amp=(0, 300, 0, 3000)[v % 4]):
                return s.each(lambda c: add_noise(scale(c, num, sh), rng, amp), x)
            s.emit("x%d>>%d.%d" % (num, sh, v), "overdriven", make)


def _offset(s, dcs, both):
    """DC towards either rail of I and of Q separately, of both at once (where `both`), stepping in inside a frame, and -- two chains -- on one chain alone"""
    signs = ((1, 0), (-1, 0), (0, 1), (0, -1)) + (((1, -1), (-1, -1)) if both else ())
    for d in dcs:
        for v, (si, sq) in enumerate(signs):
            s.emit("dc%d.%d" % (d, v), "offset", lambda rng, x, di=si * d, dq=sq * d: s.each(lambda c: add_dc(c, di, dq), x))
        for v, (si, sq) in enumerate(((1, 0), (0, -1))):
            def step(rng, x, di=si * d, dq=sq * d):
                at = len(x[0] if s.pair else x) // 2 + int(rng.integers(-200, 200))
                return s.each(lambda c: add_dc(c, di, dq, start=at), x)
            s.emit("dcstep%d.%d" % (d, v), "offset", step)
        if s.pair:
            s.emit("dc%d.a" % d, "offset", lambda rng, x, d=d: (add_dc(x[0], d, -d), x[1]))


def _silent(s, gains, floor):
    """around the carrier-sense threshold and down to 1-3 LSB, bare and on a noise floor of +-floor in turn"""
    for num, sh in gains:
        for v in range(8):
            def make(rng, x, num=num, sh=sh, amp=floor if v % 2 else 0):
                return s.each(lambda c: add_noise(scale(c, num, sh), rng, amp), x)
            s.emit("x%d>>%d.%d" % (num, sh, v), "silent", make)


def _rails(s):
    """constant rails and rail noise without a frame; frames whose ONLY extreme value is -32768; a frame between stretches of constant rail"""
    n = 28 * 120
    both = np.array([-32768, 32767], np.int16)

    def const(i, q):
        return np.ascontiguousarray(np.broadcast_to(np.array([i, q], np.int16), (n, 2)))
    for name, one in (
            ("+rail", lambda rng: const(32767, 32767)), ("-rail", lambda rng: const(-32768, -32768)), ("+-rail", lambda rng: const(32767, -32768)),
            ("rail noise", lambda rng: both[rng.integers(0, 2, size=(n, 2))]),
            ("full-range noise", lambda rng: rng.integers(-32768, 32768, size=(n, 2)).astype(np.int16)),
            ("rail bursts", lambda rng: (both[rng.integers(0, 2, size=(n, 2))] * (np.arange(n) // 160 % 2)[:, None]).astype(np.int16))):
        s.emit(name, "rails", lambda rng, x, one=one: (one(rng), one(rng)) if s.pair else one(rng), clean=False)
    for count in (1, 1, 3, 3, 40, 40):
        def lone(rng, x, count=count):
            def put(c):
                c = c.copy()
                for p in rng.choice(np.flatnonzero(np.abs(c).sum(1)), size=count, replace=False):
                    c[p, int(rng.integers(0, 2))] = -32768
                return c
            return s.each(put, x)
        s.emit("lone -32768 x%d" % count, "rails", lone)
    for v, level in enumerate(((32767, 32767), (-32768, -32768), (32767, -32768), (-32768, 32767))):
        def fenced(rng, x, r=const(*level)[:28 * (20 + 10 * v)]):
            return s.each(lambda c: np.concatenate([r, zeros(28 * 30), c, r]), x)
        s.emit("rail, frame, rail %d" % v, "rails", fenced)


def _stream(s, members):
    """one long capture for the stream-continuation runs: the captures (family, index) of `members` back to back, then a quiet tail, so that the end of the
    stream raises nothing"""
    def make(rng, x):
        parts = [s.of(f)[i].iq for f, i in members] + [s.each(lambda c: add_noise(zeros(28 * 150), rng, 2), (0, 0) if s.pair else 0)]
        return tuple(np.concatenate([p[c] for p in parts]) for c in range(2)) if s.pair else np.concatenate(parts)
    s.emit("every family", "stream", make, clean=False)


def _families(chain, wave, over, per_gain, dcs, dc_both, silent, members):
    s = _Set(chain, wave)
    _overdriven(s, over, per_gain)
    _offset(s, dcs, dc_both)
    _silent(s, silent, floor=2)
    _rails(s)
    _stream(s, members)
    return s.out


# ------------------------------------------------------------------ the chains
def chain_11a(oracle):
    """802.11a at 40 MHz: one to three frames per capture, all eight rates in turn"""
    def wave(rng, k):
        parts = []
        for j in range(1 + k % 3):
            rate = RATES_11A[(k + 3 * j) % 8]; ln = (14, 60, 150, 33)[(k // 8 + j) % 4]
            mp = rng.integers(0, 256, ln).astype(np.uint8).tobytes()
            parts.append(oracle.tx_capture(mp, rate, seed=int(rng.integers(1, 128)), lead=int(rng.integers(0, 120)), tail=int(rng.integers(40, 400))))
        return np.concatenate(parts)
    return _families("11a", wave, OVER_11A, 8, DC_11A, True, SILENT_11A, STREAM_OF)


def chain_11a44(oracle):
    """the same captures as a 44 MHz receiver would have sampled them (CreateDemodGraph11a_44M)"""
    return [Cap(c.name, c.family, whole(up44(c.iq))) for c in chain_11a(oracle)]


def _tx11b():
    w = []
    for f in ("refgraph_11b.npz", "refgraph_11b_cck.npz"):
        z = np.load(os.path.join(GOLD, f))
        w += [z["tx_%d" % i].astype(np.int16) << 8 for i in range(int(z["frames"]))]
    return w                                                                # 1, 1, 1, 2, 2, 2, 5.5, 5.5, 5.5, 11, 11, 11 Mbps


def chain_11b():
    """802.11b at 44 MHz: the twelve recorded frames (1, 2, 5.5, 11 Mbps) in turn, every fourth capture two or three of them"""
    tx = _tx11b(); short = (0, 3, 6, 9, 7, 10)
    def wave(rng, k):
        idx = [(5 * k) % 12] if k % 4 else [short[(k // 4 + j) % 6] for j in range(2 + k // 4 % 2)]
        parts = [zeros(int(rng.integers(0, 2000)))]
        for i in idx:
            parts += [tx[i], zeros(int(rng.integers(1600, 2800)))]
        return np.concatenate(parts + [zeros(1200)])
    return _families("11b", wave, OVER_11B, 6, DC_11B, False, SILENT_11B, STREAM_OF[:6])


def _tx11n():
    z = np.load(os.path.join(GOLD, "refgraph_11n.npz")); m = np.load(os.path.join(GOLD, "refmod_11n_mcs11_14.npz"))
    w = [(z["tx%d_0" % i], z["tx%d_1" % i]) for i in range(4)]            # MCS 8, 9, 10, 12
    return w + [(m["tx%d_0" % i], m["tx%d_1" % i]) for i in (11, 13, 14, 9)]


def chain_11n():
    """802.11n 2x2 at 40 MHz: MCS 8, 9, 10 (decoded), 12 (refused at the reference's gate), then 11, 13, 14 and a short MCS 9 frame; one to three frames per
    capture; the channel is a rotation of each chain by a multiple of 90 degrees, cross-talk of 0, 1/8 or 1/4 and a carrier offset (spin)"""
    tx = _tx11n(); order = (0, 1, 2, 3, 0, 1, 2, 4, 5, 6, 7)
    def wave(rng, k):
        a, b = [], []
        for j in range(1 + k % 3):
            s0, s1 = tx[order[(k + 4 * j) % len(order)]]
            xs = (None, 3, 2)[(k // 3 + j) % 3]; gap = zeros(int(rng.integers(200, 1500)))
            r0 = s0.astype(np.int32) + ((s1.astype(np.int32) >> xs) if xs else 0); r1 = s1.astype(np.int32) + ((s0.astype(np.int32) >> xs) if xs else 0)
            cfo = (0, 300000, -1200000, 4000000, -300000, 1200000, -4000000)[(k + j) % 7]   # up to 0.0037 rad per sample (24 kHz), both chains alike
            a += [gap, spin(rot90(_clip(r0), k + j), cfo)]; b += [gap, spin(rot90(_clip(r1), 3 * k + j), cfo)]
        return np.concatenate(a + [zeros(600)]), np.concatenate(b + [zeros(600)])
    return _families("11n", wave, OVER_11N, 8, DC_11N, True, SILENT_11N, STREAM_OF)


def chain(name, oracle=None):
    return {"11a": lambda: chain_11a(oracle), "11a44": lambda: chain_11a44(oracle), "11b": chain_11b, "11n": chain_11n}[name]()


# ------------------------------------------------------------------ events: one canonical form for the reference, the oracle and the GPU rows
def _payload(chain, code):
    """whether rate, length, FCS word and MPDU of an event are compared (elsewhere the reference reports what an earlier frame left in its context)"""
    return code != E_PLCP if chain == "11n" else code in (E_OK, E_CRC)


def event(chain, code, pos, rate=0, length=0, crc=0, mpdu=b""):
    if not _payload(chain, code):
        return (code, pos, 0, 0, 0, "")
    if chain == "11b":
        crc &= 0xFFFFFF                                                     # the top byte of the reference's FCS word is a stale buffer byte (PHY_11b.hpp:725-731)
    return (code, pos, rate, length, crc, hashlib.sha256(mpdu).digest()[:8].hex())


def reference_events(chain, ev):
    """events of oracle.pyoracle.ReferenceGraph -> canonical"""
    return [event(chain, e["error_code"], e["sample_index"], e["rate_kbps"], e["length"], e["crc32"], e["mpdu"]) for e in ev]


def row_events(chain, rows):
    """rows of the oracle or of a GPU handle -> canonical (the 802.11a rows carry a 20 MHz sample index: the reference's event falls at the end of the source call)"""
    from gpu_util import source_position, source_position_44
    pos = {"11a": source_position, "11a44": source_position_44}.get(chain, lambda p: p)
    return [event(chain, r["error_code"], pos(r["end_sample"]), r["rate_kbps"], r["length"], r["crc32"], r["mpdu"]) for r in rows]


def run_reference(graph, chain, cap):
    if chain == "11n":
        ev = graph.rx11n(cap.iq[0], cap.iq[1], max_frames=MAX_EVENTS[chain])
    else:
        ev = {"11a": graph.rx11a, "11a44": graph.rx11a_44, "11b": graph.rx11b}[chain](cap.iq, max_frames=MAX_EVENTS[chain])
    assert len(ev) < MAX_EVENTS[chain], "%s %s: the reference's event list is cut short" % (chain, cap.name)
    return reference_events(chain, ev)


def run_oracle(oracle, chain, cap):
    if chain == "11n":
        rows = oracle.rx11n_capture(cap.iq[0], cap.iq[1], max_frames=MAX_EVENTS[chain])
    elif chain == "11b":
        rows = oracle.rx11b_capture(cap.iq, max_frames=MAX_EVENTS[chain])
    elif chain == "11a44":
        x = oracle.down44to40(cap.iq)
        rows = oracle.rx_capture(x[:len(x) // 28 * 28], 44, max_frames=MAX_EVENTS[chain])
    else:
        rows = oracle.rx_capture(cap.iq, 40, max_frames=MAX_EVENTS[chain])
    return row_events(chain, rows)


def recorded(chain, caps):
    """the recorded reference events of every capture of `caps`, after checking that the captures are the recorded ones"""
    z = np.load(FIXTURE)
    sha = z[chain + "_sha"]
    assert len(sha) == len(caps), "%s: %d captures regenerated, %d recorded -- regenerate tests/golden/refgraph_levels.npz" % (chain, len(caps), len(sha))
    for c, s in zip(caps, sha):
        assert c.sha() == s.tobytes(), "%s %s: the regenerated capture is not the recorded one (a regeneration mismatch, not a receiver difference)" % (chain, c.name)
    out, k = [], 0
    for n in z[chain + "_count"]:
        out.append([(int(z[chain + "_code"][j]), int(z[chain + "_pos"][j]), int(z[chain + "_rate"][j]), int(z[chain + "_length"][j]), int(z[chain + "_crc"][j]),
                     z[chain + "_mpdu"][j].tobytes().hex() if _payload(chain, int(z[chain + "_code"][j])) else "") for j in range(k, k + int(n))])
        k += int(n)
    return out


def pack(chain, caps, events):
    """-> the arrays recorded() reads"""
    flat = [e for ev in events for e in ev]
    return {chain + "_sha": np.stack([np.frombuffer(c.sha(), np.uint8) for c in caps]), chain + "_count": np.array([len(ev) for ev in events], np.uint8),
            chain + "_code": np.array([e[0] for e in flat], np.uint32), chain + "_pos": np.array([e[1] for e in flat], np.uint32),
            chain + "_rate": np.array([e[2] for e in flat], np.uint16), chain + "_length": np.array([e[3] for e in flat], np.uint16),
            chain + "_crc": np.array([e[4] for e in flat], np.uint32),
            chain + "_mpdu": np.stack([np.frombuffer(bytes.fromhex(e[5] or "00" * 8), np.uint8) for e in flat]) if flat else np.zeros((0, 8), np.uint8)}


def census(caps, events):
    """per family: captures, captures in which a frame is reported (FRAME_OK or CRC32_FAIL), captures without any event, events per code"""
    out = {}
    for c, ev in zip(caps, events):
        f = out.setdefault(c.family, {"captures": 0, "framed": 0, "mute": 0, "codes": {}})
        f["captures"] += 1; f["framed"] += any(e[0] in (E_OK, E_CRC) for e in ev); f["mute"] += not ev
        for e in ev:
            f["codes"][e[0]] = f["codes"].get(e[0], 0) + 1
    return out
