"""The capture set the 40 MHz HT front end (k_scan_ht40, k_ht40_plan) is held to its integer model on (tests/test_gpu_ht40_front.py), and whose reach the model
alone is asked about first (tests/test_ht40_front_model_cpu.py: the census).  Frames are py_ht40's (tx_frame's waveform, restated here so that the SIG fields can
lie: a wrong parity bit, a wrong CRC-8, MCS 7 and 15, CBW 20, LENGTH 3 and 4001, an L-SIG LENGTH of 751); levels, DC, noise and rotations are tests/level_captures.py's integer
operations.  Where a case depends on the receiver's own timing -- a frame that ends on the capture's last sample, a capture that ends behind 0, 1 or 2 SIG
symbols -- the cut is placed with the model's a20; the census then asserts that the branch was reached.  TEST INFRASTRUCTURE."""
import numpy as np

from oracle import py_ht40 as m
import ht40_front_model as fm
import ht40_joint_model as J
from level_captures import add_dc, add_noise, rot90, scale, spin, whole, zeros

PRE = 1280                                             # samples in front of HT-LTF 1: L-STF 320, L-LTF 320, L-SIG 160, HT-SIG 320, HT-STF 160
H_UNIT = np.eye(2)
H_MIX = np.array([[1.0, 0.3j], [-0.25, 0.9j]])         # cross-talk and quarter turns: exact in the float channel up to its rounding
MAX_EVENTS = 8                                         # max_frames_per_capture of the GPU runs: no capture of the set but `slots` raises as many


class Cap:
    """one capture: name, family, iq = the two chains (int16 [n, 2], n a multiple of 28), sent = [{mcs, length, nsym, htstf (40 MHz sample of the first HT-STF
    sample), psdus, tag}], tags = what the census expects this capture to reach"""
    def __init__(self, name, family, iq, sent=(), tags=()):
        self.name, self.family, self.iq, self.sent, self.tags = name, family, iq, list(sent), set(tags)
        assert iq[0].shape == iq[1].shape and len(iq[0]) % 28 == 0 and iq[0].dtype == np.int16


# ------------------------------------------------------------------ frames
def preamble(ht_mcs, ht_len, nsym, cbw40=1, bad_parity=False, bad_crc=False, l_length=None):
    """py_ht40.tx_frame's legacy part, HT-SIG and HT-STF with the SIG fields as given -> complex128 [1280]"""
    if l_length is None:
        l_length = max(1, -(-(36 + 4 * nsym + 4 - 20) // 4) * 3 - 3)
    stf = np.fft.ifft(m._dup40(m._STF)) * 128.0
    ltf = np.fft.ifft(m._dup40(m._LTF)) * 128.0
    parts = [np.tile(stf, 3)[:320], np.concatenate([ltf[-64:], ltf, ltf])]
    lb = m.l_sig_bits(l_length)
    if bad_parity:
        lb[17] ^= 1
    a, b = m.encode(lb)
    sym = np.fft.ifft(m._dup40(m._leg_symbol(np.stack([a, b], 1).reshape(-1), False, 1.0))) * 128.0
    parts.append(np.concatenate([sym[-32:], sym]))
    hb = m.ht_sig_bits(ht_mcs, ht_len, cbw40)
    if bad_crc:
        hb[34] ^= 1
    a, b = m.encode(hb)
    coded = np.stack([a, b], 1).reshape(-1)
    for h in range(2):
        sym = np.fft.ifft(m._dup40(m._leg_symbol(coded[48 * h:48 * h + 48], True, 1.0))) * 128.0
        parts.append(np.concatenate([sym[-32:], sym]))
    parts.append(np.tile(stf, 2)[:160])
    return np.concatenate(parts)


def frame(rng, mcs, length, joint=False, **sig):
    """a frame whose data field is MCS `mcs` with PSDUs of `length` bytes (FCS included); sig: ht_mcs / ht_len override what HT-SIG says, cbw40, bad_parity,
    bad_crc, l_length (the L-SIG LENGTH field) -> (complex128 [2, n], nsym, psdus)"""
    nb, cr = m.MCS2[mcs]
    if joint:
        ps = [m.add_fcs(rng.integers(0, 256, length - 4, dtype=np.uint8).tobytes())]
        data, nsym = J.tx_joint(ps[0], nb, cr, seed=int(rng.integers(1, 128)))
    else:
        ps = [m.add_fcs(rng.integers(0, 256, length - 4, dtype=np.uint8).tobytes()) for _ in range(2)]
        data, nsym = m.tx(ps, nb, cr, seeds=(int(rng.integers(1, 128)), int(rng.integers(1, 128))))
    pre = preamble(sig.pop("ht_mcs", mcs), sig.pop("ht_len", length), nsym, **sig)
    return np.concatenate([np.stack([pre, pre]), data], axis=1), nsym, ps


def through(x, H=H_MIX, cfo_step=0.0, amp=250.0):
    """the float channel without noise -> the two chains, int16 [n, 2] each"""
    y = m.channel(x, H, 0.0, None, scale=amp, cfo_step=cfo_step)
    return y[0], y[1]


def gauss(pair, rng, sigma):
    """a noise floor of `sigma` LSB per component"""
    if not sigma:
        return pair
    return tuple(np.clip(np.rint(c + rng.normal(0, sigma, c.shape)), -32768, 32767).astype(np.int16) for c in pair)


def each(f, pair):
    return tuple(f(c) for c in pair)


def cat(*pairs):
    return tuple(np.concatenate([p[c] for p in pairs]) for c in range(2))


def quiet(n):
    return (zeros(n), zeros(n))


def step_lengths(mcs, lo=4, hi=200, joint=False):
    """two PSDU lengths in lo..hi on both sides of a symbol-count step of `mcs`: (L, L + 1) with one more data symbol for L + 1"""
    nb, cr = m.MCS2[mcs]
    ns = (lambda L: J.nsym_for(L, nb, cr)) if joint else (lambda L: m.nsym_for([L, L], nb, cr))
    steps = [L for L in range(lo, hi) if ns(L + 1) == ns(L) + 1]
    return steps[len(steps) // 2], steps[len(steps) // 2] + 1


class _Set:
    def __init__(self, seed, joint=False):
        self.out, self.seed, self.joint = [], seed, joint

    def rng(self):
        return np.random.default_rng([20261019, self.seed, len(self.out)])

    def one(self, name, family, mcs, length, lead=400, tail=600, H=H_MIX, cfo_step=0.0, sigma=0.0, post=None, tags=(), rng=None, **sig):
        """one frame in a capture: lead zeros, the frame, tail zeros; post(pair, rng) -> pair is applied to the whole, then the noise floor"""
        rng = rng or self.rng()
        x, nsym, ps = frame(rng, mcs, length, self.joint, **sig)
        pair = cat(quiet(lead), through(x, H, cfo_step), quiet(tail))
        if post:
            pair = post(pair, rng)
        pair = each(whole, gauss(pair, rng, sigma))
        sent = [{"mcs": sig.get("ht_mcs", mcs), "length": sig.get("ht_len", length), "nsym": nsym, "htstf": lead + PRE - 160, "psdus": ps, "sound": not sig}]
        self.out.append(Cap(name, family, pair, sent, tags))
        return self.out[-1]

    def add(self, name, family, pair, sent=(), tags=()):
        self.out.append(Cap(name, family, each(whole, pair), sent, tags))
        return self.out[-1]


def _model_first(cap, joint):
    ev = fm.front(cap.iq[0], cap.iq[1], flags=fm.OWN | (fm.JOINT if joint else 0))
    return ev[0] if ev else None


def build(joint=False, full=True):
    """-> [Cap].  joint: the frames are joint-coded (one PSDU) and the cuts follow the joint symbol count; full=False: a representative third of the set"""
    s = _Set(1 if joint else 0, joint)
    # ---- plain: every MCS, lengths on both sides of a symbol-count step, a 10 LSB floor
    for mcs in range(8, 15):
        for L in step_lengths(mcs, joint=joint):
            s.one("mcs%d len%d" % (mcs, L), "plain", mcs, L, lead=300 + 4 * mcs, sigma=10.0, tags={"mcs%d" % mcs})
    s.one("mcs14 len4000", "plain", 14, 4000, sigma=10.0)
    if full:
        s.one("mcs8 len4", "plain", 8, 4, sigma=10.0)
        s.one("mcs13 len200", "plain", 13, 200, H=H_UNIT, sigma=10.0)
    # ---- overdriven: gains that clip, up to a square wave
    for num in ((3, 8, 30, 256) if full else (8, 256)):
        for amp in (0, 300):
            s.one("x%d noise%d" % (num, amp), "overdriven", 9 + num % 5, 60 + num % 50,
                  post=lambda p, rng, num=num, amp=amp: each(lambda c: add_noise(scale(c, num, 0), rng, amp), p))
    # ---- rails and constants (level_captures._rails' recipe)
    n = 28 * 120
    both = np.array([-32768, 32767], np.int16)
    const = lambda i, q: np.ascontiguousarray(np.broadcast_to(np.array([i, q], np.int16), (n, 2)))
    for name, one in (("+rail", lambda rng: const(32767, 32767)), ("-rail", lambda rng: const(-32768, -32768)), ("+-rail", lambda rng: const(32767, -32768)),
                      ("rail noise", lambda rng: both[rng.integers(0, 2, size=(n, 2))]),
                      ("full-range noise", lambda rng: rng.integers(-32768, 32768, size=(n, 2)).astype(np.int16)),
                      ("rail bursts", lambda rng: (both[rng.integers(0, 2, size=(n, 2))] * (np.arange(n) // 160 % 2)[:, None]).astype(np.int16)),
                      ("constant 1", lambda rng: const(1, -1))):
        rng = s.rng()
        s.add(name, "rails", (one(rng), one(rng)))
    for v, level in enumerate(((32767, 32767), (-32768, -32768), (32767, -32768), (-32768, 32767))[:4 if full else 2]):
        r = const(*level)[:28 * (20 + 10 * v)]
        s.one("rail, frame, rail %d" % v, "rails", 10 + v, 90, lead=0, tail=0, post=lambda p, rng, r=r: each(lambda c: np.concatenate([r, zeros(28 * 30), c, r]), p))
    for count in (1, 3, 40):
        # frames whose only extreme value is -32768, at kept samples with m odd (40 MHz sample 2 mod 4) inside the L-LTF: the derotation's negate meets it
        def lone(p, rng, count=count):
            out = []
            for c in p:
                c = c.copy()
                at = 400 + 320 + 2 + 4 * rng.choice(80, size=count, replace=False)
                c[at, rng.integers(0, 2, size=count)] = -32768
                out.append(c)
            return tuple(out)
        s.one("lone -32768 x%d" % count, "rails", 11, 77, lead=400, post=lone, tags={"neg_rail"})
    # ---- DC on one chain and on both
    for d in ((100, 600, 1500) if full else (600,)):
        s.one("dc%d both" % d, "dc", 12, 100, post=lambda p, rng, d=d: each(lambda c: add_dc(c, d, -d), p))
        s.one("dc%d chain 0" % d, "dc", 13, 100, post=lambda p, rng, d=d: (add_dc(p[0], d, d), p[1]))
        s.one("dc%d steps in" % d, "dc", 9, 100, post=lambda p, rng, d=d: each(lambda c: add_dc(c, 0, d, start=400 + 700), p))
    # ---- near-silent: a peak of a few LSB, bare and on a floor of +-2
    for sh in ((5, 6, 7, 8, 9, 10) if full else (6, 9)):
        for amp in (0, 2):
            s.one("x1>>%d noise%d" % (sh, amp), "silent", 8 + sh % 7, 50, post=lambda p, rng, sh=sh, amp=amp: each(lambda c: add_noise(scale(c, 1, sh), rng, amp), p))
    # ---- noise floors: none, the 4 - 6 LSB at which carrier sense fires on the frame's own first samples, 10 LSB
    for sigma in (0.0, 4.0, 5.0, 6.0, 10.0):
        for k in range(1 if sigma in (0.0, 10.0) else (6 if full else 2)):
            s.one("floor %g.%d" % (sigma, k), "floor", 8 + (k + int(sigma)) % 7, 40 + 9 * k, lead=400 + 28 * k, sigma=sigma, tags={"floor46"} if 4 <= sigma <= 6 else ())
    # ---- carrier offsets: none, +-40 kHz (65.5 per 40 MHz sample), up to the estimator's range (pi over 64 samples at 20 MHz: 256 per 40 MHz sample), and an
    # integer rotor (level_captures.spin)
    for k, cfo in enumerate((0.0, 65.5, -65.5, 21.0, -20.5, -37.25, 150.0, -200.0, 250.0, -255.0) if full else (65.5, -37.25, -255.0)):
        s.one("cfo %g" % cfo, "cfo", 8 + k % 7, 64 + k, cfo_step=cfo, sigma=3.0 * (k % 2), tags={"cfo"})
    s.one("spin -1200000", "cfo", 10, 80, post=lambda p, rng: each(lambda c: spin(c, -1200000), p), tags={"cfo"})
    s.one("spin 4000000 turned", "cfo", 12, 80, post=lambda p, rng: (spin(rot90(p[0], 1), 4000000), spin(rot90(p[1], 3), 4000000)), tags={"cfo"})
    # ---- the gate: each cause of a header failure
    for name, tag, sig in (("parity", "lsig_parity", {"bad_parity": True}), ("crc8", "ht_crc", {"bad_crc": True}), ("mcs7", "mcs_low", {"ht_mcs": 7}),
                           ("mcs15", "mcs_high", {"ht_mcs": 15}), ("cbw20", "cbw20", {"cbw40": 0}), ("len3", "len_short", {"ht_len": 3}),
                           ("len4001", "len_long", {"ht_len": 4001}), ("len4000 cut", "cut", {"ht_len": 4000}),
                           ("l-sig 751", "lsig_length", {"l_length": 751}), ("l-sig 750", "lsig_750", {"l_length": 750})):
        s.one("gate %s" % name, "gate", 9, 60, tags={tag}, **sig)
    # ---- the cut-offs, placed by the model's timing
    base_rng = s.rng()
    for lead in range(400, 400 + 8 * 14, 8):           # a20 moves in steps of 4 with the lead: one of seven leads puts the frame's end on a source-call boundary
        c = s.one("probe", "cut", 11, 150, lead=lead, tail=600, rng=np.random.default_rng([77, int(joint)]))
        s.out.pop()
        e = _model_first(c, joint)
        if e is None or e["error_code"]:
            continue
        end20 = e["a20"] + 240 + 80 * e["nsym"]
        if end20 % 14 == 0 and "exact" not in [t for k in s.out for t in k.tags]:
            s.add("ends on the last sample", "cut", each(lambda a: a[:2 * end20], c.iq), c.sent, {"exact"})
            s.add("ends 28 samples early", "cut", each(lambda a: a[:2 * end20 - 28], c.iq), c.sent, {"short28"})
        for k in range(3):                             # the capture ends behind k SIG symbols
            cut20 = e["a20"] - 240 + 80 * k
            if cut20 % 14 == 0 and ("flush%d" % k) not in [t for q in s.out for t in q.tags]:
                s.add("ends behind %d SIG symbols" % k, "cut", each(lambda a: a[:2 * cut20], c.iq), (), {"flush%d" % k})
    del base_rng
    for gap in range(300, 300 + 8 * 14, 8):            # the same behind a whole frame with the same header: what the SIG buffer still holds of it must not be read
        rng = np.random.default_rng([78, int(joint)])
        xa, nsa, psa = frame(rng, 10, 40, joint)
        xb, _, _ = frame(rng, 10, 40, joint)
        pair = each(whole, cat(quiet(400), through(xa), quiet(gap), through(xb), quiet(200)))
        ev = fm.front(pair[0], pair[1], flags=fm.OWN | (fm.JOINT if joint else 0))
        if len(ev) == 2 and ev[0]["error_code"] == 0 and ev[1]["error_code"] == 0 and (ev[1]["a20"] - 80) % 14 == 0:
            sent = [{"mcs": 10, "length": 40, "nsym": nsa, "htstf": 400 + PRE - 160, "psdus": psa, "sound": True}]
            s.add("a frame, then one that ends behind 2 SIG symbols", "cut", each(lambda a: a[:2 * (ev[1]["a20"] - 80)], pair), sent, {"flush2_behind_a_frame"})
            break
    s.one("ends inside the L-LTF", "cut", 9, 60, lead=400, tail=0, post=lambda p, rng: each(lambda c: c[:28 * 38], p))
    s.one("ends inside HT-SIG 2", "cut", 9, 60, lead=400, tail=0, post=lambda p, rng: each(lambda c: c[:28 * 56], p))
    s.one("ends inside the data field", "cut", 8, 200, lead=400, tail=0, post=lambda p, rng: each(lambda c: c[:28 * 90], p), tags={"cut"})
    # ---- several frames per capture, at gaps from nothing up
    for gaps in (((0, 8, 28), (28, 40, 56), (56, 100, 160), (200, 300, 444)) if full else ((28, 40, 56), (200, 300, 444))):
        rng = s.rng(); parts, sent, pos = [quiet(300)], [], 300
        for i, g in enumerate(gaps):
            mcs, L = 8 + (i + gaps[0]) % 7, 30 + 10 * i
            x, nsym, ps = frame(rng, mcs, L, joint)
            sent.append({"mcs": mcs, "length": L, "nsym": nsym, "htstf": pos + PRE - 160, "psdus": ps, "sound": True})
            parts += [through(x), quiet(g)]; pos += x.shape[1] + g
        s.add("three frames, gaps %s" % (gaps,), "several", gauss(cat(*parts, quiet(28 * 40)), rng, 8.0), sent, {"several"})
    rng = s.rng(); parts, sent, pos = [quiet(280)], [], 280
    for i in range(MAX_EVENTS + 2):                    # more events than row slots: short frames, every third with a header that fails
        x, nsym, ps = frame(rng, 9 + i % 5, 24 + i, joint, **({"bad_crc": True} if i % 3 == 2 else {}))
        sent.append({"mcs": 9 + i % 5, "length": 24 + i, "nsym": nsym, "htstf": pos + PRE - 160, "psdus": ps, "sound": i % 3 != 2})
        parts += [through(x), quiet(420)]; pos += x.shape[1] + 420
    s.add("%d events" % (MAX_EVENTS + 2), "several", gauss(cat(*parts), rng, 8.0), sent, {"slots"})
    return s.out


def layout(caps, offsets_mod8=4):
    """the captures in one buffer per chain, each at an offset that is a multiple of 4 but not of 8 nor of 28 (capture lengths are multiples of 28, so without
    the pads every offset would be one) -> (iq int16 [2, N, 2], [(offset, nsamples, id)])"""
    parts, descs, pos = [], [], 0
    for i, c in enumerate(caps):
        pad = 0
        while (pos + pad) % 8 != offsets_mod8 or (pos + pad) % 28 == 0:
            pad += 4
        parts.append(np.zeros((2, pad, 2), np.int16)); pos += pad
        descs.append((pos, len(c.iq[0]), 1000 + i))
        parts.append(np.stack(c.iq)); pos += len(c.iq[0])
    return np.concatenate(parts, axis=1), descs
