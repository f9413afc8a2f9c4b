"""What tests/test_gpu_ht40_gi_soft.py and tests/test_gpu_ht40_gi_stages.py share: frames of the numpy model of the format (oracle/py_ht40.py, tests/ht40_joint_model.py)
from HT-LTF 1 on, long or with the short guard interval (every data symbol: the last 16 of its 128 samples, then the 128), through a 2x2 channel; their placement in a
buffer with random filler around them; their descriptors; and tests/ht40_gi_model.py run over a call's descriptors.  TEST INFRASTRUCTURE."""
import numpy as np

from oracle import py_ht40 as m
import ht40_gi_model as G
import ht40_joint_model as J

H0 = np.array([[1.0 * np.exp(0.3j), 0.35 * np.exp(-1.1j)], [0.3 * np.exp(2.0j), 0.9 * np.exp(-0.4j)]])
SHORT = 0x100
ROW_SHORT_GI = 4
SHAPES = [(1, 1), (2, 2), (4, 40), (6, 1), (1, 40), (2, 1), (4, 2), (6, 40), (6, 2), (4, 1), (2, 41), (1, 2)]      # (n_bpsc, N_SYM)
RATES = {1: (2, 0), 2: (0, 2), 4: (2, 0), 6: (1, 2)}
CFOS = (0, 37, 4096, -511)


def symbols(lens, nb, cr, joint):
    return J.nsym_for(lens[0], nb, cr) if joint else m.nsym_for(list(lens), nb, cr)


def lengths(rng, nb, cr, nsym, joint, longer):
    """PSDU lengths (FCS included) that need exactly nsym symbols: two different ones per stream (the longer in stream `longer`), or one (joint: (len, 0))"""
    nd = m.ndbps(nb, cr) * (2 if joint else 1)
    top = min(4000, (nsym * nd - 22) // 8); low = max(5, ((nsym - 1) * nd - 22) // 8 + 1)
    assert low <= top, (nb, cr, nsym, joint)
    big = int(rng.integers(low, top + 1))
    if joint:
        return (big, 0)
    small = int(rng.integers(4, big))
    return (small, big) if longer else (big, small)


def frame(rng, nb, cr, lens, gi, joint, sigma, cfo):
    """a numpy-model frame from HT-LTF 1 on, long or short, through the 2x2 channel with the carrier offset the descriptor will state -> int16 [2, 320 + pitch nsym, 2], psdus"""
    if joint:
        ps = [m.add_fcs(rng.integers(0, 256, lens[0] - 4, dtype=np.uint8).tobytes())]
        x, nsym = J.tx_joint(ps[0], nb, cr, int(rng.integers(1, 128)))
    else:
        ps = [m.add_fcs(rng.integers(0, 256, ln - 4, dtype=np.uint8).tobytes()) for ln in lens]
        x, nsym = m.tx(ps, nb, cr, seeds=(int(rng.integers(1, 128)), int(rng.integers(1, 128))))
    if gi:
        sym = x.reshape(2, 2 + nsym, 160)
        data = sym[:, 2:, 32:]
        x = np.concatenate([sym[:, :2].reshape(2, -1), np.concatenate([data[:, :, -16:], data], axis=2).reshape(2, -1)], axis=1)
    assert x.shape[1] == 320 + (144 if gi else 160) * nsym
    return m.channel(x, H0, sigma, rng, cfo_step=-float(cfo)), ps


def bank(joint):
    """every shape as a long and as a short frame, ordered L S S L | S L L S | ..., so that every workgroup of four holds both kinds"""
    rng = np.random.default_rng(5100 + joint)
    out = []
    for i, (nb, nsym) in enumerate(SHAPES):
        cr = RATES[nb][i & 1]
        if joint and ((nsym - 1) * 2 * m.ndbps(nb, cr) - 22) // 8 + 1 > 4000:
            cr = 0                                                         # (one PSDU of at most 4000 bytes over both streams: the long shapes at rate 1/2)
        for k in range(2):
            gi = (k + i) & 1
            lens = lengths(rng, nb, cr, nsym, joint, (i + k) & 1)
            assert symbols(lens, nb, cr, joint) == nsym
            cfo = CFOS[(i + 2 * k) % 4]; nv = (0.0, 3000.0)[sum(1 for b, _ in SHAPES[:i] if b == nb) & 1]      # per n_bpsc: zero forcing, MMSE, zero forcing
            seg, ps = frame(rng, nb, cr, lens, gi, joint, 6.0, cfo)
            out.append({"seg": seg, "nb": nb, "cr": cr, "lens": lens, "gi": gi, "cfo": cfo, "nv": nv, "ps": ps, "nsym": nsym})
    return out


def place(rng, frames, residues):
    """-> (iq int16 [2, N, 2], offsets): frame i at an offset whose residue mod 4 is residues[i % len]; random filler in front of, between and behind the frames, at
    least 16 nsym + 64 samples behind each"""
    parts, offs, pos = [], [], 0
    for i, f in enumerate(frames):
        gap = 3 + (residues[i % len(residues)] - (pos + 3)) % 4
        parts.append(rng.integers(-300, 301, (2, gap, 2)).astype(np.int16)); pos += gap
        offs.append(pos); parts.append(f["seg"]); pos += f["seg"].shape[1]
        tail = 16 * f["nsym"] + 64
        parts.append(rng.integers(-300, 301, (2, tail, 2)).astype(np.int16)); pos += tail
    return np.concatenate(parts, axis=1), offs


def descs(frames, offs, flagged=True):
    return [(offs[i], f["nb"], f["cr"] | (SHORT if (f["gi"] and flagged) else 0), f["lens"][0], f["lens"][1], f["cfo"], f["nv"], 200 + i) for i, f in enumerate(frames)]


def capacity(frames):
    return sum(2 * (f["nsym"] * 108 * f["nb"] + 64) for f in frames)


class JointWant:
    """ht40_gi_model.Result in the shape ht40_soft_check.assert_is_the_joint_model reads"""
    def __init__(self, r):
        self.soft, self.nsym, self.theta, self.xs = r.soft, r.nsym, r.theta, r.xs
        self.error_code, self.crc32, self.psdu = r.streams[0].error_code, r.streams[0].crc32, r.streams[0].psdu


def models(joint, iq, descs, w):
    out = []
    for f, d in enumerate(descs):
        r = G.model(iq, d[0], d[1], d[2] & ~SHORT, d[3] if joint else (d[3], d[4]), d[5], w[f], gi=1 if d[2] & SHORT else 0, joint=bool(joint))
        out.append(JointWant(r) if joint else r)
    return out
