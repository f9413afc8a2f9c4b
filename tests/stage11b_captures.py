"""The capture set of the 802.11b stage tests (tests/test_11b_stage_model_cpu.py, tests/test_gpu_11b_stages.py, tests/test_gpu_11b_stage_hosts.py): 35 single-frame
captures that decode -- long preamble x {1, 2, 5.5, 11 Mbps}, short x {2, 5.5, 11}, MPDUs of 1, 5, 14, 33 and 120 bytes -- and 9 that do not, all from
tx11b_model.tx11b through rx11b_ext_model.capture; and the intermediate streams of one capture, brick by brick, from the stage model.  TEST INFRASTRUCTURE."""
import functools

import numpy as np

import rx11b_ext_model as rxm
import rx11b_stage_model as sm
import tx11b_model as txm
from sora_amd import capi

SEED = 1911
KINDS = [(0, 1000), (0, 2000), (0, 5500), (0, 11000), (1, 2000), (1, 5500), (1, 11000)]
LENGTHS = (1, 5, 14, 33, 120)


class Cap:
    def __init__(self, name, iq, mpdu=None, rate=0, preamble=0):
        self.name, self.iq, self.mpdu, self.rate, self.preamble = name, iq, mpdu, rate, preamble


def _negated(wave, symbol):
    w = wave.astype(np.int16)
    w[44 * symbol:44 * symbol + 44] *= -1
    return np.clip(w, -128, 127).astype(np.int8)


@functools.lru_cache(maxsize=None)
def captures():
    """-> (the 35 that decode, the 9 that do not)"""
    rng = np.random.default_rng(SEED)
    good = []
    for pre, rate in KINDS:
        for ln in LENGTHS:
            mp = rng.integers(0, 256, ln).astype(np.uint8).tobytes()
            w, _ = txm.tx11b(mp, rate, preamble=pre)
            iq = rxm.capture(rng, [w], [int(rng.integers(1500, 4001))], float(rng.uniform(0, 20)), scale=96)
            good.append(Cap("%s-%d-%d" % ("short" if pre else "long", rate, ln), iq, mp, rate, pre))
    bad = [Cap("noise10-%d" % k, rxm.capture(rng, [], [], 10.0, tail=6000)) for k in range(3)]
    bad += [Cap("noise1500-%d" % k, rxm.capture(rng, [], [], 1500.0, tail=6000)) for k in range(3)]
    mp = rng.integers(0, 256, 33).astype(np.uint8).tobytes()
    w, _ = txm.tx11b(mp, 1000, preamble=0)
    bad.append(Cap("header-symbol-negated", rxm.capture(rng, [_negated(w, 144 + 20)], [2000], 5.0, scale=96), mp, 1000))
    bad.append(Cap("payload-symbol-negated", rxm.capture(rng, [_negated(w, 144 + 48 + 77)], [2000], 5.0, scale=96), mp, 1000))
    bad.append(Cap("sync-cut", rxm.capture(rng, [w[:44 * 100]], [2000], 5.0, scale=96, tail=9000)))
    return good, bad


def all_captures():
    good, bad = captures()
    return good + bad


def batch():
    """-> (iq int16 [n, 2], descs) of the whole set back to back"""
    caps = all_captures()
    descs, at = [], 0
    for c in caps:
        descs.append((at, len(c.iq))); at += len(c.iq)
    return np.concatenate([c.iq for c in caps]), descs


@functools.lru_cache(maxsize=None)
def streams(index, mode=1):
    """The intermediate streams of capture `index` of all_captures(), as the composition routes them, from the stage model: a dict with
    front (up to 400 bursts from where the energy detector last started afresh), behind (DC-removed samples behind the switch), chips, synced (the chips behind
    TBarkerSync), sfd_symbols, and for a capture that decodes: payload_chips, rate, length, state (the stream record at the payload's first chip)."""
    c = all_captures()[index]
    rec = _Recorder()
    capi.rx11b_stages(rec, c.iq, [(0, len(c.iq))], mode)
    out = dict(rec.seen)
    out["front"] = c.iq[out["front_at"]:out["front_at"] + 4 * 400]
    return out


class _Recorder(sm.ModelOps):
    """the model's bricks, keeping what each stage of the walk was given"""

    def __init__(self):
        self.seen = {}

    def energy_detect(self, x, first, n, state):
        if int(state[0][10]) == 0:
            self.seen["front_at"] = int(first[0])
        return super().energy_detect(x, first, n, state)

    def symtiming(self, x, first, n, out_first, state, out):
        self.seen["behind"] = x[int(first[0]):int(first[0]) + 28 * int(n[0])].copy()
        st, nch = super().symtiming(x, first, n, out_first, state, out)
        self.seen["chips"] = out[:int(nch[0])].copy()
        return st, nch

    def barker_sync(self, x, first, n, state):
        st, used = super().barker_sync(x, first, n, state)
        self.seen["synced"] = x[int(used[0]):int(n[0])].copy()
        return st, used

    def sfd_sync(self, x, first, n, state, mode):
        self.seen["sfd_symbols"] = x[int(first[0]):int(first[0]) + int(n[0])].copy()
        return super().sfd_sync(x, first, n, state, mode)

    def stream_stage(self, kind, x, first, n, out_first, state, out):
        if kind != "desc741" and int(n[0]) != 6 or kind.startswith("cck"):
            per = 11 * sm.PER[kind] if kind in ("dbpsk", "dqpsk") else sm.PER[kind]
            self.seen["payload_kind"] = kind; self.seen["payload_state"] = np.array(state[0], np.int32)
            self.seen["payload_bytes"] = int(n[0])
            if kind.startswith("cck"):
                self.seen["payload_chips"] = x[int(first[0]):int(first[0]) + per * int(n[0])].copy()
        return super().stream_stage(kind, x, first, n, out_first, state, out)

    def despread(self, x, first, n, out_first, out):
        self.seen["last_despread_chips"] = x[int(first[0]):int(first[0]) + 11 * int(n[0])].copy()
        super().despread(x, first, n, out_first, out)


def drifting_stream(rng, nblocks, amp=6000, swing=14.0):
    """28 nblocks samples of random QPSK chips, 4 samples per chip, whose energy peaks mid-chip, sampled at an instant that slides late by `swing` samples over the
    first half and back past where it began over the second: TSymTiming's m_index follows it through 3 -> 4 -> 0 and through 0 -> -1 -> 3."""
    n = 28 * nblocks
    i = np.arange(n, dtype=np.float64)
    half = n / 2
    t = i + np.where(i < half, swing * i / half, swing - 2 * swing * (i - half) / half) + 2.0
    c = (rng.choice([-1, 1], n // 4 + 32) + 1j * rng.choice([-1, 1], n // 4 + 32)) * amp
    k = np.floor(t / 4).astype(np.int64) + 8
    frac = t / 4 - np.floor(t / 4)
    s = c[k] * (0.25 + 0.75 * np.cos(np.pi * (frac - 0.5)) ** 2)
    x = np.stack([s.real, s.imag], 1) + rng.normal(0, 30, (n, 2))
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)
