"""Inputs shared by the CPU and GPU tests of the 802.11a front-end stages (tests/test_11a_stage_model_cpu.py, tests/test_gpu_11a_rx_stages.py): soft values of SIGNAL
symbols, SIGNAL words, and carrier-sense streams with the records they enter with.  Everything is seeded."""
import numpy as np

import scan_captures as sc
from sora_amd import capi

RATES = (6000, 9000, 12000, 18000, 24000, 36000, 48000, 54000)
_cache = {}


def signal_softs(o):
    """uint8 [n, 48]: the de-interleaved soft values of real SIGNAL symbols at all eight rates (noisy captures through the oracle's chain), random values over the
    demapper's output alphabet 0 .. 7, and the tie patterns: all equal (every level), alternating"""
    if "softs" not in _cache:
        rng = np.random.default_rng(20261201); out = []
        for i, rate in enumerate(RATES):
            mp = rng.integers(0, 256, 30 + 17 * i).astype(np.uint8).tobytes()
            x = o.tx_capture(mp, rate, seed=0x5D, lead=200, tail=200).astype(np.int32)
            x = np.clip(x + np.rint(rng.normal(0, 400, x.shape)).astype(np.int32), -32768, 32767).astype(np.int16)
            rows, tr = o.rx_capture(x, 40, trace=True)
            assert len(rows) == 1 and rows[0]["rate_kbps"] == rate
            out.append(o.deinterleave(1, o.demap(1, tr["tracked"][0])))
        out += list(rng.integers(0, 8, (64, 48)).astype(np.uint8))
        out += [np.full(48, v, np.uint8) for v in range(8)]
        out += [np.tile(np.array(p, np.uint8), 24) for p in ((0, 7), (7, 0), (3, 4), (4, 3))]
        _cache["softs"] = np.stack(out).astype(np.uint8)
    return _cache["softs"]


def signal_words():
    """uint32: all 131072 words with the reserved bits 0xFC0010 clear, then 4096 seeded words with one of them set"""
    if "words" not in _cache:
        k = np.arange(1 << 17, dtype=np.uint32)
        clear = (k & 0xF) | ((k >> 4) << 5)                                       # bits 0-3, 5-17
        rng = np.random.default_rng(20261202)
        w = rng.integers(0, 1 << 24, 4096).astype(np.uint32)
        bit = np.array([4, 18, 19, 20, 21, 22, 23], np.uint32)[rng.integers(0, 7, 4096)]
        _cache["words"] = np.concatenate([clear, w | (np.uint32(1) << bit)])
    return _cache["words"]


def x20(cap, rate_mhz=40):
    """a capture at the 20 MHz rate: TDownSample2 keeps the even samples"""
    return np.ascontiguousarray(cap[::2] if rate_mhz == 40 else cap)


EVENT_KEYS = ("start_sample", "end_sample", "error_code", "rate_kbps", "length", "nsym", "crc32", "cfo_est", "mpdu")


def composition_captures(o, rate_mhz=40):
    """the captures the composition is held on: the composite stream, every 37th capture of lead_sweep, every 29th of gap_sweep, every 11th of sts_fragments"""
    fam = sc.families(o)
    caps = fam["composite_stream"] + fam["lead_sweep"][::37] + fam["gap_sweep"][::29] + fam["sts_fragments"][::11]
    return [c if rate_mhz == 40 else np.ascontiguousarray(c[::2]) for c in caps]


def same_events(got, want):
    """-> None, or where the composition's events differ from rows with the handle's fields"""
    if len(got) != len(want):
        return "%d events, not %d" % (len(got), len(want))
    for i, (g, w) in enumerate(zip(got, want)):
        for k in EVENT_KEYS:
            if g[k] != w[k]:
                return "event %d, %s: %r, not %r" % (i, k, g[k] if k != "mpdu" else g[k][:16].hex(), w[k] if k != "mpdu" else w[k][:16].hex())
    return None


def sense_streams(o, model):
    """-> list of (raw samples int16 [4 n, 2] at the 20 MHz rate, n <= 2048 bursts; entering sora_cs11a_state int32 [48]): the families' captures with the
    constructed record, rails, thresholds, and records that enter mid-lock, with auto_count 1 .. 3 and with a time-out standing (the tests run all of them under
    both flags)"""
    if "streams" in _cache:
        return _cache["streams"]
    fam = sc.families(o); rng = np.random.default_rng(20261203)
    fresh = capi.cs11a_states(1)[0]
    out = []
    picks = (("dc_steps", 23), ("sts_fragments", 11), ("blip_gap_frame", 25), ("lead_sweep", 19), ("gap_sweep", 13), ("loud_noise", 1), ("many_frames", 1))
    for name, stride in picks:
        for cap in fam[name][::stride]:
            x = x20(cap)[:8192]
            out.append((x[:len(x) // 4 * 4], fresh.copy()))
    comp = x20(fam["composite_stream"][0])
    # rails: all +32767, all -32768, alternating; thresholds 0, 10^6, 2^31 - 1
    for thr in (0, 1000 * 1000, 0x7FFFFFFF):
        s = fresh.copy(); s[2] = thr
        for v in ((32767, 32767), (-32768, -32768)):
            out.append((np.tile(np.array(v, np.int16), (1024, 1)), s.copy()))
        alt = np.empty((1024, 2), np.int16); alt[0::2] = 32767; alt[1::2] = -32768
        out.append((alt, s.copy()))
        alt4 = np.empty((1024, 2), np.int16); alt4[:] = 32767; alt4[(np.arange(1024) // 4) % 2 == 1] = -32768
        out.append((alt4, s.copy()))
        out.append((comp[4000:9000 // 4 * 4], s.copy()))
        out.append((sc.frame(o)[::2].copy()[:960 // 2 // 4 * 4], s.copy()))
    # records picked up along the composite stream and a loud-noise capture, one burst at a time: mid-lock, auto_count 1 .. 3, a time-out standing
    want = {"lock": 12, "auto1": 6, "auto2": 6, "auto3": 6, "timeout": 12}
    for src in [comp, x20(fam["loud_noise"][20]), x20(fam["loud_noise"][33])] + [x20(c) for c in fam["sts_fragments"][::37] + fam["blip_gap_frame"][::97]]:
        s = fresh.copy(); b = 0; nb = len(src) // 4
        while b < nb and any(want.values()):
            s, u = model.carrier_sense(src[4 * b:4 * b + 4], s, 0)
            b += 1
            if s[0] == 1:
                capi.cca11a_reset(s.reshape(1, -1)); continue
            kind = "lock" if s[5] == 1 else "auto%d" % s[6] if 1 <= s[6] <= 3 else "timeout" if np.uint32(s[1]) == capi.E_CS_TIMEOUT else None
            if kind and want[kind] and (kind.startswith("auto") or rng.integers(0, 3) == 0):
                want[kind] -= 1
                out.append((src[4 * b:4 * min(nb, b + 600)], s.copy()))
            if np.uint32(s[1]) == capi.E_CS_TIMEOUT and b % 7 == 0:
                capi.cca11a_reset(s.reshape(1, -1))
    assert not any(want.values()), want
    _cache["streams"] = out
    return out
