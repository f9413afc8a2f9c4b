"""Capture families that walk the branches of 802.11a carrier sense (TDCRemoveEx -> TCCA11a -> TDCEstimator, cca.hpp:126-437, dc.hpp:92-166) which
frames behind a quiet lead never reach: a true carrier test between a time-out being raised and the end of its source call, a lock dropped on the
burst that updates the DC estimate, establish_sync that does not lock, more frames in a capture than k_scan has lanes to queue them in.  Used by
tests/test_scan_captures_cpu.py (the restatement against the compiled reference graph, and which branches the families reach) and
tests/test_gpu_scan_sense.py (k_scan against the restatement: rows, and the whole carrier-sense state at every resume point).

Everything is a 40 MHz raw capture of whole 28-sample source calls, generated from fixed seeds.  The frame is 20 bytes at 54 Mbps: 960 raw samples."""
import numpy as np

SIGMA = 30.0
DC_AMPLITUDES = (1000, 2000, 2850, 2900, 3000, 3200, 4000, 8000, 16000, 30000)      # a bare offset trips the carrier test from about 2800 on
FRAGMENT_LENGTHS = tuple(range(32, 421, 12))
_cache = {}


def frame(o, rate_kbps=54000, seed=1):
    """int16 [n, 2]: a 20-byte frame (16 bytes + FCS) at 40 MHz, no lead, no tail"""
    key = (rate_kbps, seed)
    if key not in _cache:
        mp = np.random.default_rng(1000 + seed).integers(0, 256, 16).astype(np.uint8).tobytes()
        _cache[key] = o.tx_capture(mp, rate_kbps, seed=1 + seed % 127, lead=0, tail=0)
    return _cache[key]


def _mix(n, parts, rng, sigma=SIGMA, offsets=()):
    """n raw samples (rounded up to whole source calls): parts = [(position, samples)], offsets = [(from, to, re, im)], white noise on top"""
    n = -(-n // 28) * 28
    x = np.zeros((n, 2), np.float64)
    for at, s in parts:
        x[at:at + len(s)] += s
    for a, b, re, im in offsets:
        x[a:b, 0] += re; x[a:b, 1] += im
    if sigma:
        x += rng.normal(0, sigma, x.shape)
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


def dc_steps(o):
    """an offset (A, -A / 2) switched on 600 .. 710 raw samples in, with and without a frame riding on it 3000 samples later"""
    rng = np.random.default_rng(20261101); f = frame(o); out = []
    for A in DC_AMPLITUDES:
        for lead in range(0, 112, 2):
            on = 600 + lead
            out.append(_mix(on + 2000, [], rng, offsets=[(on, None, A, -A // 2)]))
            out.append(_mix(on + 3000 + len(f) + 300, [(on + 3000, f)], rng, offsets=[(on, None, A, -A // 2)]))
    return out


def sts_fragments(o):
    """the preamble cut after n raw samples, then quiet; the lead over the eight burst phases of TDCEstimator's counter; also on a sub-threshold offset"""
    rng = np.random.default_rng(20261102); f = frame(o); out = []
    for off in ((0, 0), (700, -500)):
        for n in FRAGMENT_LENGTHS:
            for ph in range(8):
                lead = 280 + 8 * ph
                out.append(_mix(lead + n + 920, [(lead, f[:n])], rng, offsets=[(0, None) + off] if off != (0, 0) else ()))
    return out


def blip_gap_frame(o):
    """a fragment of the short training symbols, d raw samples of quiet, then a frame: an isolated true carrier test moves the phase of sense_count, so that
    a time-out is raised in the middle of a source call and the frame's first true tests fall in front of that call's end"""
    rng = np.random.default_rng(20261103); f = frame(o); out = []
    for n in (72, 88, 104):
        for d in range(60, 260, 2):
            for lead in (224, 230, 244, 258):
                at = lead + n + d
                out.append(_mix(at + len(f) + 200, [(lead, f[:n]), (at, f)], rng))
    return out


def lead_sweep(o):
    """one frame behind 0 .. 895 raw samples: 896 = 2 lcm(64, 14, 4) at the 20 MHz rate"""
    rng = np.random.default_rng(20261104); f = frame(o)
    return [_mix(lead + len(f) + 200, [(lead, f)], rng) for lead in range(896)]


def gap_sweep(o):
    """two frames, 0 .. 447 raw samples apart"""
    rng = np.random.default_rng(20261105); f = frame(o); g = frame(o, seed=2)
    return [_mix(300 + len(f) + gap + len(g) + 200, [(300, f), (300 + len(f) + gap, g)], rng) for gap in range(448)]


MANY_FRAMES = (16, 63, 64, 65, 70)


def many_frames(o):
    """captures of 16, 63, 64, 65 and 70 frames, 320 raw samples apart, the rates cycling 54 / 48 / 24 Mbps (all three code rates' job lists fill)"""
    rng = np.random.default_rng(20261106); out = []
    for nf in MANY_FRAMES:
        parts = []; at = 320
        for i in range(nf):
            s = frame(o, (54000, 48000, 24000)[i % 3], seed=3 + i % 7)
            parts.append((at, s)); at += len(s) + 320
        out.append(_mix(at, parts, rng))
    return out


def loud_noise(o):
    """150 source calls of white noise, sigma 300 .. 9000: carrier tests, locks that do not hold and time-outs at every phase"""
    rng = np.random.default_rng(20261107)
    return [_mix(28 * 150, [], rng, sigma=s) for s in (300, 500, 700, 1000, 1400, 2000, 2800, 4000, 5600, 7000, 8000, 9000) for _ in range(3)]


def composite_stream(o):
    """One stream of 18,200 raw samples (65 periods of 280, 325 source bursts of 56) that strings the families together: quiet; a DC step with a frame on it;
    four fragments; three frames 320 and 90 samples apart; 2800 samples of sigma = 3000; quiet."""
    rng = np.random.default_rng(20261108); f = frame(o); g = frame(o, seed=2); h = frame(o, 24000, seed=4)
    parts = [(4500, f)]
    # the three short fragments sit where the lock they cause is dropped again and a resume point follows before the time-out resets the brick: only
    # there does a record hold a stale high_count / peak_corr / peak_index (tests/test_scan_captures_cpu.py checks that both traces have such points)
    for at, n in ((6430, 88), (6900, 200), (7442, 72), (7918, 104)):
        parts.append((at, f[:n]))
    at = 8800
    for s, gap in ((f, 320), (g, 90), (h, 0)):
        parts.append((at, s)); at += len(s) + gap
    x = _mix(18200, parts, rng, offsets=[(1500, 6000, 3000, -1500)]).astype(np.int32)
    x[12400:15200] += np.rint(rng.normal(0, 3000, (2800, 2))).astype(np.int32)
    x = np.clip(x, -32768, 32767).astype(np.int16)
    assert len(x) == 18200
    return x


FAMILIES = (("dc_steps", dc_steps), ("sts_fragments", sts_fragments), ("blip_gap_frame", blip_gap_frame), ("lead_sweep", lead_sweep),
            ("gap_sweep", gap_sweep), ("many_frames", many_frames), ("loud_noise", loud_noise), ("composite_stream", lambda o: [composite_stream(o)]))


def families(o):
    """{name: [capture]}, generated once per process"""
    if "families" not in _cache:
        _cache["families"] = {name: fn(o) for name, fn in FAMILIES}
    return _cache["families"]
