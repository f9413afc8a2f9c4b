"""The 802.11b modulation graph's stage entry points (sora_amd/csrc/k_mod11b.hip) against the HBM roofline, and the chain composed of them against the fused
transmitter, on 4096 frames x 1500-byte MPDUs (with the FCS) at each of the four rates.

Per-stage rows, per rate: ppdu over the 4096 frames; sc741 and the rate's spreader over 4096 streams of the frame's 1524 PPDU bytes; pulse_shape over 4096 streams of
the chips those bytes spread to, with Flush; and, in the SAME run, sora_hip_pack16to8 over the shaper's samples as the yardstick: a stateless move of 16-byte words,
what a streaming kernel reaches on this device.  Distinct buffer sets in rotation so that consecutive launches share no line -- as many as bring the bytes in play past
600 MB (the Infinity Cache holds 256 MiB), at most 16; a row whose sets stay below that says so (`past_cache: false`).  Timed with device events after a warm-up of
every set; a probe of --reps calls sizes the timed window to about 100 ms.  A row gives the time per call, the algorithmic bytes (input + output, from the shapes),
GB/s, the fraction of benchlib.common.HBM_PEAK and that fraction over pack16to8's.

Chain row, per rate: Mod11bStages.run() (every intermediate through HBM) against sora_hip_tx11b on the same batch, in the same run, the two alternated block by
block; the ratio is reported, it is not a gate.
usage: python tools/bench_mod11b_stages.py [--nframes N] [--reps R] [--out profiles/mod11b_stages.json]   -> one JSON line per row, the whole record in the file"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SPREAD = {1000: ("dbpsk_spread", "sora_hip_dbpsk_spread11b", 88), 2000: ("dqpsk_spread", "sora_hip_dqpsk_spread11b", 44),
          5500: ("cck5_encode", "sora_hip_cck5_encode11b", 16), 11000: ("cck11_encode", "sora_hip_cck11_encode11b", 8)}


def bench_stages(torch, dev, rate, nframes, mpdu_len, reps, window_ms=100.0):
    from benchlib.common import HBM_PEAK
    from sora_amd import capi
    L = capi.load()
    P = capi._dev_ptr
    st = capi._stream_ptr(None)
    g = torch.Generator(device=dev); g.manual_seed(11)
    label, entry, cpb = SPREAD[rate]
    nb = 24 + mpdu_len + 4                                                       # PPDU bytes of a frame
    nchips = nb * cpb
    rows = {}

    def sets(nbytes):
        return int(min(16, max(2, -(-600e6 // nbytes))))

    def timed(label, make, nbytes, units):
        k = sets(nbytes)
        fns = [make() for _ in range(k)]
        for f in fns:
            assert f() == 0, (label, L.sora_hip_last_error())
        def window(n):
            e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(); e0.record()
            for i in range(n):
                fns[i % k]()
            e1.record(); torch.cuda.synchronize()
            return e0.elapsed_time(e1) / n
        n = int(min(8000, max(reps, window_ms / max(window(reps), 1e-4))))        # a short probe sizes the timed window
        ms = window(n)
        rows[label] = {"units": units, "ms_per_call": round(ms, 4), "calls_timed": n, "algorithmic_bytes": int(nbytes), "gb_s": round(nbytes / ms / 1e6, 1),
                       "hbm_peak_gb_s": HBM_PEAK / 1e9, "frac_hbm": round(nbytes / (ms * 1e-3) / HBM_PEAK, 4), "buffer_sets": k, "bytes_in_play": int(nbytes) * k,
                       "past_cache": bool(nbytes * k >= 512e6)}
        del fns
        torch.cuda.empty_cache()

    u8 = lambda *shape: torch.randint(0, 256, shape, dtype=torch.uint8, device=dev, generator=g)
    e = lambda dtype, *shape: torch.empty(shape, dtype=dtype, device=dev)
    ar = lambda step: (torch.arange(nframes, device=dev, dtype=torch.int64) * step).to(torch.int32).contiguous()    # (offsets: unsigned 32-bit words)
    full = lambda v: torch.full((nframes,), v, dtype=torch.int32, device=dev)
    stride = (mpdu_len + 3) // 4 * 4

    def mk_ppdu():
        a, b = u8(nframes * stride), e(torch.uint8, nframes * nb)
        off, ln, rt, kd, of = ar(stride), full(mpdu_len), full(rate), torch.zeros(nframes, dtype=torch.uint8, device=dev), ar(nb)
        return lambda: L.sora_hip_ppdu11b(P(a), P(off), P(ln), P(rt), P(kd), P(b), P(of), nframes, st)

    def mk_sc741():
        a, b, reg = u8(nframes * nb), e(torch.uint8, nframes * nb), full(0x6C)
        f, n = ar(nb), full(nb)
        return lambda: L.sora_hip_sc741_11b(P(a), P(f), P(n), P(f), P(reg), P(b), nframes, nb, st)

    def mk_spread():
        a, b, state = u8(nframes * nb), e(torch.int8, nframes * nchips, 2), torch.zeros((nframes, 4), dtype=torch.int32, device=dev)
        f, n, of = ar(nb), full(nb), ar(nchips)
        return lambda: getattr(L, entry)(P(a), P(f), P(n), P(of), P(state), P(b), nframes, nb, st)

    def mk_shape():
        a = torch.randint(-1, 2, (nframes * nchips, 2), dtype=torch.int8, device=dev, generator=g)
        b, state = e(torch.int16, nframes * 4 * (nchips + 6), 2), torch.zeros((nframes, 16), dtype=torch.int32, device=dev)
        f, n, of, fl = ar(nchips), full(nchips), ar(4 * (nchips + 6)), torch.ones(nframes, dtype=torch.uint8, device=dev)
        return lambda: L.sora_hip_pulse_shape11b(P(a), P(f), P(n), P(of), P(fl), P(state), P(b), nframes, nchips, st)

    nsamp = nframes * 4 * (nchips + 6)

    def mk_pack():
        a = torch.randint(-200, 200, (nsamp, 2), dtype=torch.int16, device=dev, generator=g)
        b = e(torch.int8, nsamp, 2)
        return lambda: L.sora_hip_pack16to8(P(a), P(b), nsamp, st)

    timed("ppdu", mk_ppdu, nframes * (mpdu_len + nb), nframes)
    timed("sc741", mk_sc741, nframes * 2 * nb, nframes * nb)
    timed(label, mk_spread, nframes * (nb + 2 * nchips), nframes * nb)
    timed("pulse_shape", mk_shape, nframes * (2 * nchips + 16 * (nchips + 5)), nframes * nchips)
    timed("pack16to8_yardstick", mk_pack, nsamp * 6, nsamp)
    for k, r in rows.items():
        r["frac_hbm_over_pack16to8"] = round(r["frac_hbm"] / rows["pack16to8_yardstick"]["frac_hbm"], 3)
        print(json.dumps({"row": k, "rate_kbps": rate, **r}), flush=True)
    return {"ppdu_bytes_per_frame": nb, "chips_per_frame": nchips, "rows": rows}


def bench_chain(torch, sora_amd, dev, rate, nframes, mpdu_len, reps=10, blocks=5):
    from benchlib.common import HBM_PEAK
    from sora_amd import capi
    L = capi.load()
    P = capi._dev_ptr
    rng = np.random.default_rng(0x5EED)
    mpdus = [bytes(rng.integers(0, 256, mpdu_len).astype(np.uint8)) for _ in range(64)] * (nframes // 64)
    plan = sora_amd.Mod11bStages(mpdus, [rate] * nframes)
    per = plan.offsets[1] - plan.offsets[0]
    stride = (mpdu_len + 3) // 4 * 4
    blob = np.zeros(nframes * stride, np.uint8)
    for f, m in enumerate(mpdus):
        blob[f * stride:f * stride + mpdu_len] = np.frombuffer(m, np.uint8)
    blob = torch.from_numpy(blob).to(dev)
    moff = torch.arange(nframes, dtype=torch.int32, device=dev) * stride
    lens = torch.full((nframes,), mpdu_len, dtype=torch.int32, device=dev); rates = torch.full((nframes,), rate, dtype=torch.int32, device=dev)
    ooff = torch.arange(nframes, dtype=torch.int64, device=dev) * per
    w = torch.zeros((per * nframes, 2), dtype=torch.int8, device=dev)
    fused = lambda: L.sora_hip_tx11b(P(blob), P(moff), P(lens), P(rates), None, None, nframes, P(w), P(ooff), capi._stream_ptr(None))
    assert fused() == 0, L.sora_hip_last_error()
    got = plan.run(); torch.cuda.synchronize()
    equal = bool(torch.equal(got, w))
    forms = {"tx11b_fused": (fused, []), "chain_of_stages": (plan.run, [])}
    for _ in range(blocks):
        for fn, ms in forms.values():
            e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record(); torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1) / reps)
    nsamp = per * nframes
    alg = nframes * mpdu_len + 2 * nsamp
    out = {"workload": "%d frames x %d-byte MPDU (+FCS) at %d kbps -> COMPLEX8 @44 MHz (%d samples)" % (nframes, mpdu_len, rate, nsamp),
           "chain_equals_fused": equal, "reps_per_block": reps, "blocks": blocks}
    for k, (_, ms) in forms.items():
        m = float(np.median(ms))
        out[k] = {"ms": round(m, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4), "msamples_per_s": round(nsamp / m / 1e3, 1),
                  "frac_hbm_of_the_frames_own_bytes": round(alg / (m * 1e-3) / HBM_PEAK, 4)}
    out["chain_over_fused"] = round(out["chain_of_stages"]["ms"] / out["tx11b_fused"]["ms"], 2)
    print(json.dumps({"row": "chain", "rate_kbps": rate, **out}), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nframes", type=int, default=4096)
    ap.add_argument("--mpdu-len", type=int, default=1496, help="bytes without the FCS: 1500 with it")
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mod11b_stages.json"))
    a = ap.parse_args()
    import torch
    import sora_amd
    if not torch.cuda.is_available():
        sys.exit("bench_mod11b_stages: no GPU -- nothing is measured without one")
    dev = torch.device("cuda", 0)
    rec = {"tool": "tools/bench_mod11b_stages.py", "device": torch.cuda.get_device_name(0), "nframes": a.nframes, "mpdu_len": a.mpdu_len, "reps": a.reps, "rates": {}}
    ok = True
    for rate in (1000, 2000, 5500, 11000):
        r = {"stages": bench_stages(torch, dev, rate, a.nframes, a.mpdu_len, a.reps)}
        torch.cuda.empty_cache()
        r["chain"] = bench_chain(torch, sora_amd, dev, rate, a.nframes, a.mpdu_len)
        torch.cuda.empty_cache()
        ok = ok and r["chain"]["chain_equals_fused"]
        rec["rates"][str(rate)] = r
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
