"""The 802.11a transmitter at 40 MHz (sora_hip_tx11a) and at 44 MHz (sora_hip_tx11a44) side by side: 4096 frames of one 1500-byte MPDU
(1496 bytes + FCS) per call, at 54 and at 6 Mbps.  The two calls are alternated in one process -- a block of back-to-back 40 MHz calls,
a block of 44 MHz calls, and again -- each block timed with hipEvents after warm-up; a row gives the median block, the spread of the
blocks, output Msamples/s and the fraction of the HBM peak counted with the algorithmic bytes (MPDU bytes in, 2 bytes per COMPLEX8
sample out).  Every frame of a call carries the same MPDU and seed, so the last frame must equal the first.
usage: python tools/bench_tx11a44.py [reps per block] [blocks]   -> one JSON line per row"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12                     # B/s, benchlib/common.py
MPDU = 1496                           # without FCS
NFRAMES = 4096
RATES = (54000, 6000)


def bench_rate(torch, sora_amd, rate, reps, blocks):
    from sora_amd import capi
    L = capi.load()
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(rate)
    blob = torch.from_numpy(rng.integers(0, 256, MPDU).astype(np.uint8)).to(dev)
    moff = torch.zeros(NFRAMES, dtype=torch.int32, device=dev)                  # every frame reads the one MPDU
    lens = torch.full((NFRAMES,), MPDU, dtype=torch.int32, device=dev)
    rates = torch.full((NFRAMES,), rate, dtype=torch.int32, device=dev)
    seeds = torch.full((NFRAMES,), 0x5B, dtype=torch.uint8, device=dev)
    forms = {}
    for mhz, fn in ((40, L.sora_hip_tx11a), (44, L.sora_hip_tx11a44)):
        per = sora_amd.tx11a_samples(MPDU, rate, sample_rate_mhz=mhz)
        ooff = torch.arange(NFRAMES, dtype=torch.int64, device=dev) * per
        out = torch.empty((NFRAMES * per, 2), dtype=torch.int8, device=dev)
        call = (lambda fn=fn, out=out, ooff=ooff: fn(capi._dev_ptr(blob), capi._dev_ptr(moff), capi._dev_ptr(lens), capi._dev_ptr(rates), capi._dev_ptr(seeds),
                                                      NFRAMES, capi._dev_ptr(out), capi._dev_ptr(ooff), capi._stream_ptr(None)))
        forms[mhz] = {"per": per, "out": out, "ooff": ooff, "call": call, "ms": []}
        for _ in range(3):
            assert call() == 0
    torch.cuda.synchronize()
    for _ in range(blocks):
        for mhz in (40, 44):
            F = forms[mhz]
            e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                F["call"]()
            e1.record(); torch.cuda.synchronize()
            F["ms"].append(e0.elapsed_time(e1) / reps)
    rows = []
    for mhz in (40, 44):
        F = forms[mhz]
        per, out = F["per"], F["out"]
        ms = float(np.median(F["ms"]))
        nsamp = per * NFRAMES
        alg = NFRAMES * MPDU + 2 * nsamp
        rows.append({"row": "tx11a_%d" % mhz, "rate_kbps": rate, "workload": "%d frames x %d-byte MPDU (+FCS) at %g Mbps -> COMPLEX8 @%d MHz (%d samples)"
                     % (NFRAMES, MPDU, rate / 1000, mhz, nsamp), "ms": round(ms, 4), "ms_min": round(min(F["ms"]), 4), "ms_max": round(max(F["ms"]), 4),
                     "msamples_per_s": round(nsamp / ms / 1e3, 1), "algorithmic_bytes": alg, "achieved_gb_s": round(alg / ms / 1e6, 1),
                     "hbm_peak_gb_s": HBM_PEAK / 1e9, "frac_hbm": round(alg / (ms * 1e-3) / HBM_PEAK, 4),
                     "last_frame_equals_first": bool(torch.equal(out[:per], out[(NFRAMES - 1) * per:])), "reps_per_block": reps, "blocks": blocks})
    rows[1]["ms_over_40mhz"] = round(rows[1]["ms"] / rows[0]["ms"], 3)
    return rows


def main():
    import torch
    import sora_amd
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    blocks = int(sys.argv[2]) if len(sys.argv) > 2 else 9
    ok = True
    for rate in RATES:
        for r in bench_rate(torch, sora_amd, rate, reps, blocks):
            ok &= r["last_frame_equals_first"]
            print(json.dumps(r), flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
