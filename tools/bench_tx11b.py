"""The 802.11b transmitter (sora_hip_tx11b): one 1500-byte MPDU (1496 bytes + FCS) per frame, 4096 frames per call at 11 and at
5.5 Mbps and 1024 frames at 1 Mbps (about 1.1 GB of output: byte offsets past 2^31), timed with hipEvents over back-to-back calls.
Reports ms per call, output Msamples/s and the fraction of the HBM peak counted with the algorithmic bytes (MPDU bytes in, 2 bytes
per COMPLEX8 sample out).  Every frame of a call carries the same MPDU from the same start phase, so the last frame must equal the
first.  Where oracle/_ref is built, also the compiled reference modulator (ref_tx11b) on one core, per frame.
usage: python tools/bench_tx11b.py [reps]   -> one JSON line per row"""
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12                     # B/s, benchlib/common.py
MPDU = 1496                           # without FCS
ROWS = [(11000, 4096), (5500, 4096), (1000, 1024)]


def bench_gpu(torch, sora_amd, rate, nframes, reps):
    from sora_amd import capi
    per = sora_amd.tx11b_samples(MPDU, rate)
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(rate)
    blob = torch.from_numpy(rng.integers(0, 256, MPDU).astype(np.uint8)).to(dev)
    moff = torch.zeros(nframes, dtype=torch.int32, device=dev)                  # every frame reads the one MPDU
    lens = torch.full((nframes,), MPDU, dtype=torch.int32, device=dev)
    rates = torch.full((nframes,), rate, dtype=torch.int32, device=dev)
    ooff = torch.arange(nframes, dtype=torch.int64, device=dev) * per
    out = torch.empty((nframes * per, 2), dtype=torch.int8, device=dev)
    L = capi.load()
    call = lambda: L.sora_hip_tx11b(capi._dev_ptr(blob), capi._dev_ptr(moff), capi._dev_ptr(lens), capi._dev_ptr(rates), None, None, nframes,
                                    capi._dev_ptr(out), capi._dev_ptr(ooff), capi._stream_ptr(None))
    for _ in range(3):
        assert call() == 0
    e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(); e0.record()
    for _ in range(reps):
        call()
    e1.record(); torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / reps
    same = bool(torch.equal(out[:per], out[(nframes - 1) * per:]))
    nsamp = per * nframes
    alg = nframes * MPDU + 2 * nsamp
    return {"row": "tx11b_gpu", "rate_kbps": rate, "workload": "%d frames x %d-byte MPDU (+FCS) at %g Mbps -> COMPLEX8 @44 MHz (%d samples)"
            % (nframes, MPDU, rate / 1000, nsamp), "ms": round(ms, 4), "msamples_per_s": round(nsamp / ms / 1e3, 1), "algorithmic_bytes": alg,
            "achieved_gb_s": round(alg / ms / 1e6, 1), "hbm_peak_gb_s": HBM_PEAK / 1e9, "frac_hbm": round(alg / (ms * 1e-3) / HBM_PEAK, 4),
            "last_frame_equals_first": same, "reps": reps}


def bench_reference(rate, nframes):
    from oracle.pyoracle import ReferenceGraph
    g = ReferenceGraph()
    if not g.available():
        return None
    import sora_amd
    rng = np.random.default_rng(rate)
    mp = rng.integers(0, 256, MPDU).astype(np.uint8)
    cap = sora_amd.tx11b_samples(MPDU, rate) + 64                              # TModSink does not bound its writes: room for the whole frame
    o = np.zeros((cap, 2), np.int8)
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    call = lambda: g.L.ref_tx11b(P(mp), MPDU, rate, P(o), cap)                  # the graph straight, into a buffer allocated once
    nsamp = call()
    assert nsamp == cap - 64
    n = 16
    t0 = time.perf_counter()
    for _ in range(n):
        call()
    dt = (time.perf_counter() - t0) / n                                        # per frame, one core
    return {"row": "tx11b_reference_one_core", "rate_kbps": rate, "ms_per_frame": round(dt * 1e3, 4),
            "ms_for_%d_frames" % nframes: round(dt * 1e3 * nframes, 1), "msamples_per_s": round(nsamp / dt / 1e6, 2), "frames_timed": n}


def main():
    import torch
    import sora_amd
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    ok = True
    for rate, nframes in ROWS:
        r = bench_gpu(torch, sora_amd, rate, nframes, reps)
        ok &= r["last_frame_equals_first"]
        print(json.dumps(r), flush=True)
    for rate, nframes in ROWS:
        r = bench_reference(rate, nframes)
        if r:
            print(json.dumps(r), flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
