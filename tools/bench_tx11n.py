"""The 802.11n 2x2 transmitter (sora_hip_tx11n): 4096 frames of a 1500-byte MPDU (1496 bytes + FCS) at MCS 10 and at MCS 14 per call,
timed with hipEvents over back-to-back calls.  Reports ms per call, output Msamples/s per chain and the fraction of the HBM peak
counted with the algorithmic bytes (MPDU bytes in, 2 chains x 4 bytes per sample out), as benchlib/stages.py:bench_tx counts the
802.11a transmitter.  Where oracle/_ref is built, also the compiled reference modulator (ref_tx11n) on one core, per frame.
usage: python tools/bench_tx11n.py [frames] [reps]   -> one JSON line per row"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12                     # B/s, benchlib/common.py
MPDU = 1496                           # without FCS


def bench_gpu(torch, sora_amd, mcs, nframes, reps):
    from sora_amd import capi
    rng = np.random.default_rng(mcs)
    mpdus = [bytes(rng.integers(0, 256, MPDU).astype(np.uint8)) for _ in range(64)] * (nframes // 64)
    out0, out1, off = sora_amd.tx11n(mpdus, [mcs] * nframes)                   # allocates the outputs; also the warm-up
    dev = out0.device
    per = off[1] - off[0]
    lens = torch.full((nframes,), MPDU, dtype=torch.int32, device=dev)
    mcsv = torch.full((nframes,), mcs, dtype=torch.int32, device=dev)
    moff = torch.arange(nframes, dtype=torch.int32, device=dev) * MPDU
    blob = torch.randint(0, 256, (nframes * MPDU,), dtype=torch.uint8, device=dev)
    ooff = torch.arange(nframes, dtype=torch.int64, device=dev) * per
    L = capi.load()
    call = lambda: L.sora_hip_tx11n(capi._dev_ptr(blob), capi._dev_ptr(moff), capi._dev_ptr(lens), capi._dev_ptr(mcsv), None, nframes,
                                    capi._dev_ptr(out0), capi._dev_ptr(out1), capi._dev_ptr(ooff), capi._stream_ptr(None))
    for _ in range(3):
        assert call() == 0
    e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(); e0.record()
    for _ in range(reps):
        call()
    e1.record(); torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / reps
    nsamp = per * nframes                                                       # per chain
    alg = nframes * MPDU + 2 * 4 * nsamp
    return {"row": "tx11n_gpu", "mcs": mcs, "workload": "%d frames x %d-byte MPDU (+FCS) at MCS %d -> 2 x COMPLEX16 @40 MHz (%d samples per chain)"
            % (nframes, MPDU, mcs, nsamp), "ms": round(ms, 4), "msamples_per_s_per_chain": round(nsamp / ms / 1e3, 1), "algorithmic_bytes": alg,
            "achieved_gb_s": round(alg / ms / 1e6, 1), "hbm_peak_gb_s": HBM_PEAK / 1e9, "frac_hbm": round(alg / (ms * 1e-3) / HBM_PEAK, 4), "reps": reps}


def bench_reference(mcs, nframes):
    from oracle.pyoracle import ReferenceGraph
    g = ReferenceGraph()
    if not g.available():
        return None
    import ctypes
    rng = np.random.default_rng(mcs)
    mp = rng.integers(0, 256, MPDU).astype(np.uint8)
    cap = 1 << 16
    o0 = np.zeros((cap, 2), np.int16); o1 = np.zeros((cap, 2), np.int16)
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    call = lambda: g.L.ref_tx11n(P(mp), MPDU, mcs, P(o0), P(o1), cap)          # the graphs straight, into buffers allocated once
    nsamp = call()
    assert nsamp > 0
    n = 64
    t0 = time.perf_counter()
    for _ in range(n):
        call()
    dt = (time.perf_counter() - t0) / n                                        # per frame, one core
    return {"row": "tx11n_reference_one_core", "mcs": mcs, "ms_per_frame": round(dt * 1e3, 4), "ms_for_%d_frames" % nframes: round(dt * 1e3 * nframes, 1),
            "msamples_per_s_per_chain": round(nsamp / dt / 1e6, 2), "frames_timed": n}


def main():
    import torch
    import sora_amd
    nframes = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    for mcs in (10, 14):
        print(json.dumps(bench_gpu(torch, sora_amd, mcs, nframes, reps)), flush=True)
    for mcs in (10, 14):
        r = bench_reference(mcs, nframes)
        if r:
            print(json.dumps(r), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
