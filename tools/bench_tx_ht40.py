"""The 40 MHz HT 2x2 transmitter (sora_hip_tx_ht40): 4096 frames of two 1500-byte PSDUs (1496 bytes + FCS per stream) at MCS 14 and at
MCS 8 per call, timed with hipEvents over back-to-back calls.  Reports ms per call and the output bytes (2 chains x 4 bytes per sample)
over that time as a share of the HBM peak; beside them sora_hip_tx11n at MCS 14 on the same batch size from the same run, and the time
oracle/py_ht40.py::tx_frame (the float64 model every HT40 capture came from until now) takes for one such frame on the host.
Every GPU row runs in a process of its own under `timeout -k 10`; the first one that fails ends the run.
usage: python tools/bench_tx_ht40.py [frames] [reps]   -> one JSON line per row"""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12                     # B/s, benchlib/common.py
MPDU = 1496                           # without FCS, per stream
ROW_TIMEOUT_S = 240


def _time(torch, call, reps):
    for _ in range(3):
        assert call() == 0
    e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(); e0.record()
    for _ in range(reps):
        call()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def bench_ht40(mcs, nframes, reps):
    import torch
    import sora_amd
    from sora_amd import capi
    dev = torch.device("cuda")
    per = sora_amd.tx_ht40_samples(MPDU, mcs)
    lens = torch.full((nframes,), MPDU, dtype=torch.int32, device=dev)
    mcsv = torch.full((nframes,), mcs, dtype=torch.int32, device=dev)
    moff = torch.arange(2 * nframes, dtype=torch.int32, device=dev) * MPDU
    blob = torch.randint(0, 256, (2 * nframes * MPDU,), dtype=torch.uint8, device=dev)
    ooff = torch.arange(nframes, dtype=torch.int64, device=dev) * per
    out0 = torch.zeros((nframes * per, 2), dtype=torch.int16, device=dev); out1 = torch.zeros_like(out0)
    L = capi.load()
    call = lambda: L.sora_hip_tx_ht40(capi._dev_ptr(blob), capi._dev_ptr(moff), capi._dev_ptr(lens), capi._dev_ptr(mcsv), None, nframes,
                                      capi._dev_ptr(out0), capi._dev_ptr(out1), capi._dev_ptr(ooff), capi._stream_ptr(None))
    ms = _time(torch, call, reps)
    nsamp = per * nframes                                                       # per chain
    outb = 2 * 4 * nsamp
    return {"row": "tx_ht40_gpu", "mcs": mcs, "workload": "%d frames x 2 x %d-byte MPDU (+FCS) at MCS %d -> 2 x COMPLEX16 @40 MHz (%d samples per chain)"
            % (nframes, MPDU, mcs, nsamp), "ms": round(ms, 4), "data_symbols_per_frame": (per - 1600) // 160, "msamples_per_s_per_chain": round(nsamp / ms / 1e3, 1),
            "output_bytes": outb, "achieved_gb_s": round(outb / ms / 1e6, 1), "hbm_peak_gb_s": HBM_PEAK / 1e9, "frac_hbm": round(outb / (ms * 1e-3) / HBM_PEAK, 4), "reps": reps}


def bench_tx11n(mcs, nframes, reps):
    import torch
    import sora_amd
    from sora_amd import capi
    dev = torch.device("cuda")
    per = sora_amd.tx11n_samples(MPDU, mcs)
    lens = torch.full((nframes,), MPDU, dtype=torch.int32, device=dev)
    mcsv = torch.full((nframes,), mcs, dtype=torch.int32, device=dev)
    moff = torch.arange(nframes, dtype=torch.int32, device=dev) * MPDU
    blob = torch.randint(0, 256, (nframes * MPDU,), dtype=torch.uint8, device=dev)
    ooff = torch.arange(nframes, dtype=torch.int64, device=dev) * per
    out0 = torch.zeros((nframes * per, 2), dtype=torch.int16, device=dev); out1 = torch.zeros_like(out0)
    L = capi.load()
    call = lambda: L.sora_hip_tx11n(capi._dev_ptr(blob), capi._dev_ptr(moff), capi._dev_ptr(lens), capi._dev_ptr(mcsv), None, nframes,
                                    capi._dev_ptr(out0), capi._dev_ptr(out1), capi._dev_ptr(ooff), capi._stream_ptr(None))
    ms = _time(torch, call, reps)
    outb = 2 * 4 * per * nframes
    return {"row": "tx11n_gpu", "mcs": mcs, "workload": "%d frames x %d-byte MPDU (+FCS) at MCS %d, 20 MHz (%d samples per chain)" % (nframes, MPDU, mcs, per * nframes),
            "ms": round(ms, 4), "data_symbols_per_frame": (per - 1600) // 160, "output_bytes": outb, "frac_hbm": round(outb / (ms * 1e-3) / HBM_PEAK, 4), "reps": reps}


def bench_model(mcs):
    from oracle import py_ht40 as m
    rng = np.random.default_rng(mcs)
    ps = [m.add_fcs(rng.integers(0, 256, MPDU, dtype=np.uint8).tobytes()) for _ in range(2)]
    t0 = time.perf_counter()
    x, nsym, _ = m.tx_frame(ps, mcs)
    dt = time.perf_counter() - t0
    return {"row": "py_ht40_tx_frame_host", "mcs": mcs, "ms_per_frame": round(dt * 1e3, 1), "data_symbols_per_frame": nsym}


ROWS = {"ht40_mcs14": lambda n, r: bench_ht40(14, n, r), "ht40_mcs8": lambda n, r: bench_ht40(8, n, r), "tx11n_mcs14": lambda n, r: bench_tx11n(14, n, r)}


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--row":                            # one GPU row, in this process
        print(json.dumps(ROWS[sys.argv[2]](int(sys.argv[3]), int(sys.argv[4]))), flush=True)
        return 0
    nframes = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    for row in ROWS:
        rc = subprocess.run(["timeout", "-k", "10", str(ROW_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--row", row, str(nframes), str(reps)]).returncode
        if rc != 0:
            print(json.dumps({"row": row, "failed": rc}), flush=True)
            return 1
    for mcs in (14, 8):
        print(json.dumps(bench_model(mcs)), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
