"""The stage entry points of the 40 MHz HT receiver (sora_amd/csrc/k_ht40_stages.hip) on one GPU, by the method of tools/bench_11a_rx_stages.py: 8192 symbols (or
frames / streams) per call, two buffer sets in rotation, device events after a warm-up.  Nothing here is a gate.

  every stage   microseconds per call and the share of benchlib.common.HBM_PEAK its algorithmic bytes (input + output, tables not counted) make, beside sora_hip_fft128
                on 8192 symbols IN THE SAME RUN
  composition   sora_amd.rx_ht40_by_stages (host wall clock: it builds tables on the host and reads theta back every symbol) against RxHt40.process_dev + wait on the
                same frames, every row compared
usage: python tools/bench_ht40_stages.py [--n N] [--frames F] [--reps R] [--out profiles/ht40_stages.json]   -> one JSON line per row, the record in the file"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def bench_stages(torch, dev, n, reps, nsets=2):
    from benchlib.common import HBM_PEAK
    from sora_amd import capi
    L = capi.load(); P = capi._dev_ptr; st = capi._stream_ptr(None)
    g = torch.Generator(device=dev); g.manual_seed(40)
    rows = {}

    def timed(label, fns, nbytes, unit="symbols"):
        for f in fns:
            assert f() == 0, (label, L.sora_hip_last_error())
        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(); e0.record()
        for i in range(reps):
            fns[i % len(fns)]()
        e1.record(); torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / reps
        rows[label] = {unit: n, "us": round(1e3 * ms, 1), "algorithmic_bytes": int(nbytes), "gb_s": round(nbytes / ms / 1e6, 1), "hbm_peak_gb_s": HBM_PEAK / 1e9,
                       "frac_hbm": round(nbytes / (ms * 1e-3) / HBM_PEAK, 4), "buffer_sets": len(fns)}
        print(json.dumps({"row": label, **rows[label]}), flush=True)

    c16 = lambda count, amp=9000: torch.randint(-amp, amp, (count, 2), dtype=torch.int16, device=dev, generator=g)
    ar = torch.arange(n, device=dev, dtype=torch.int64)
    tab = lambda per: (ar * per).to(torch.int32).contiguous()
    full = lambda v: torch.full((n,), v, dtype=torch.int32, device=dev)
    # ---- fft128, the yardstick: 8192 symbols in, 8192 out
    x = [c16(n * 128) for _ in range(nsets)]; y = torch.empty_like(x[0]); y1 = torch.empty_like(x[0])
    timed("fft128", [(lambda a=a: L.sora_hip_fft128(P(a), P(y), n, st)) for a in x], n * 128 * 4 * 2)
    # ---- mimo_comp_ht40: two chains in, two streams out, the weights of 64 frames
    w = c16(64 * 512, 3000); fi = (ar % 64).to(torch.int32).contiguous(); x2 = [c16(n * 128) for _ in range(nsets)]
    timed("mimo_comp_ht40", [(lambda a=a, b=b: L.sora_hip_mimo_comp_ht40(P(w), P(fi), P(a), P(b), P(y), P(y1), n, st)) for a, b in zip(x, x2)], n * 128 * 4 * 4)
    # ---- pilot_track_ht40: the symbols as frames of 64, and as frames of one (the composition's shape)
    state = torch.zeros((n, 24), dtype=torch.int16, device=dev); th = torch.zeros(n, dtype=torch.int16, device=dev)
    f64 = (torch.arange(n // 64, device=dev) * 64).to(torch.int32).contiguous(); n64 = torch.full((n // 64,), 64, dtype=torch.int32, device=dev)
    timed("pilot_track_ht40 (%d frames x 64 symbols)" % (n // 64), [(lambda a=a, b=b: L.sora_hip_pilot_track_ht40(P(a), P(b), P(f64), P(n64), P(state), P(th), n // 64, st)) for a, b in zip(x, x2)],
          n * 12 * 4 + n * 2)
    f1, n1 = tab(1), full(1)
    timed("pilot_track_ht40 (%d frames x 1 symbol)" % n, [(lambda a=a, b=b: L.sora_hip_pilot_track_ht40(P(a), P(b), P(f1), P(n1), P(state), P(th), n, st)) for a, b in zip(x, x2)],
          n * 12 * 4 + n * 2 + n * 32)
    del x2, y1
    # ---- demap_ht40, deinterleave_ht40, stream_join_ht40 per modulation
    for nb in (1, 2, 4, 6):
        soft = [torch.empty((n, 108 * nb), dtype=torch.uint8, device=dev) for _ in range(nsets)]
        timed("demap_ht40 n_bpsc %d" % nb, [(lambda a=a, s=s: L.sora_hip_demap_ht40(P(a), P(s), nb, n, st)) for a, s in zip(x, soft)], n * (128 * 4 + 108 * nb))
        de = torch.empty_like(soft[0])
        timed("deinterleave_ht40 n_bpsc %d" % nb, [(lambda s=s: L.sora_hip_deinterleave_ht40(P(s), P(de), nb, 1, n, st)) for s in soft], n * 108 * nb * 2)
        jn = torch.empty((n, 216 * nb), dtype=torch.uint8, device=dev)
        timed("stream_join_ht40 n_bpsc %d" % nb, [(lambda s=s: L.sora_hip_stream_join_ht40(P(s), P(de), P(jn), nb, n, st)) for s in soft], n * 108 * nb * 4)
        del soft, de, jn
    del y
    # ---- data_symbol_ht40: 8192 symbols as 512 frames of 16
    nf, per = n // 16, 16
    raw = [c16(n * 160) for _ in range(nsets)]; raw1 = c16(n * 160); o0 = torch.empty((n * 128, 2), dtype=torch.int16, device=dev); o1 = torch.empty_like(o0)
    ff = (torch.arange(nf, device=dev) * (per * 160)).to(torch.int32).contiguous(); fn = torch.full((nf,), per, dtype=torch.int32, device=dev)
    fo = (torch.arange(nf, device=dev) * per).to(torch.int32).contiguous()
    timed("data_symbol_ht40", [(lambda a=a: L.sora_hip_data_symbol_ht40(P(a), P(raw1), P(ff), P(fn), P(fo), P(o0), P(o1), nf, per, st)) for a in raw], n * (160 + 128) * 4 * 2)
    # ---- downsample_ht40: 8192 x 160 raw samples of both chains as 512 streams
    kept = n * 80 // nf
    df = (torch.arange(nf, device=dev) * (2 * kept)).to(torch.int32).contiguous(); dn = torch.full((nf,), kept, dtype=torch.int32, device=dev)
    do = (torch.arange(nf, device=dev) * kept).to(torch.int32).contiguous(); dm0 = torch.zeros(nf, dtype=torch.int32, device=dev)
    timed("downsample_ht40", [(lambda a=a: L.sora_hip_downsample_ht40(P(a), P(raw1), P(df), P(dn), P(dm0), P(do), P(o0), P(o1), nf, kept, st)) for a in raw],
          n * 160 * 4 * 2 + n * 80 * 4 * 2)
    rows["downsample_ht40"]["note"] = "algorithmic bytes count every raw sample: the odd ones share the even ones' 16-byte loads"
    del raw, raw1, o0, o1
    # ---- mimo_est_ht40, noise_var_ht40: 8192 frames
    l = [c16(n * 256, 3000) for _ in range(nsets)]; l1 = c16(n * 256, 3000); hh = torch.empty((n, 4, 128, 2), dtype=torch.int16, device=dev); ww = torch.empty_like(hh)
    nv = torch.full((n,), 3000.0, dtype=torch.float32, device=dev)
    timed("mimo_est_ht40 (MMSE)", [(lambda a=a: L.sora_hip_mimo_est_ht40(P(a), P(l1), P(nv), P(hh), P(ww), n, st)) for a in l], n * (256 * 4 * 2 + 512 * 4 * 2 + 4), "frames")
    timed("mimo_est_ht40 (zero forcing)", [(lambda a=a: L.sora_hip_mimo_est_ht40(P(a), P(l1), None, P(hh), P(ww), n, st)) for a in l], n * (256 * 4 * 2 + 512 * 4 * 2), "frames")
    S = torch.zeros(n, dtype=torch.int64, device=dev); nvo = torch.zeros(n, dtype=torch.float32, device=dev)
    timed("noise_var_ht40", [(lambda a=a: L.sora_hip_noise_var_ht40(P(a), P(l1), P(S), P(nvo), n, st)) for a in l], n * (128 * 4 * 2 + 12), "frames")
    return rows


def bench_chain(torch, sora, dev, nframes, reps=3):
    import time
    from oracle import py_ht40 as m
    from test_gpu_ht40 import make_frames
    rng = np.random.default_rng(41)
    specs = [((1, 0), (2, 0), (2, 2), (4, 0), (4, 2), (6, 1), (6, 2))[i % 7] + (int(rng.integers(40, 400)),) * 2 for i in range(nframes)]
    iq, descs, _ = make_frames(rng, specs, sigma=8.0)
    d0, d1 = torch.from_numpy(iq[0].copy()).to(dev), torch.from_numpy(iq[1].copy()).to(dev)
    nsoft = sum(2 * (sora.ht40_symbols(d[3], d[4], d[1], d[2]) * 108 * d[1] + 64) for d in descs)
    rx = sora.RxHt40(len(descs), nsoft)
    rows = rx.results(ticket=rx.process_dev(d0, d1, descs))
    t = []
    for _ in range(reps):
        torch.cuda.synchronize(); t0 = time.perf_counter(); r = sora.rx_ht40_by_stages(d0, d1, descs); t.append(time.perf_counter() - t0)
    equal = len(rows) == len(r["rows"]) and all((a["error_code"], a["length"], a["crc32"], a["mpdu"]) == (b["error_code"], b["length"], b["crc32"], b["mpdu"])
                                                 for a, b in zip(r["rows"], rows))
    h = []
    for _ in range(reps + 2):
        torch.cuda.synchronize(); t0 = time.perf_counter(); tk = rx.process_dev(d0, d1, descs); rx.wait(tk); h.append(time.perf_counter() - t0)
    rx.close()
    out = {"workload": "%d described frames, MCS 8..14 in turn, PSDUs of 40..400 bytes, sigma 8" % nframes, "rows": len(rows),
           "data_symbols_of_the_longest_frame": max(x["nsym"] for x in rows), "every_row_equals_the_handles": bool(equal),
           "by_stages_ms": round(1e3 * float(np.median(t)), 1), "handle_ms": round(1e3 * float(np.median(h[2:])), 2)}
    out["by_stages_over_handle"] = round(out["by_stages_ms"] / out["handle_ms"], 1)
    print(json.dumps({"row": "chain", **out}), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ht40_stages.json"))
    a = ap.parse_args()
    import torch
    dev = torch.device("cuda", 0)
    git = lambda *c: subprocess.run(("git",) + c, cwd=ROOT, capture_output=True, text=True).stdout.strip() or None
    rec = {"tool": "tools/bench_ht40_stages.py", "parent_commit": "01e3bce", "head_when_measured": git("rev-parse", "--short", "HEAD"),
           "tree_differs_from_head": bool(git("status", "--porcelain")) if git("rev-parse", "--short", "HEAD") else None, "device": torch.cuda.get_device_name(0), "n": a.n, "reps": a.reps,
           "stages": bench_stages(torch, dev, a.n, a.reps)}
    torch.cuda.empty_cache()
    import sora_amd
    rec["chain"] = bench_chain(torch, sora_amd, dev, a.frames)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")
    return 0 if rec["chain"]["every_row_equals_the_handles"] else 1


if __name__ == "__main__":
    sys.exit(main())
