"""The 802.11b receive graph's stage entry points (sora_amd/csrc/k_11b.hip) against the HBM roofline, the symbol-timing brick's scan share, and the composition of
the stages against the sora_rx11b_* handle.  Nothing here is a gate.

Per-stage rows, 8192 streams per call, two buffer sets in rotation, device events after a warm-up: the CCK decoders, the descrambler and the sink on one 11 Mbps x
1500-byte frame per stream (12 000 chips, 1500 bytes); despread, DBPSK demap and symbol timing on one 1 Mbps x 500-byte frame per stream (176 000 samples, 44 000 chips,
4000 symbols).  A row gives ms, the algorithmic bytes (input + output, from the shapes), GB/s and the fraction of benchlib.common.HBM_PEAK.

Scan share: sora_hip_symtiming11b of this library against the same entry of a tools variant built with SORA_DBG_SYMT_NO_SCAN (the kernel without thread 0's walk over
the energies; sora_amd.build.build_variant), on the same streams, and on ONE stream of 19 000 blocks, where nothing else hides the walk.

Composition row: sora_amd.rx11b_by_stages (host wall clock: it reads counts back between stages) against Rx11b.process_dev + wait on the same 8192 captures, one 11 Mbps x
1500-byte frame each behind 2000 samples of silence.
usage: python tools/bench_11b_stages.py [--streams N] [--reps R] [--out profiles/11b_stages.json]   -> one JSON line per row, the whole record in the file"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def bench_stages(torch, sora, dev, ns, reps, nsets=2):
    from benchlib.common import HBM_PEAK
    from sora_amd import build, capi
    L = capi.load()
    P = capi._dev_ptr
    st = capi._stream_ptr(None)
    g = torch.Generator(device=dev); g.manual_seed(11)
    rows = {}

    def timed(label, fns, nbytes, r=reps):
        for f in fns:
            assert f() == 0, (label, L.sora_hip_last_error())
        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(); e0.record()
        for i in range(r):
            fns[i % len(fns)]()
        e1.record(); torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / r
        rows[label] = {"streams": ns, "ms": round(ms, 4), "algorithmic_bytes": int(nbytes), "gb_s": round(nbytes / ms / 1e6, 1), "hbm_peak_gb_s": HBM_PEAK / 1e9,
                       "frac_hbm": round(nbytes / (ms * 1e-3) / HBM_PEAK, 4), "buffer_sets": len(fns)}
        print(json.dumps({"row": label, **rows[label]}), flush=True)
        return ms

    c16 = lambda n: [torch.randint(-9000, 9000, (n, 2), dtype=torch.int16, device=dev, generator=g) for _ in range(nsets)]
    u8 = lambda n: [torch.randint(0, 256, (n,), dtype=torch.uint8, device=dev, generator=g) for _ in range(nsets)]
    ar = torch.arange(ns, device=dev, dtype=torch.int64)
    tab = lambda per: (ar * per).to(torch.int32).contiguous()
    full = lambda v: torch.full((ns,), v, dtype=torch.int32, device=dev)
    state = torch.zeros((ns, 4), dtype=torch.int32, device=dev)

    # ---- one 11 Mbps x 1500-byte frame per stream
    nby = 1500
    chips = c16(ns * nby * 8); by = u8(ns * nby); out = [torch.empty(ns * nby, dtype=torch.uint8, device=dev) for _ in range(nsets)]
    n, of = full(nby), tab(nby)
    f11 = tab(nby * 8)
    timed("cck11_decode", [(lambda a=a, b=b: L.sora_hip_cck11_decode11b(P(a), P(f11), P(n), P(of), P(state), P(b), ns, nby, st)) for a, b in zip(chips, out)], ns * nby * 33)
    n5 = full(nby // 2); of5 = tab(nby // 2)
    timed("cck5p5_decode", [(lambda a=a, b=b: L.sora_hip_cck5p5_decode11b(P(a), P(f11), P(n5), P(of5), P(state), P(b), ns, nby // 2, st)) for a, b in zip(chips, out)],
          ns * (nby // 2) * 65)
    del chips
    timed("desc741", [(lambda a=a, b=b: L.sora_hip_desc741_11b(P(a), P(of), P(n), P(of), P(state), P(b), ns, nby, st)) for a, b in zip(by, out)], ns * nby * 2)
    rec = torch.zeros((ns, 2), dtype=torch.int32, device=dev)
    timed("frame_sink", [(lambda a=a: L.sora_hip_frame_sink11b(P(a), P(of), P(n), P(rec), ns, st)) for a in by], ns * nby)
    del by, out
    # ---- one 1 Mbps x 500-byte frame per stream
    nsym = 500 * 8
    chips = c16(ns * nsym * 11); sym = [torch.empty((ns * nsym, 2), dtype=torch.int16, device=dev) for _ in range(nsets)]
    fc, nsy, fs = tab(nsym * 11), full(nsym), tab(nsym)
    timed("despread", [(lambda a=a, b=b: L.sora_hip_despread11b(P(a), P(fc), P(nsy), P(fs), P(b), ns, nsym, st)) for a, b in zip(chips, sym)], ns * nsym * 48)
    del chips
    out = [torch.empty(ns * 500, dtype=torch.uint8, device=dev) for _ in range(nsets)]
    nb, fb = full(500), tab(500)
    timed("dbpsk_demap", [(lambda a=a, b=b: L.sora_hip_dbpsk_demap11b(P(a), P(fs), P(nb), P(fb), P(state), P(b), ns, 500, st)) for a, b in zip(sym, out)], ns * 500 * 33)
    del sym, out
    nblk = nsym * 11 * 4 // 28                                                  # 6285 blocks of 28 samples
    smp = c16(ns * nblk * 28); ch = [torch.empty((ns * nblk * 8, 2), dtype=torch.int16, device=dev) for _ in range(nsets)]
    fx, nbl, fo = tab(nblk * 28), full(nblk), tab(nblk * 8)
    sst = torch.zeros((ns, 2), dtype=torch.int32, device=dev); sst[:, 0] = 2
    nch = torch.zeros(ns, dtype=torch.int32, device=dev)
    symt = lambda lib: [(lambda a=a, b=b: lib.sora_hip_symtiming11b(P(a), P(fx), P(nbl), P(fo), P(sst), P(b), P(nch), ns, nblk, st)) for a, b in zip(smp, ch)]
    ms = timed("symtiming", symt(L), ns * nblk * (112 + 28), r=max(2, reps // 3))
    # the scan's share: the same kernel without thread 0's walk (a tools variant of the library)
    var = os.path.join(os.path.dirname(build.LIB), "variants", "symt_no_scan.so")
    if not os.path.exists(var) or os.path.getmtime(var) < os.path.getmtime(build.LIB):
        var = build.build_variant("symt_no_scan", ["SORA_DBG_SYMT_NO_SCAN"])
    V = ctypes.CDLL(var)
    V.sora_hip_symtiming11b.argtypes = L.sora_hip_symtiming11b.argtypes
    ms0 = timed("symtiming_without_the_scan", symt(V), ns * nblk * (112 + 28), r=max(2, reps // 3))
    n19 = full(19000)
    one = lambda lib: [lambda: lib.sora_hip_symtiming11b(P(smp[0]), P(fx), P(n19), P(fo), P(sst), P(ch[0]), P(nch), 1, 19000, st)]
    m1 = timed("symtiming_one_stream_19000_blocks", one(L), 19000 * 140, r=5); m10 = timed("symtiming_one_stream_without_the_scan", one(V), 19000 * 140, r=5)
    rows["symtiming"]["scan_share"] = round(max(0.0, 1 - ms0 / ms), 3)
    rows["symtiming_one_stream_19000_blocks"]["scan_share"] = round(max(0.0, 1 - m10 / m1), 3)
    return rows


def bench_chain(torch, sora, dev, ncaps, reps=3):
    import rx11b_ext_model as rxm
    import tx11b_model as txm
    rng = np.random.default_rng(0x11B)
    base = []
    for _ in range(64):
        w, _ = txm.tx11b(rng.integers(0, 256, 1500).astype(np.uint8).tobytes(), 11000, preamble=0)
        base.append(rxm.capture(rng, [w], [2000], 5.0, scale=96))
    n0 = max(len(c) for c in base)
    base = [np.concatenate([c, np.zeros((n0 - len(c), 2), np.int16)]) for c in base]
    iq = np.concatenate(base * (ncaps // 64))
    descs = [(i * n0, n0) for i in range(ncaps)]
    d_iq = torch.from_numpy(iq).to(dev)
    rx = sora.Rx11b(ncaps, len(iq), max_frames_per_capture=4)
    caps = [(o, n, i) for i, (o, n) in enumerate(descs)]
    rx.process_dev(d_iq, caps); rows = rx.results()
    firsts = {}
    for r in rows:
        firsts.setdefault(r["capture_id"], r)
    t = []
    for _ in range(reps):
        t0 = time.perf_counter(); ev = sora.rx11b_by_stages(d_iq, descs, 0); t.append(time.perf_counter() - t0)
    equal = all(e is not None and (e["error_code"], e["length"], e["mpdu"][:-1]) == (firsts[i]["error_code"], firsts[i]["length"], firsts[i]["mpdu"][:-1]) for i, e in enumerate(ev))
    h = []
    for _ in range(reps + 2):
        torch.cuda.synchronize(); t0 = time.perf_counter(); tk = rx.process_dev(d_iq, caps); rx.wait(tk); h.append(time.perf_counter() - t0)
    rx.close()
    out = {"workload": "%d captures of %d samples, one 11 Mbps x 1500-byte frame each" % (ncaps, n0), "first_events_equal_the_handles": bool(equal),
           "decoded": sum(e is not None and e["error_code"] == 1 for e in ev),
           "by_stages_ms": round(1e3 * float(np.median(t)), 1), "handle_ms": round(1e3 * float(np.median(h[2:])), 2)}
    out["by_stages_over_handle"] = round(out["by_stages_ms"] / out["handle_ms"], 1)
    print(json.dumps({"row": "chain", **out}), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "11b_stages.json"))
    a = ap.parse_args()
    import torch
    import sora_amd
    dev = torch.device("cuda", 0)
    rec = {"tool": "tools/bench_11b_stages.py", "device": torch.cuda.get_device_name(0), "streams": a.streams, "reps": a.reps,
           "stages": bench_stages(torch, sora_amd, dev, a.streams, a.reps)}
    torch.cuda.empty_cache()
    rec["chain"] = bench_chain(torch, sora_amd, dev, a.streams)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")
    return 0 if rec["chain"]["first_events_equal_the_handles"] else 1


if __name__ == "__main__":
    sys.exit(main())
