"""The stages that complete the 802.11n receive graph (sora_amd/csrc/k_11n.hip: cca11n, data_symbol11n, stream_join11n, desc11a, frame_sink11a) against the HBM roofline,
beside sora_hip_fft64 in the same run, and the composition of all the graph's stages against the sora_rx11n_* handle.  Nothing here is a gate.

Per-stage rows, 8192 streams / frames per call, two buffer sets in rotation, device events after a warm-up, on a 1500-byte MCS 10 frame's worth of data per frame: 78 OFDM
symbols (data_symbol: 2 x 78 x 80 samples in, 2 x 78 x 64 out; stream_join: 78 x 208 soft values; fft64: 2 x 78 symbols), 1500 bytes for the tail.  cca11n: 8192 streams of
2048 bursts, noise with a recorded frame at the end (the stream is consumed up to the L-STF's fall).  A row gives microseconds per call, the algorithmic bytes (input +
output, from the shapes; for cca11n the samples consumed), GB/s and the fraction of benchlib.common.HBM_PEAK.  k_cca11n's registers and LDS are read from the library's code
object.

Composition row: sora_amd.rx11n_by_stages (host wall clock: it reads counts back between stages, and the data field goes symbol by symbol) against Rx11n.process_dev + wait
on the same captures, one MCS 10 x 1500-byte frame each behind 400 .. 1400 samples.
usage: python tools/bench_11n_rx_stages.py [--streams N] [--chain-captures N] [--reps R] [--out profiles/11n_rx_stages.json]   -> one JSON line per row, the record in the file"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def kernel_resources(name):
    """{vgpr_count, sgpr_count, group_segment_fixed_size, private_segment_fixed_size} of kernel `name` in libsora_hip.so, or None where the LLVM tools are missing"""
    from sora_amd import build
    from test_isa_dpp_guard import LLVM, code_objects
    if not os.path.exists(os.path.join(LLVM, "llvm-readobj")):
        return None
    with tempfile.TemporaryDirectory() as d:
        fat = os.path.join(d, "fatbin")
        subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", build.LIB, fat])
        for k, co in enumerate(code_objects(open(fat, "rb").read())):
            if name.encode() not in co:
                continue
            p = os.path.join(d, "co%d.o" % k)
            with open(p, "wb") as fh:
                fh.write(co)
            notes = subprocess.run([os.path.join(LLVM, "llvm-readobj"), "--notes", p], capture_output=True, text=True, check=True).stdout
            for blk in re.split(r"\n\s*- \.agpr_count:", notes)[1:]:
                nm = re.search(r"\.name:\s+(\S+)", blk)
                if nm and name in nm.group(1):
                    return {f: int(v) for f, v in re.findall(r"\.(vgpr_count|sgpr_count|group_segment_fixed_size|private_segment_fixed_size):\s+(\d+)", blk)}
    return None


def bench_stages(torch, sora, dev, ns, reps, nsets=2):
    from benchlib.common import HBM_PEAK
    from sora_amd import capi
    import rx11n_stage_cases as cases
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
        rows[label] = {"streams": ns, "us": round(1e3 * ms, 1), "algorithmic_bytes": int(nbytes), "gb_s": round(nbytes / ms / 1e6, 1), "hbm_peak_gb_s": HBM_PEAK / 1e9,
                       "frac_hbm": round(nbytes / (ms * 1e-3) / HBM_PEAK, 4), "buffer_sets": len(fns)}
        print(json.dumps({"row": label, **rows[label]}), flush=True)

    c16 = lambda n: [torch.randint(-9000, 9000, (n, 2), dtype=torch.int16, device=dev, generator=g) for _ in range(nsets)]
    u8 = lambda n, hi=256: [torch.randint(0, hi, (n,), dtype=torch.uint8, device=dev, generator=g) for _ in range(nsets)]
    ar = torch.arange(ns, device=dev, dtype=torch.int64)
    tab = lambda per: (ar * per).to(torch.int32).contiguous()
    full = lambda v: torch.full((ns,), v, dtype=torch.int32, device=dev)
    nsym = 78                                                                   # a 1500-byte MCS 10 frame: ceil((16 + 8 * 1500 + 6) / 156)
    # ---- T11nDataSymbol, and TFFT64 on what it writes
    x0, x1 = c16(ns * nsym * 80), c16(ns * nsym * 80)
    y0 = [torch.empty((ns * nsym * 64, 2), dtype=torch.int16, device=dev) for _ in range(nsets)]; y1 = [torch.empty_like(y0[0]) for _ in range(nsets)]
    f80, n78, o78 = tab(nsym * 80), full(nsym), tab(nsym)
    timed("data_symbol11n", [(lambda a=a, b=b, c=c, d=d: L.sora_hip_data_symbol11n(P(a), P(b), P(f80), P(n78), P(o78), P(c), P(d), ns, nsym, st))
                             for a, b, c, d in zip(x0, x1, y0, y1)], ns * nsym * 2 * (80 + 64) * 4)
    del x0, x1
    timed("fft64", [(lambda a=a, b=b: L.sora_hip_fft64(P(a), P(b), 2 * ns * nsym // 2, st)) for a, b in zip(y0, y1)], ns * nsym * 64 * 4 * 2)
    del y0, y1
    # ---- TStreamJoin + TStreamConcat, QPSK
    s0, s1 = u8(ns * nsym * 104, 8), u8(ns * nsym * 104, 8)
    jo = [torch.empty(ns * nsym * 208, dtype=torch.uint8, device=dev) for _ in range(nsets)]
    timed("stream_join11n", [(lambda a=a, b=b, c=c: L.sora_hip_stream_join11n(P(a), P(b), P(c), 2, ns * nsym, st)) for a, b, c in zip(s0, s1, jo)], ns * nsym * 416)
    del s0, s1, jo
    # ---- T11aDesc, TBB11aFrameSink
    nby = 1500
    dec = u8(ns * 1504); out = [torch.empty(ns * 1504, dtype=torch.uint8, device=dev) for _ in range(nsets)]
    off, ln = tab(1504), full(nby)
    timed("desc11a", [(lambda a=a, b=b: L.sora_hip_desc11a(P(a), P(off), P(ln), P(b), P(off), ns, st)) for a, b in zip(dec, out)], ns * (2 * nby + 2))
    rec = torch.zeros((ns, 2), dtype=torch.int32, device=dev)
    timed("frame_sink11a", [(lambda a=a: L.sora_hip_frame_sink11a(P(a), P(off), P(ln), P(rec), ns, st)) for a in out], ns * nby)
    del dec, out
    # ---- TCCA11n: 2048 bursts per stream, the frame at the end
    z = np.load(cases.GOLD)
    rng = np.random.default_rng(7)
    nbur = 2048
    a, b = cases.capture40(rng, [(z["tx1_0"], z["tx1_1"])], [2 * 4 * nbur - 2880], sigma=20.0, tail=0)
    a, b = cases.down2(a)[:4 * nbur], cases.down2(b)[:4 * nbur]
    import rx11n_stage_model as model
    want_state, want_used = model.cca(a, b, capi.cca11n_states(1)[0], capi.CCA11N_REARM)
    d0 = torch.from_numpy(a).to(dev).repeat(ns, 1).contiguous(); d1 = torch.from_numpy(b).to(dev).repeat(ns, 1).contiguous()
    fresh = torch.from_numpy(capi.cca11n_states(ns)).to(dev)
    sts = [fresh.clone() for _ in range(nsets)]
    used = torch.zeros(ns, dtype=torch.int32, device=dev)
    fb, nb_ = tab(4 * nbur), full(nbur)

    def cca(s):
        s.copy_(fresh)                                                          # (a constructed record each time: 8.7 MB of the call's traffic, counted below)
        return L.sora_hip_cca11n(P(d0), P(d1), P(fb), P(nb_), P(s), P(used), ns, nbur, capi.CCA11N_REARM, st)

    timed("cca11n", [(lambda s=s: cca(s)) for s in sts], ns * (want_used * 4 * 4 * 2 + 3 * 1056))
    ok = bool((used.cpu().numpy() == want_used).all() and (sts[0].cpu().numpy() == want_state).all())
    rows["cca11n"].update({"bursts_per_stream": nbur, "bursts_consumed": int(want_used), "equals_the_model": ok, "kernel": kernel_resources("k_cca11n"),
                           "note": "the time includes the copy that re-arms the records"})
    print(json.dumps({"row": "cca11n", **rows["cca11n"]}), flush=True)
    return rows


def bench_chain(torch, sora, dev, ncaps, reps=3):
    import rx11n_ext_model as ext
    rng = np.random.default_rng(0x11)
    o0, o1, off = sora.tx11n([rng.integers(0, 256, 1496).astype(np.uint8).tobytes() for _ in range(16)], [10] * 16)
    a, b = o0.cpu().numpy(), o1.cpu().numpy()
    base = [ext.clean_channel(rng, a[off[i]:off[i + 1]], b[off[i]:off[i + 1]], sigma=15.0, lead=int(rng.integers(400, 1401))) for i in range(16)]
    n0 = max(len(c[0]) for c in base)
    pad = lambda c: np.concatenate([c, np.zeros((n0 - len(c), 2), np.int16)])
    iq0 = np.concatenate([pad(c[0]) for c in base] * (ncaps // 16)); iq1 = np.concatenate([pad(c[1]) for c in base] * (ncaps // 16))
    ncaps = ncaps // 16 * 16
    descs = [(i * n0, n0) for i in range(ncaps)]
    d0, d1 = torch.from_numpy(iq0).to(dev), torch.from_numpy(iq1).to(dev)
    rx = sora.Rx11n(ncaps, len(iq0))
    caps = [(o, n, i) for i, (o, n) in enumerate(descs)]
    rx.process_dev(d0, d1, caps); rows = rx.results()
    firsts = {}
    for r in sorted(rows, key=lambda r: r["end_sample"]):
        firsts.setdefault(r["capture_id"], r)
    t = []
    for _ in range(reps):
        torch.cuda.synchronize(); t0 = time.perf_counter(); ev = sora.rx11n_by_stages(d0, d1, descs); t.append(time.perf_counter() - t0)
    key = lambda r: (r["error_code"], r["rate_kbps"], r["length"], r["crc32"], r["mpdu"])
    equal = all(e is not None and i in firsts and key(e) == key(firsts[i]) for i, e in enumerate(ev))
    h = []
    for _ in range(reps + 2):
        torch.cuda.synchronize(); t0 = time.perf_counter(); tk = rx.process_dev(d0, d1, caps); rx.wait(tk); h.append(time.perf_counter() - t0)
    rx.close()
    out = {"workload": "%d captures of %d samples, one MCS 10 x 1500-byte frame each" % (ncaps, n0), "first_events_equal_the_handles": bool(equal),
           "decoded": sum(e is not None and e["error_code"] == 1 for e in ev),
           "by_stages_ms": round(1e3 * float(np.median(t)), 1), "handle_ms": round(1e3 * float(np.median(h[2:])), 2)}
    out["by_stages_over_handle"] = round(out["by_stages_ms"] / out["handle_ms"], 1)
    print(json.dumps({"row": "chain", **out}), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=8192)
    ap.add_argument("--chain-captures", type=int, default=512)
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "11n_rx_stages.json"))
    a = ap.parse_args()
    import torch
    import sora_amd
    dev = torch.device("cuda", 0)
    rec = {"tool": "tools/bench_11n_rx_stages.py", "device": torch.cuda.get_device_name(0), "streams": a.streams, "reps": a.reps,
           "stages": bench_stages(torch, sora_amd, dev, a.streams, a.reps)}
    torch.cuda.empty_cache()
    rec["chain"] = bench_chain(torch, sora_amd, dev, a.chain_captures)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")
    return 0 if rec["chain"]["first_events_equal_the_handles"] and rec["stages"]["cca11n"]["equals_the_model"] else 1


if __name__ == "__main__":
    sys.exit(main())
