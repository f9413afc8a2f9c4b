"""The 40 MHz HT modulation graph's stage entry points (sora_amd/csrc/k_mod_ht40.hip) against the HBM roofline, and the chains composed of them against the fused
transmitters, on 4096 frames x 1500-byte PSDUs at MCS 10 (QPSK 3/4) and at MCS 14 (64-QAM 3/4).

Per-stage rows, per MCS: each stage over the symbols ONE spatial stream of the per-stream-coded batch has (4096 x N_SYM; sig_map and preamble over the 4096 frames),
on distinct buffer sets in rotation so that consecutive launches share no line -- as many sets as bring the bytes in play past 600 MB (the Infinity Cache holds
256 MiB), at most 16; a row whose sets stay below that says so (`past_cache: false`): its figure is a rate out of the cache, not an HBM rate.  Timed with device
events after a warm-up of every set; the calls take tens of microseconds, so a probe of --reps calls sizes the timed window to about 100 ms.  A row gives the time per
call, the algorithmic bytes (input + output, from the shapes), GB/s and the fraction of benchlib.common.HBM_PEAK.  All are bound by bytes, not by operations; ifft is
the one with arithmetic worth naming (sora_hip_fft128 over the same count, in the same run, is its yardstick: the same butterflies on the same 512 + 512 bytes).

Chain rows, per MCS and coding: ModHt40Stages.run() (every intermediate through HBM, a gather into frame order at the end) against sora_hip_tx_ht40 / _joint on the
same batch, in the same run, the two alternated block by block, medians; the ratio is reported, it is not a gate.
usage: python tools/bench_mod_ht40_stages.py [--nframes N] [--reps R] [--commit C --parent P] [--out profiles/mod_ht40_stages.json]
-> one JSON line per row, the whole record in the file"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def bench_stages(torch, dev, mcs, nframes, mpdu_len, reps, window_ms=100.0):
    from benchlib.common import HBM_PEAK
    from sora_amd import capi
    L = capi.load()
    P = capi._dev_ptr
    st = capi._stream_ptr(None)
    g = torch.Generator(device=dev); g.manual_seed(40)
    nb = capi._MCS_HT40[mcs][0]
    row = capi._row_ht40(nb)
    fsym = capi.mod_ht40_fields((bytes(mpdu_len), bytes(mpdu_len)), mcs)[5]
    nsym = nframes * fsym
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
        n = int(min(8000, max(reps, window_ms / max(window(reps), 1e-4))))        # a short probe sizes the timed window: the calls are tens of microseconds
        ms = window(n)
        rows[label] = {"units": units, "us_per_call": round(ms * 1e3, 2), "calls_timed": n, "algorithmic_bytes": int(nbytes), "gb_s": round(nbytes / ms / 1e6, 1),
                       "hbm_peak_gb_s": HBM_PEAK / 1e9, "frac_hbm": round(nbytes / (ms * 1e-3) / HBM_PEAK, 4), "buffer_sets": k, "bytes_in_play": int(nbytes) * k,
                       "past_cache": bool(nbytes * k >= 512e6)}
        print(json.dumps({"row": label, "mcs": mcs, **rows[label]}), flush=True)
        del fns
        torch.cuda.empty_cache()

    u8 = lambda *shape: torch.randint(0, 256, shape, dtype=torch.uint8, device=dev, generator=g)
    c16 = lambda *shape: torch.randint(-9000, 9000, shape + (2,), dtype=torch.int16, device=dev, generator=g)
    e8 = lambda *shape: torch.empty(shape, dtype=torch.uint8, device=dev)
    e16 = lambda *shape: torch.empty(shape + (2,), dtype=torch.int16, device=dev)
    first = (torch.arange(nframes, device=dev, dtype=torch.int32) * fsym).contiguous()
    ns = torch.full((nframes,), fsym, dtype=torch.int32, device=dev)
    fbytes = (fsym * 108 * nb + 7) // 8 + 3                                      # a frame's coded stream, frames at odd byte offsets
    soff = (torch.arange(nframes, device=dev, dtype=torch.int32) * fbytes + 1).contiguous()

    def mk_parse():
        a, b, c = u8(nsym, 27 * nb), e8(nsym, row), e8(nsym, row)
        return lambda: L.sora_hip_stream_parse_ht40(P(a), P(b), P(c), nb, nsym, st)

    def mk_interleave():
        a, b = u8(nsym, row), e8(nsym, row)
        return lambda: L.sora_hip_interleave_ht40(P(a), P(b), nb, 1, nsym, st)

    def mk_interleave_stream():
        a, b = u8(nframes * fbytes + 16), e8(nsym, row)
        return lambda: L.sora_hip_interleave_ht40_stream(P(a), P(soff), P(first), P(ns), P(b), nb, 1, nframes, st)

    def mk_map():
        a, b = u8(nsym, row), e16(nsym, 108)
        return lambda: L.sora_hip_map_ht40(P(a), P(b), nb, nsym, st)

    def mk_sig_map():
        a, b = u8(nframes, 18), e16(nframes, 384)
        return lambda: L.sora_hip_sig_map_ht40(P(a), P(b), nframes, st)

    def mk_add_pilot():
        a, b = c16(nsym, 108), e16(nsym, 128)
        return lambda: L.sora_hip_add_pilot_ht40(P(a), P(b), P(first), P(ns), nframes, st)

    def mk_ifft():
        a, b = c16(nsym, 128), e16(nsym, 128)
        return lambda: L.sora_hip_ifft_ht40(P(a), P(b), nsym, st)

    def mk_fft128():
        a, b = c16(nsym, 128), e16(nsym, 128)
        return lambda: L.sora_hip_fft128(P(a), P(b), nsym, st)

    def mk_add_gi(gi):
        def mk():
            a, b = c16(nsym, 128), e16(nsym, 144 if gi else 160)
            return lambda: L.sora_hip_add_gi_ht40(P(a), P(b), gi, nsym, st)
        return mk

    def mk_preamble(field):
        def mk():
            a, b = e16(nframes, 480 if field else 640), e16(nframes, 480 if field else 640)
            return lambda: L.sora_hip_preamble_ht40(P(a), P(b), field, nframes, st)
        return mk

    timed("stream_parse", mk_parse, nsym * (27 * nb + 2 * row), nsym)
    timed("interleave", mk_interleave, nsym * 2 * row, nsym)
    timed("interleave_stream", mk_interleave_stream, nsym * 2 * row, nsym)
    timed("map", mk_map, nsym * (row + 432), nsym)
    timed("sig_map", mk_sig_map, nframes * (18 + 1536), nframes)
    timed("add_pilot", mk_add_pilot, nsym * (432 + 512), nsym)
    timed("ifft", mk_ifft, nsym * 1024, nsym)
    timed("fft128_yardstick", mk_fft128, nsym * 1024, nsym)
    rows["ifft"]["symbols_per_s_over_fft128"] = round(rows["fft128_yardstick"]["us_per_call"] / rows["ifft"]["us_per_call"], 3)
    timed("add_gi_long", mk_add_gi(0), nsym * (512 + 640), nsym)
    timed("add_gi_short", mk_add_gi(1), nsym * (512 + 576), nsym)
    timed("preamble_l", mk_preamble(0), nframes * 2 * 640 * 4, nframes)
    timed("preamble_ht", mk_preamble(1), nframes * 2 * 480 * 4, nframes)
    return {"symbols_per_stream": nsym, "symbols_per_frame": fsym, "rows": rows}


def bench_chain(torch, sora_amd, dev, mcs, nframes, mpdu_len, joint, reps=40, blocks=7):
    from benchlib.common import HBM_PEAK
    from sora_amd import capi
    L = capi.load()
    P = capi._dev_ptr
    rng = np.random.default_rng(0x5EED)
    mp0 = [bytes(rng.integers(0, 256, mpdu_len).astype(np.uint8)) for _ in range(64)] * (nframes // 64)
    mp1 = [bytes(rng.integers(0, 256, mpdu_len).astype(np.uint8)) for _ in range(64)] * (nframes // 64)
    nstr = 1 if joint else 2
    plan = sora_amd.ModHt40Stages(mp0, None if joint else mp1, [mcs] * nframes)
    w0, w1, off = sora_amd.tx_ht40_joint(mp0, [mcs] * nframes) if joint else sora_amd.tx_ht40(mp0, mp1, [mcs] * nframes)
    g0, g1 = plan.run(); torch.cuda.synchronize()
    equal = bool(torch.equal(g0, w0) and torch.equal(g1, w1))
    del g0, g1
    per = off[1] - off[0]
    stride = (mpdu_len + 3) // 4 * 4
    blob = np.zeros(nstr * nframes * stride, np.uint8)
    for f in range(nframes):
        for s, m in enumerate((mp0[f],) if joint else (mp0[f], mp1[f])):
            at = (nstr * f + s) * stride
            blob[at:at + mpdu_len] = np.frombuffer(m, np.uint8)
    blob = torch.from_numpy(blob).to(dev)
    moff = torch.arange(nstr * nframes, dtype=torch.int32, device=dev) * stride
    lens = torch.full((nframes,), mpdu_len, dtype=torch.int32, device=dev); vmcs = torch.full((nframes,), mcs, dtype=torch.int32, device=dev)
    ooff = torch.arange(nframes, dtype=torch.int64, device=dev) * per
    entry = L.sora_hip_tx_ht40_joint if joint else L.sora_hip_tx_ht40
    name = "tx_ht40_joint_fused" if joint else "tx_ht40_fused"
    fused = lambda: entry(P(blob), P(moff), P(lens), P(vmcs), None, nframes, P(w0), P(w1), P(ooff), capi._stream_ptr(None))
    forms = {name: (fused, []), "chain_of_stages": (plan.run, [])}
    for fn, _ in forms.values():
        fn()
    torch.cuda.synchronize()
    for _ in range(blocks):
        for fn, ms in forms.values():
            e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record(); torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1) / reps)
    nsamp = per * nframes
    alg = nstr * nframes * mpdu_len + 2 * 4 * nsamp
    out = {"workload": "%d frames x %d x %d-byte MPDU (+FCS) at MCS %d, %s coding -> 2 x COMPLEX16 @40 MHz (%d samples per chain)"
                       % (nframes, nstr, mpdu_len, mcs, "joint" if joint else "per-stream", nsamp),
           "chain_equals_fused": equal, "reps_per_block": reps, "blocks": blocks}
    for k, (_, ms) in forms.items():
        m = float(np.median(ms))
        out[k] = {"ms": round(m, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4), "msamples_per_s_per_chain": round(nsamp / m / 1e3, 1),
                  "frac_hbm_of_the_frames_own_bytes": round(alg / (m * 1e-3) / HBM_PEAK, 4)}
    out["chain_over_fused"] = round(out["chain_of_stages"]["ms"] / out[name]["ms"], 2)
    print(json.dumps({"row": "chain_joint" if joint else "chain_per_stream", "mcs": mcs, **out}), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nframes", type=int, default=4096)
    ap.add_argument("--mpdu-len", type=int, default=1496, help="bytes without the FCS: 1500 with it")
    ap.add_argument("--reps", type=int, default=24)
    ap.add_argument("--commit", default=None, help="recorded in the file: the commit that is measured")
    ap.add_argument("--parent", default=None, help="recorded in the file: its parent")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mod_ht40_stages.json"))
    a = ap.parse_args()
    import torch
    import sora_amd
    if not torch.cuda.is_available():
        sys.exit("bench_mod_ht40_stages: no GPU -- nothing is measured without one")
    dev = torch.device("cuda", 0)
    rec = {"tool": "tools/bench_mod_ht40_stages.py", "device": torch.cuda.get_device_name(0), "commit": a.commit, "parent": a.parent, "nframes": a.nframes,
           "mpdu_len": a.mpdu_len, "reps": a.reps, "mcs": {}}
    ok = True
    for mcs in (10, 14):
        r = {"stages": bench_stages(torch, dev, mcs, a.nframes, a.mpdu_len, a.reps)}
        torch.cuda.empty_cache()
        for joint in (False, True):
            key = "chain_joint" if joint else "chain_per_stream"
            r[key] = bench_chain(torch, sora_amd, dev, mcs, a.nframes, a.mpdu_len, joint)
            torch.cuda.empty_cache()
            ok = ok and r[key]["chain_equals_fused"]
        rec["mcs"][str(mcs)] = r
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
