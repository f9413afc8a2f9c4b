"""The 802.11a modulation graph's stage entry points (sora_amd/csrc/k_mod.hip) against the HBM roofline, and the chain composed of them against the fused
transmitter.

Per-stage rows: each stage over 2^20 OFDM symbols of a 54 Mbps stream (64-QAM, rate 3/4: 27 data bytes, 36 coded bytes, 48 carriers, 64 bins, 160 samples per
symbol; 4096 frames of 256 symbols where a stage takes frames), three distinct buffer sets in rotation so that consecutive launches share no line (the
symbol-wide stages have 1.3 to 4.2 GB in play, far past the 256 MiB Infinity Cache; the byte-wide ones 170 to 690 MB), timed with device events after a warm-up.
A row gives ms, the algorithmic bytes (input + output, from the shapes), GB/s and the fraction of benchlib.common.HBM_PEAK.  sora_hip_fft128 over the same number
of transforms, in the same run, is the yardstick for ifftx (the same butterflies; 512 + 512 bytes against 256 + 640).

Chain row: Mod11aStages.run() (the nine stages, every intermediate through HBM, a gather into frame order at the end) against sora_hip_tx11a on 4096 x 1500-byte
MPDUs at 54 Mbps, the two alternated block by block; the ratio is reported, it is not a gate.
usage: python tools/bench_mod_stages.py [--nsym N] [--reps R] [--out profiles/mod_stages.json]   -> one JSON line per row, the whole record in the file"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def bench_stages(torch, sora_amd, dev, nsym, reps, nsets=3):
    from benchlib.common import HBM_PEAK
    from sora_amd import capi
    L = capi.load()
    P = capi._dev_ptr
    st = capi._stream_ptr(None)
    g = torch.Generator(device=dev); g.manual_seed(11)
    rows = {}

    def timed(label, fns, nbytes, n=nsym):
        for f in fns:
            assert f() == 0, (label, L.sora_hip_last_error())
        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(); e0.record()
        for i in range(reps):
            fns[i % len(fns)]()
        e1.record(); torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / reps
        rows[label] = {"symbols": n, "ms": round(ms, 4), "algorithmic_bytes": int(nbytes), "gb_s": round(nbytes / ms / 1e6, 1), "hbm_peak_gb_s": HBM_PEAK / 1e9,
                       "frac_hbm": round(nbytes / (ms * 1e-3) / HBM_PEAK, 4), "buffer_sets": len(fns), "bytes_in_play": int(nbytes) * len(fns)}
        print(json.dumps({"row": label, **rows[label]}), flush=True)

    u8 = lambda *shape: [torch.randint(0, 256, shape, dtype=torch.uint8, device=dev, generator=g) for _ in range(nsets)]
    c16 = lambda *shape: [torch.randint(-9000, 9000, shape + (2,), dtype=torch.int16, device=dev, generator=g) for _ in range(nsets)]
    like = lambda xs, *shape, dt=None: [torch.empty(shape or xs[0].shape, dtype=dt or xs[0].dtype, device=dev) for _ in range(nsets)]
    fsym = 256; nfr = nsym // fsym                                               # frames of 256 symbols
    ar = torch.arange(nfr, device=dev, dtype=torch.int32)

    # T11aSc: 27 bytes per symbol in and out
    x = u8(nsym * 27); y = like(x)
    off = (ar * (fsym * 27)).contiguous(); ln = torch.full((nfr,), fsym * 27, dtype=torch.int32, device=dev)
    tail = torch.full((nfr,), fsym * 27 - 20, dtype=torch.int32, device=dev); seed = torch.full((nfr,), 0x5B, dtype=torch.uint8, device=dev)
    timed("scramble", [(lambda a=a, b=b: L.sora_hip_scramble11a(P(a), P(b), P(off), P(ln), P(tail), P(seed), nfr, fsym * 27, st)) for a, b in zip(x, y)], nsym * 54)
    # TConvEncode_34: 27 -> 36
    c = like(x, nsym * 36); ooff = (ar * (fsym * 36)).contiguous()
    timed("conv_encode_34", [(lambda a=a, b=b: L.sora_hip_conv_encode11a(P(a), P(off), P(ln), 2, P(b), P(ooff), nfr, fsym * 27, st)) for a, b in zip(x, c)], nsym * 63)
    del x, y
    # T11aInterleaveQAM64: 36 -> 36
    il = like(c)
    timed("interleave_qam64", [(lambda a=a, b=b: L.sora_hip_interleave11a(P(a), P(b), 6, nsym, st)) for a, b in zip(c, il)], nsym * 72)
    del c
    # TMap11aQAM64: 36 -> 192
    car = like(il, nsym, 48, 2, dt=torch.int16)
    timed("map_qam64", [(lambda a=a, b=b: L.sora_hip_map11a(P(a), P(b), 6, 0, nsym, st)) for a, b in zip(il, car)], nsym * 228)
    del il
    # T11aAddPilot: 192 -> 256
    bins = like(car, nsym, 64, 2)
    first = (ar * fsym).contiguous(); ns = torch.full((nfr,), fsym, dtype=torch.int32, device=dev)
    timed("add_pilot", [(lambda a=a, b=b: L.sora_hip_add_pilot11a(P(a), P(b), P(first), P(ns), nfr, 0, st)) for a, b in zip(car, bins)], nsym * 448)
    del car
    # TIFFTx: 256 -> 640, and FFT<128> (512 -> 512) on the same count as its yardstick
    t = like(bins, nsym, 160, 2)
    timed("ifftx", [(lambda a=a, b=b: L.sora_hip_ifftx11a(P(a), P(b), nsym, st)) for a, b in zip(bins, t)], nsym * 896)
    del bins
    x128 = c16(nsym, 128); y128 = like(x128)
    timed("fft128_yardstick", [(lambda a=a, b=b: L.sora_hip_fft128(P(a), P(b), nsym, st)) for a, b in zip(x128, y128)], nsym * 1024)
    del x128, y128
    rows["ifftx"]["bytes_per_s_over_fft128"] = round(rows["ifftx"]["gb_s"] / rows["fft128_yardstick"]["gb_s"], 3)
    rows["ifftx"]["symbols_per_s_over_fft128"] = round(rows["fft128_yardstick"]["ms"] / rows["ifftx"]["ms"], 3)
    # TPackSample16to8: 640 -> 320
    o8 = like(t, nsym, 160, 2, dt=torch.int8)
    timed("pack16to8", [(lambda a=a, b=b: L.sora_hip_pack16to8(P(a), P(b), nsym * 160, st)) for a, b in zip(t, o8)], nsym * 960)
    del o8
    # TUpsample40MTo44M: 640 -> 704, every fourth block not seeing its successor (the preamble's pattern)
    u = like(t, nsym, 176, 2)
    sees = (torch.arange(nsym, device=dev) % 4 != 3).to(torch.uint8)
    timed("upsample40to44", [(lambda a=a, b=b: L.sora_hip_upsample40to44(P(a), P(b), P(sees), nsym, st)) for a, b in zip(t, u)], nsym * 1344)
    del u
    # TTS11aSrc: 640 samples = four symbols' worth per copy, nothing read
    timed("preamble", [(lambda b=b: L.sora_hip_preamble11a(P(b), nsym // 4, st)) for b in t], nsym * 640)
    del t
    return rows


def bench_chain(torch, sora_amd, dev, nframes=4096, mpdu_len=1496, rate=54000, reps=5, blocks=5):
    from benchlib.common import HBM_PEAK
    from sora_amd import capi
    L = capi.load()
    P = capi._dev_ptr
    rng = np.random.default_rng(0x5EED)
    mpdus = [bytes(rng.integers(0, 256, mpdu_len).astype(np.uint8)) for _ in range(64)] * (nframes // 64)
    plan = sora_amd.Mod11aStages(mpdus, [rate] * nframes)
    want, off = sora_amd.tx11a(mpdus, [rate] * nframes)
    got = plan.run(); torch.cuda.synchronize()
    equal = bool(torch.equal(got, want))
    per = off[1] - off[0]
    blob = torch.from_numpy(np.frombuffer(b"".join(mpdus), np.uint8).copy()).to(dev)
    moff = torch.arange(nframes, dtype=torch.int32, device=dev) * mpdu_len
    lens = torch.full((nframes,), mpdu_len, dtype=torch.int32, device=dev); rates = torch.full((nframes,), rate, dtype=torch.int32, device=dev)
    seeds = torch.full((nframes,), 0xFF, dtype=torch.uint8, device=dev); ooff = torch.arange(nframes, dtype=torch.int64, device=dev) * per
    fused = lambda: L.sora_hip_tx11a(P(blob), P(moff), P(lens), P(rates), P(seeds), nframes, P(want), P(ooff), capi._stream_ptr(None))
    del got
    forms = {"tx11a_fused": (fused, []), "chain_of_stages": (plan.run, [])}
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
    alg = nframes * mpdu_len + 2 * nsamp
    out = {"workload": "%d frames x %d-byte MPDU (+FCS) at %g Mbps -> COMPLEX8 @40 MHz (%d samples)" % (nframes, mpdu_len, rate / 1000, nsamp),
           "chain_equals_fused": equal, "reps_per_block": reps, "blocks": blocks}
    for k, (_, ms) in forms.items():
        m = float(np.median(ms))
        out[k] = {"ms": round(m, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4), "msamples_per_s": round(nsamp / m / 1e3, 1),
                  "frac_hbm_of_the_frames_own_bytes": round(alg / (m * 1e-3) / HBM_PEAK, 4)}
    out["chain_over_fused"] = round(out["chain_of_stages"]["ms"] / out["tx11a_fused"]["ms"], 2)
    print(json.dumps({"row": "chain", **out}), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nsym", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mod_stages.json"))
    a = ap.parse_args()
    import torch
    import sora_amd
    dev = torch.device("cuda", 0)
    rec = {"tool": "tools/bench_mod_stages.py", "device": torch.cuda.get_device_name(0), "nsym": a.nsym, "reps": a.reps,
           "stages": bench_stages(torch, sora_amd, dev, a.nsym, a.reps)}
    torch.cuda.empty_cache()
    rec["chain"] = bench_chain(torch, sora_amd, dev)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")
    return 0 if rec["chain"]["chain_equals_fused"] else 1


if __name__ == "__main__":
    sys.exit(main())
