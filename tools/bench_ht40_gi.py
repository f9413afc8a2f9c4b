"""The short guard interval of the 40 MHz HT 2x2 pair (sora_hip_tx_ht40_gi, SORA_HT40_SHORT_GI, sora_ht40_set_guard) beside the long one, one run
on one box: 4096 per-stream frames of 2 x 1500-byte PSDUs per call at MCS 14 and at MCS 8, as three rows, each in a process of its own under `timeout -k 10`:
  tx        the transmitter: sora_hip_tx_ht40 (long), sora_hip_tx_ht40_gi with every kind 0 (long) and with every kind 1 (short); wall clock over 10 x reps back-to-back calls, then a synchronize;
  rx_desc   the descriptor form of the receiver on what the transmitter sent (identity channel at the level the receiver's tests use, zero forcing): long frames, and
            the same payloads behind the short guard interval with SORA_HT40_SHORT_GI on the code rate; wall clock over back-to-back sora_ht40_process_dev calls, eight
            in flight, then a synchronize;
  rx_raw    the raw-capture form, one frame per capture: SORA_HT40_GUARD_LONG and SORA_HT40_GUARD_SIGNALLED on the long-GI captures, SORA_HT40_GUARD_SIGNALLED on the
            same payloads behind the short guard interval; wall clock over back-to-back sora_ht40_process_captures_dev calls, then a synchronize.
Within a row the variants ALTERNATE, block after block of `reps` calls, `blocks` times: every figure is reported as the list of its blocks' means (ms per call), so the
spread of a figure and the difference between two variants come from the same run.  Every variant's last call is checked: all rows FRAME_OK, the short ones flagged.
On a library without the option (the parent commit: copy this file into its tools/) only the long variants run: the figures to compare this commit's with.
usage: python tools/bench_ht40_gi.py [frames] [reps] [blocks]   -> one JSON line per row"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ROW_TIMEOUT_S = 400
GAIN = 250.0 * 128.0 / 16384.0        # tests/test_gpu_tx_ht40.py: the level at which the receiver's own tests decode
MCS2 = {8: (1, 0), 9: (2, 0), 10: (2, 2), 11: (4, 0), 12: (4, 2), 13: (6, 1), 14: (6, 2)}
MPDU = 1496                           # + FCS = 1500-byte PSDUs, one per stream
SHORT, ROW_SHORT_GI = 0x100, 4


def _alternate(variants, reps, blocks, sync):
    """variants: {name: call} -> {name: [ms per call of each block]}; warmed up, alternating"""
    out = {k: [] for k in variants}
    for k, call in variants.items():
        for _ in range(3):
            call()
    sync()
    for _ in range(blocks):
        for k, call in variants.items():
            t0 = time.perf_counter()
            for _ in range(reps):
                call()
            sync()
            out[k].append(round((time.perf_counter() - t0) * 1e3 / reps, 4))
    return out


def _tx_setup(sora_amd, capi, torch, mcs, nframes, gi, lead):
    """-> (call through the _gi entry point or the plain one, out0, out1, samples per frame slot, nsym): frame f's first sample at f * slot + lead"""
    dev = torch.device("cuda")
    L = capi.load()
    per = sora_amd.tx_ht40_samples(MPDU, mcs) if gi is None else sora_amd.tx_ht40_gi_samples(MPDU, mcs, gi)
    nsym = (per - 1600) // (144 if gi else 160)
    slot = lead + per
    slot += -slot % 28                                                        # raw captures are whole 28-sample source bursts
    lens = torch.full((nframes,), MPDU, dtype=torch.int32, device=dev); mcsv = torch.full((nframes,), mcs, dtype=torch.int32, device=dev)
    moff = torch.arange(2 * nframes, dtype=torch.int32, device=dev) * MPDU
    blob = torch.randint(0, 256, (2 * nframes * MPDU,), dtype=torch.uint8, generator=torch.Generator(device=dev).manual_seed(1), device=dev)
    ooff = torch.arange(nframes, dtype=torch.int64, device=dev) * slot + lead
    out0 = torch.zeros((nframes * slot + 256, 2), dtype=torch.int16, device=dev); out1 = torch.zeros_like(out0)
    p = capi._dev_ptr
    if gi is None:
        call = lambda: L.sora_hip_tx_ht40(p(blob), p(moff), p(lens), p(mcsv), None, nframes, p(out0), p(out1), p(ooff), None)
    else:
        kinds = torch.full((nframes,), gi, dtype=torch.uint8, device=dev)
        call = lambda: L.sora_hip_tx_ht40_gi(p(blob), p(moff), p(lens), p(mcsv), None, p(kinds), nframes, p(out0), p(out1), p(ooff), None)
    call.keep = (lens, mcsv, moff, blob, ooff)
    assert call() == 0
    torch.cuda.synchronize()
    return call, out0, out1, slot, nsym


def bench(row, mcs, nframes, reps, blocks):
    import torch
    import sora_amd
    from sora_amd import capi
    has_gi = hasattr(sora_amd, "tx_ht40_gi_samples")
    nb, cr = MCS2[mcs]
    scale = lambda o: torch.clamp(torch.round(o.float() * GAIN), -32768, 32767).to(torch.int16)
    out = {"row": "ht40_gi_%s" % row, "mcs": mcs, "frames": nframes, "psdu_bytes_per_frame": 2 * (MPDU + 4), "reps": reps, "blocks": blocks, "option_present": has_gi}
    ok = True
    if row == "tx":
        variants = {"long": _tx_setup(sora_amd, capi, torch, mcs, nframes, None, 0)[0]}
        if has_gi:
            variants["long_by_kind_0"] = _tx_setup(sora_amd, capi, torch, mcs, nframes, 0, 0)[0]
            variants["short"] = _tx_setup(sora_amd, capi, torch, mcs, nframes, 1, 0)[0]
        out["ms"] = _alternate(variants, 10 * reps, blocks, torch.cuda.synchronize)      # (a call is a fraction of a millisecond: ten times the calls per block)
    else:
        lead = 420 if row == "rx_raw" else 0
        sets = {}
        for name, gi in (("long", None), ("short", 1)):
            if gi is None or has_gi:
                _, o0, o1, slot, nsym = _tx_setup(sora_amd, capi, torch, mcs, nframes, gi, lead)
                sets[name] = (scale(o0), scale(o1), slot, nsym)
                del o0, o1
        nsym = sets["long"][3]
        out["data_symbols_per_frame"] = nsym
        rx = sora_amd.RxHt40(nframes, nframes * 2 * (nsym * 108 * nb + 64))
        if row == "rx_desc":
            variants = {}
            for name, (i0, i1, slot, _) in sets.items():
                d = sora_amd.RxHt40.frames([(f * slot + 1280, nb, cr | (SHORT if name == "short" else 0), MPDU + 4, MPDU + 4, 0, 0.0, f) for f in range(nframes)])
                variants[name] = (lambda i0=i0, i1=i1, d=d: rx.process_dev(i0, i1, d))
            check = {k: (v, 0) for k, v in variants.items()}
        else:
            variants, check = {}, {}
            for name, mode, which in (("long_mode_0", 0, "long"), ("long_mode_1", 1, "long"), ("short_mode_1", 1, "short")):
                if mode == 0 or has_gi:
                    i0, i1, slot, _ = sets[which]
                    caps = sora_amd.Rx.captures([(f * slot, slot, f) for f in range(nframes)])                  # packed once: the same set is submitted repeatedly
                    variants[name] = (lambda i0=i0, i1=i1, caps=caps: rx.process_captures_dev(i0, i1, caps, max_frames_per_capture=1))
                    check[name] = (variants[name], mode)
        # the variants alternate; a guard mode is switched between blocks (the switch waits for every call in flight: it is outside the timed window)
        res = {k: [] for k in variants}
        for k, call in variants.items():
            if has_gi:
                rx.set_guard(check[k][1])
            for _ in range(2):
                call()
            rx.synchronize()
        for _ in range(blocks):
            for k, call in variants.items():
                if has_gi:
                    rx.set_guard(check[k][1])
                t0 = time.perf_counter()
                for _ in range(reps):
                    call()
                rx.synchronize()
                res[k].append(round((time.perf_counter() - t0) * 1e3 / reps, 4))
        out["ms"] = res
        for k, (call, mode) in check.items():
            if has_gi:
                rx.set_guard(mode)
            call()
            rows = rx.results(with_mpdu=False)
            short = k.startswith("short")
            good = len(rows) == 2 * nframes and all(r["error_code"] == 1 and bool(r["flags"] & ROW_SHORT_GI) == short for r in rows)
            out.setdefault("all_frame_ok", {})[k] = good
            ok = ok and good
        rx.close()
    out["ms_min"] = {k: min(v) for k, v in out["ms"].items()}
    out["us_per_frame_min"] = {k: round(min(v) * 1e3 / nframes, 3) for k, v in out["ms"].items()}
    out["spread_pct"] = {k: round(100.0 * (max(v) - min(v)) / min(v), 2) for k, v in out["ms"].items()}
    return out, ok


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--row":                            # one row, in this process
        out, ok = bench(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5]), int(sys.argv[6]))
        print(json.dumps(out), flush=True)
        return 0 if ok else 2
    nframes = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    blocks = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    for mcs in (14, 8):
        for row in ("tx", "rx_desc", "rx_raw"):
            rc = subprocess.run(["timeout", "-k", "10", str(ROW_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--row", row, str(mcs), str(nframes), str(reps), str(blocks)]).returncode
            if rc != 0:
                print(json.dumps({"row": "ht40_gi_%s" % row, "mcs": mcs, "failed": rc}), flush=True)
                return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
