"""MCS 15 (64-QAM, rate 5/6) of the 40 MHz HT 2x2 pair (sora_hip_tx_ht40_mcs, sora_ht40_set_mcs_max, k_viterbi56_11n) beside MCS 14, one run on one
box: 4096 per-stream frames of 2 x 1500-byte PSDUs per call, as four rows, each in a process of its own under `timeout -k 10`:
  tx        the transmitter: sora_hip_tx_ht40_gi at MCS 14 (what the parent has), sora_hip_tx_ht40_mcs with the gate at 15 at MCS 14 and at MCS 15; wall clock over
            10 x reps back-to-back calls, then a synchronize;
  rx_desc   the descriptor form of the receiver on what the transmitter sent (identity channel at the level the receiver's tests use, zero forcing): MCS 14 on a default
            handle, MCS 14 and MCS 15 on a handle whose gate is 15; back-to-back sora_ht40_process_dev calls, eight in flight, then a synchronize;
  rx_raw    the raw-capture form, one frame per capture, the same three variants; on the gate-15 handle every call launches k_viterbi56_11n, at MCS 14 over an empty list:
            the difference between the two MCS 14 variants is what that launch costs;
  trellis   the 5/6 kernel alone (sora_hip_viterbi56_11n) beside k_viterbi11n at rate 3/4 (sora_hip_viterbi11n_ws, 64 lanes per pair), 4096 jobs of a 1500-byte frame of
            random soft values each: ms per call and ns per trellis step and job.  Both are 64-lane pair kernels with the same add-compare-select work per step.  The 3/4 stage
            copies the soft bytes into its workspace first; that copy is timed alone beside it and subtracted for an estimate of k_viterbi11n by itself.
Within a row the variants ALTERNATE, block after block of `reps` calls, `blocks` times, after a warm-up block that is dropped: every figure is the list of its blocks' means
(ms per call).  Every receive variant's last call is checked: all rows FRAME_OK at the MCS that was sent.
--parent DIR: a checkout of the parent commit with its library built (it has no MCS 15): each row's MCS 14 default variants are run again from DIR, in the same run, so
that the default handle's cost on this commit and on the parent stand side by side.
usage: python tools/bench_ht40_mcs15.py [frames] [reps] [blocks] [--parent DIR]   -> one JSON line per row and tree"""
import json
import os
import subprocess
import sys
import time

ROOT = os.environ.get("SORA_BENCH_ROOT") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ROW_TIMEOUT_S = 400
GAIN = 250.0 * 128.0 / 16384.0        # tests/test_gpu_tx_ht40.py: the level at which the receiver's own tests decode
GEOM = {14: (6, 2), 15: (6, 3)}       # MCS -> (N_BPSC, code rate)
MPDU = 1496                           # + FCS = 1500-byte PSDUs, one per stream


def _alternate(variants, reps, blocks, sync):
    """variants: {name: call} -> {name: [ms per call of each block]}; alternating, the first block dropped"""
    out = {k: [] for k in variants}
    for b in range(blocks + 1):
        for k, call in variants.items():
            t0 = time.perf_counter()
            for _ in range(reps):
                call()
            sync()
            if b:
                out[k].append(round((time.perf_counter() - t0) * 1e3 / reps, 4))
    return out


def _tx_setup(sora_amd, capi, torch, mcs, nframes, gate, lead):
    """-> (call, out0, out1, samples per frame slot, nsym).  gate None: sora_hip_tx_ht40_gi with every kind 0; else sora_hip_tx_ht40_mcs with that gate"""
    dev = torch.device("cuda")
    L = capi.load()
    per = sora_amd.tx_ht40_gi_samples(MPDU, mcs, 0) if gate is None else sora_amd.tx_ht40_samples(MPDU, mcs, gate, 0)
    assert per, (mcs, gate)
    nsym = (per - 1600) // 160
    slot = lead + per
    slot += -slot % 28                                                        # raw captures are whole 28-sample source bursts
    lens = torch.full((nframes,), MPDU, dtype=torch.int32, device=dev); mcsv = torch.full((nframes,), mcs, dtype=torch.int32, device=dev)
    moff = torch.arange(2 * nframes, dtype=torch.int32, device=dev) * MPDU
    blob = torch.randint(0, 256, (2 * nframes * MPDU,), dtype=torch.uint8, generator=torch.Generator(device=dev).manual_seed(1), device=dev)
    ooff = torch.arange(nframes, dtype=torch.int64, device=dev) * slot + lead
    out0 = torch.zeros((nframes * slot + 256, 2), dtype=torch.int16, device=dev); out1 = torch.zeros_like(out0)
    kinds = torch.zeros((nframes,), dtype=torch.uint8, device=dev)
    p = capi._dev_ptr
    if gate is None:
        call = lambda: L.sora_hip_tx_ht40_gi(p(blob), p(moff), p(lens), p(mcsv), None, p(kinds), nframes, p(out0), p(out1), p(ooff), None)
    else:
        call = lambda: L.sora_hip_tx_ht40_mcs(p(blob), p(moff), p(lens), p(mcsv), None, p(kinds), nframes, p(out0), p(out1), p(ooff), gate, None)
    call.keep = (lens, mcsv, moff, blob, ooff, kinds)
    assert call() == 0
    torch.cuda.synchronize()
    return call, out0, out1, slot, nsym


def bench(row, nframes, reps, blocks):
    import torch
    import sora_amd
    from sora_amd import capi
    has = hasattr(sora_amd.RxHt40, "set_mcs_max")
    scale = lambda o: torch.clamp(torch.round(o.float() * GAIN), -32768, 32767).to(torch.int16)
    out = {"row": "ht40_mcs15_%s" % row, "tree": ROOT, "frames": nframes, "psdu_bytes_per_frame": 2 * (MPDU + 4), "reps": reps, "blocks": blocks, "mcs15_present": has}
    ok = True
    # (name, MCS, the transmitter's gate, the handle's gate)
    plan = [("mcs14_default", 14, None, 14)] + ([("mcs14_gate15", 14, 15, 15), ("mcs15_gate15", 15, 15, 15)] if has else [])
    if row == "tx":
        out["ms"] = _alternate({name: _tx_setup(sora_amd, capi, torch, mcs, nframes, gate, 0)[0] for name, mcs, gate, _ in plan}, 10 * reps, blocks, torch.cuda.synchronize)
    elif row == "trellis":
        dev = torch.device("cuda")
        steps = 8 * (MPDU + 4) + 22
        gen = torch.Generator(device=dev).manual_seed(2)
        lens = torch.full((nframes,), MPDU + 4, dtype=torch.int16, device=dev)
        n34 = -(-steps // 3) * 4
        soft34 = torch.randint(0, 8, (nframes * n34 + 64,), dtype=torch.uint8, generator=gen, device=dev)
        off34 = (torch.arange(nframes, dtype=torch.int32, device=dev) * n34).contiguous(); ns34 = torch.full((nframes,), n34, dtype=torch.int32, device=dev)
        ws = torch.empty(sora_amd.viterbi11n_workspace_bytes(soft34.numel(), nframes), dtype=torch.uint8, device=dev)
        o34 = torch.zeros((nframes, 1536), dtype=torch.uint8, device=dev); oo = (torch.arange(nframes, dtype=torch.int32, device=dev) * 1536).contiguous()
        variants = {"k_viterbi11n_rate34": lambda: sora_amd.viterbi11n_ws(soft34, off34, ns34, lens, 2, ws, out=o34, out_off=oo, lanes_per_pair=64)}
        # what that stage does in front of its kernel and the other one does not: a device-to-device copy of the soft bytes into the workspace (its job-table kernel, one
        # thread per job, is not separated).  Timed alone, so that the difference can be read as k_viterbi11n by itself
        stage_copy = ws[:soft34.numel()]
        variants["soft_copy_alone"] = lambda: stage_copy.copy_(soft34)
        if has:
            n56 = -(-steps // 5) * 6
            soft56 = torch.randint(0, 8, (nframes * n56 + 64,), dtype=torch.uint8, generator=gen, device=dev)
            off56 = (torch.arange(nframes, dtype=torch.int32, device=dev) * n56).contiguous(); ns56 = torch.full((nframes,), n56, dtype=torch.int32, device=dev)
            o56 = torch.zeros((nframes, 1536), dtype=torch.uint8, device=dev)
            variants["k_viterbi56_11n_rate56"] = lambda: sora_amd.viterbi56_11n(soft56, off56, ns56, lens, out=o56, out_off=oo)
        out["ms"] = _alternate(variants, reps, blocks, torch.cuda.synchronize)
        out["trellis_steps_per_job"] = steps
        out["note"] = ("k_viterbi11n_rate34 includes the stage's copy of the soft bytes into its workspace (soft_copy_alone) and its job-table kernel: "
                       "k_viterbi11n_alone_estimate is the stage's minimum less the copy's")
        out["ns_per_step_and_job_min"] = {k: round(min(v) * 1e6 / (nframes * steps), 4) for k, v in out["ms"].items() if k != "soft_copy_alone"}
        alone = min(out["ms"]["k_viterbi11n_rate34"]) - min(out["ms"]["soft_copy_alone"])
        out["ns_per_step_and_job_min"]["k_viterbi11n_alone_estimate"] = round(alone * 1e6 / (nframes * steps), 4)
    else:
        lead = 420 if row == "rx_raw" else 0
        handles, variants, gates = {}, {}, {}
        for name, mcs, txgate, rxgate in plan:
            nb, cr = GEOM[mcs]
            _, o0, o1, slot, nsym = _tx_setup(sora_amd, capi, torch, mcs, nframes, txgate, lead)
            i0, i1 = scale(o0), scale(o1)
            del o0, o1
            if rxgate not in handles:
                handles[rxgate] = sora_amd.RxHt40(nframes, nframes * 2 * (25 * 108 * 6 + 64))          # MCS 14's 25 symbols (MCS 15: 23): room for either
                if rxgate != 14:
                    handles[rxgate].set_mcs_max(rxgate)
            rx = handles[rxgate]
            if row == "rx_desc":
                d = sora_amd.RxHt40.frames([(f * slot + 1280, nb, cr, MPDU + 4, MPDU + 4, 0, 0.0, f) for f in range(nframes)])
                variants[name] = (lambda rx=rx, i0=i0, i1=i1, d=d: rx.process_dev(i0, i1, d))
            else:
                caps = sora_amd.Rx.captures([(f * slot, slot, f) for f in range(nframes)])                  # packed once: the same set is submitted repeatedly
                variants[name] = (lambda rx=rx, i0=i0, i1=i1, caps=caps: rx.process_captures_dev(i0, i1, caps, max_frames_per_capture=1))
            gates[name] = (rx, mcs, nsym)
        sync = lambda: [h.synchronize() for h in handles.values()]
        out["ms"] = _alternate(variants, reps, blocks, sync)
        out["data_symbols_per_frame"] = {k: v[2] for k, v in gates.items()}
        for k, call in variants.items():
            rx, mcs, _ = gates[k]
            call()
            rows = rx.results(with_mpdu=False)
            want = mcs if row == "rx_raw" else 10 * GEOM[mcs][0] + GEOM[mcs][1]
            good = len(rows) == 2 * nframes and all(r["error_code"] == 1 and r["rate_kbps"] == want for r in rows)
            out.setdefault("all_frame_ok", {})[k] = good
            ok = ok and good
        for h in handles.values():
            h.close()
    out["ms_min"] = {k: min(v) for k, v in out["ms"].items()}
    out["us_per_frame_min"] = {k: round(min(v) * 1e3 / nframes, 3) for k, v in out["ms"].items()}
    out["spread_pct"] = {k: round(100.0 * (max(v) - min(v)) / min(v), 2) for k, v in out["ms"].items()}
    return out, ok


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--row":                            # one row, in this process
        out, ok = bench(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5]))
        print(json.dumps(out), flush=True)
        return 0 if ok else 2
    args = sys.argv[1:]
    parent = None
    if "--parent" in args:
        i = args.index("--parent"); parent = os.path.abspath(args[i + 1]); del args[i:i + 2]
    nframes = int(args[0]) if len(args) > 0 else 4096
    reps = int(args[1]) if len(args) > 1 else 10
    blocks = int(args[2]) if len(args) > 2 else 5
    for row in ("tx", "rx_desc", "rx_raw", "trellis"):
        for tree in [None] + ([parent] if parent else []):
            env = dict(os.environ, **({"SORA_BENCH_ROOT": tree} if tree else {}))
            rc = subprocess.run(["timeout", "-k", "10", str(ROW_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--row", row, str(nframes), str(reps), str(blocks)],
                                env=env, cwd=tree or ROOT).returncode
            if rc != 0:
                print(json.dumps({"row": "ht40_mcs15_%s" % row, "tree": tree or ROOT, "failed": rc}), flush=True)
                return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
