"""The front-end stages of the 802.11a receive graph (sora_amd/csrc/k_11a.hip) on one GPU, by the method of tools/bench_11n_rx_stages.py: 8192 streams / frames per
call, two buffer sets in rotation, device events after a warm-up.  Nothing here is a gate.

  carrier_sense11a, cca11a   8192 noise streams (sigma 30: no detection, a time-out every 21 bursts that stands -- flags 0) of 2048 bursts, walked to the end, beside
                             cca11n on two such chains (SORA_CCA11N_REARM, so that it too walks all 2048) IN THE SAME RUN; ns per burst and stream-bursts per second
  data_symbol11a, dc_remove11a   as a share of benchlib.common.HBM_PEAK (algorithmic bytes: input + output), beside fft64 on data_symbol11a's output
  viterbi_sig11a, plcp_parse11a, dc_estimate11a   microseconds per call (8192 SIGNAL symbols / words; 8192 streams of 2048 bursts)
Composition row: sora_amd.rx11a_by_stages (host wall clock: it reads counts and records back every round) against Rx.process_dev + wait on the same batch, the first 512
captures of tests/scan_captures.lead_sweep (one 20-byte 54 Mbps frame behind 0 .. 511 raw samples), every event compared.
usage: python tools/bench_11a_rx_stages.py [--streams N] [--chain-captures N] [--reps R] [--out profiles/11a_rx_stages.json]   -> one JSON line per row, the record in the file"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def bench_stages(torch, dev, ns, reps, nsets=2):
    from bench_11n_rx_stages import kernel_resources
    from benchlib.common import HBM_PEAK
    from sora_amd import capi
    import rx11a_stage_model as model
    L = capi.load(); P = capi._dev_ptr; st = capi._stream_ptr(None)
    g = torch.Generator(device=dev); g.manual_seed(11)
    rows = {}

    def timed(label, fns, nbytes, r=reps, extra=None):
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
        rows[label].update(extra(ms) if extra else {})
        print(json.dumps({"row": label, **rows[label]}), flush=True)

    ar = torch.arange(ns, device=dev, dtype=torch.int64)
    tab = lambda per: (ar * per).to(torch.int32).contiguous()
    full = lambda v: torch.full((ns,), v, dtype=torch.int32, device=dev)
    nbur = 2048
    per_burst = lambda ms: {"bursts_per_stream": nbur, "ns_per_burst_of_one_stream": round(1e6 * ms / nbur, 2), "stream_bursts_per_s": round(ns * nbur / (ms * 1e-3))}
    # ---- the carrier-sense bricks on noise
    noise = [(torch.randn((ns * nbur * 4, 2), device=dev, generator=g) * 30.0).round().to(torch.int16) for _ in range(nsets)]
    fb, nb_ = tab(4 * nbur), full(nbur)
    used = torch.zeros(ns, dtype=torch.int32, device=dev); npass = torch.zeros_like(used)
    fresh_cs = torch.from_numpy(capi.cs11a_states(ns)).to(dev); fresh_cca = fresh_cs[:, :capi.CCA11A_WORDS].contiguous()
    s_cs = [fresh_cs.clone() for _ in range(nsets)]; s_cca = [fresh_cca.clone() for _ in range(nsets)]
    gated = torch.empty((ns * nbur * 4, 2), dtype=torch.int16, device=dev); ob = tab(nbur)

    def cs(x, s):
        s.copy_(fresh_cs)                                                        # (a constructed record each time; counted in the bytes)
        return L.sora_hip_carrier_sense11a(P(x), P(fb), P(nb_), P(s), P(used), ns, nbur, 0, st)

    def cca(x, s):
        s.copy_(fresh_cca)
        return L.sora_hip_cca11a(P(x), P(fb), P(nb_), P(ob), P(s), P(gated), P(used), P(npass), ns, nbur, 0, st)

    timed("carrier_sense11a", [(lambda x=x, s=s: cs(x, s)) for x, s in zip(noise, s_cs)], ns * (nbur * 16 + 3 * 192), extra=per_burst)
    h = noise[0][:4 * nbur].cpu().numpy()
    w_state, w_used = model.carrier_sense(h, capi.cs11a_states(1)[0], 0)
    cs(noise[0], s_cs[0]); torch.cuda.synchronize()
    rows["carrier_sense11a"].update({"equals_the_model": bool(used[0].item() == w_used and (s_cs[0][0].cpu().numpy() == w_state).all()),
                                     "kernel": kernel_resources("k_11a_carrier_sense"), "note": "the time includes the copy that re-arms the records"})
    timed("cca11a", [(lambda x=x, s=s: cca(x, s)) for x, s in zip(noise, s_cca)], ns * (nbur * 32 + 3 * 176), extra=per_burst)
    rows["cca11a"].update({"kernel": kernel_resources("k_11a_cca"), "note": "every burst of a noise stream passes the gate: the output is a copy of the input"})
    fresh_n = torch.from_numpy(capi.cca11n_states(ns)).to(dev); s_n = [fresh_n.clone() for _ in range(nsets)]

    def cca_n(s):
        s.copy_(fresh_n)
        return L.sora_hip_cca11n(P(noise[0]), P(noise[1 % nsets]), P(fb), P(nb_), P(s), P(used), ns, nbur, capi.CCA11N_REARM, st)

    timed("cca11n", [(lambda s=s: cca_n(s)) for s in s_n], ns * (nbur * 32 + 3 * 1056), extra=per_burst)
    rows["cca11n"].update({"kernel": kernel_resources("k_cca11n"), "note": "two chains; the same noise streams, re-armed at each time-out"})
    # ---- TDCEstimator, TDCRemoveEx on the same streams
    s_dc = torch.from_numpy(capi.dcest11a_states(ns)).to(dev)
    timed("dc_estimate11a", [(lambda x=x: L.sora_hip_dc_estimate11a(P(x), P(fb), P(nb_), P(s_dc), ns, nbur, st)) for x in noise], ns * nbur * 16)
    dc = torch.randint(-300, 300, (ns, 2), dtype=torch.int16, device=dev, generator=g)
    timed("dc_remove11a", [(lambda x=x: L.sora_hip_dc_remove11a(P(x), P(fb), P(nb_), P(fb), P(dc), P(gated), ns, nbur, st)) for x in noise], ns * nbur * 32)
    del noise, gated
    # ---- T11aDataSymbol on a 1500-byte 54 Mbps frame's worth (57 symbols), and TFFT64 on what it writes
    nsym = 57
    x = [torch.randint(-9000, 9000, (ns * nsym * 80, 2), dtype=torch.int16, device=dev, generator=g) for _ in range(nsets)]
    y = [torch.empty((ns * nsym * 64, 2), dtype=torch.int16, device=dev) for _ in range(nsets)]
    f80, nn, o1 = tab(nsym * 80), full(nsym), tab(nsym)
    timed("data_symbol11a", [(lambda a=a, b=b: L.sora_hip_data_symbol11a(P(a), P(f80), P(nn), P(o1), P(b), ns, nsym, st)) for a, b in zip(x, y)], ns * nsym * (80 + 64) * 4)
    z = torch.empty_like(y[0])
    timed("fft64", [(lambda a=a: L.sora_hip_fft64(P(a), P(z), ns * nsym, st)) for a in y], ns * nsym * 64 * 4 * 2)
    del x, y, z
    # ---- T11aViterbiSig, T11aPLCPParser
    soft = torch.randint(0, 8, (ns, 48), dtype=torch.uint8, device=dev, generator=g); sig = torch.zeros(ns, dtype=torch.int32, device=dev)
    rec = torch.zeros((ns, 5), dtype=torch.int32, device=dev)
    timed("viterbi_sig11a", [lambda: L.sora_hip_viterbi_sig11a(P(soft), P(sig), ns, st)], ns * 52)
    timed("plcp_parse11a", [lambda: L.sora_hip_plcp_parse11a(P(sig), P(rec), ns, st)], ns * 24)
    return rows


def bench_chain(torch, sora, dev, ncaps, reps=3):
    import time
    import rx11a_stage_cases as cases
    import scan_captures as sc
    from gpu_util import batch
    from oracle.pyoracle import Oracle
    caps = sc.lead_sweep(Oracle())[:ncaps]
    iq, descs = batch(caps)
    iq = np.concatenate([iq, np.zeros(((-len(iq)) % 8, 2), np.int16)])
    d_iq = torch.from_numpy(iq).to(dev)
    rx = sora.Rx(len(caps), len(iq), sample_rate_mhz=40, max_frames_per_capture=8)
    rows = rx.results(ticket=rx.process_dev(d_iq, descs))
    t = []
    for _ in range(reps):
        torch.cuda.synchronize(); t0 = time.perf_counter(); ev = sora.rx11a_by_stages(d_iq, [(o, n) for o, n, _ in descs]); t.append(time.perf_counter() - t0)
    equal = all(cases.same_events(ev[k], [r for r in rows if r["capture_id"] == k]) is None for k in range(len(caps)))
    h = []
    for _ in range(reps + 2):
        torch.cuda.synchronize(); t0 = time.perf_counter(); tk = rx.process_dev(d_iq, descs); rx.wait(tk); h.append(time.perf_counter() - t0)
    rx.close()
    out = {"workload": "%d captures of tests/scan_captures.lead_sweep: one 20-byte 54 Mbps frame each" % len(caps), "events": len(rows),
           "every_event_equals_the_handles": bool(equal), "by_stages_ms": round(1e3 * float(np.median(t)), 1), "handle_ms": round(1e3 * float(np.median(h[2:])), 2)}
    out["by_stages_over_handle"] = round(out["by_stages_ms"] / out["handle_ms"], 1)
    print(json.dumps({"row": "chain", **out}), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=8192)
    ap.add_argument("--chain-captures", type=int, default=512)
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "11a_rx_stages.json"))
    a = ap.parse_args()
    import torch
    dev = torch.device("cuda", 0)
    rec = {"tool": "tools/bench_11a_rx_stages.py", "parent_commit": "c44f63e", "device": torch.cuda.get_device_name(0), "streams": a.streams, "reps": a.reps,
           "stages": bench_stages(torch, dev, a.streams, a.reps)}
    torch.cuda.empty_cache()
    import sora_amd
    rec["chain"] = bench_chain(torch, sora_amd, dev, a.chain_captures)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")
    return 0 if rec["stages"]["carrier_sense11a"]["equals_the_model"] and rec["chain"]["every_event_equals_the_handles"] else 1


if __name__ == "__main__":
    sys.exit(main())
