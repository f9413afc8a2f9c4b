"""Stream mode of the 44 MHz 802.11a graph (sora_rx_set_stream_mode with sample_rate_mhz = 44) against the same captures with the mode off.
One 44 MHz capture -- a 500-byte 24 Mbps frame with quiet on either side, padded to whole 308-sample periods of TDownSample44_40 -- is
repeated REPS times into STREAMS streams, with AWGN of its own in every stream, and ingested to the 40 MHz stream outside the timed region.
Call j carries capture j of every stream.  In stream mode it continues call j - 1 (the pieces are frame-aligned, so every capture ends at a
resume point and is consumed whole); with the mode off the same captures are independent.  One call in flight; the two modes alternate
ROUNDS times in one run.  Reports ms per call, input samples per second and frames reported, per mode, and the per-sample cost of the mode.
usage: python tools/bench_stream44.py [--streams 4096] [--reps 4] [--rounds 3]   -> one JSON line"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=4, help="captures (calls) per stream")
    ap.add_argument("--rounds", type=int, default=3, help="times the two modes alternate")
    a = ap.parse_args()
    import torch
    import sora_amd
    from oracle.pyoracle import Oracle
    from gpu_util import upsample_40_to_44
    dev = torch.device("cuda", 0)
    o = Oracle()
    mp = np.random.default_rng(44).integers(0, 256, 500).astype(np.uint8).tobytes()
    c44 = upsample_40_to_44(o.tx_capture(mp, 24000, seed=0x5D, lead=1200, tail=1600))
    c44 = np.concatenate([c44, np.zeros(((-len(c44)) % 308, 2), np.int16)])
    x40 = sora_amd.ingest(torch.from_numpy(c44).to(dev), sora_amd.INGEST_44TO40)
    n = x40.shape[0]                                                     # 280 resampled samples per 308 source samples
    assert n == len(c44) // 308 * 280
    L = n * a.reps
    base = x40.to(torch.float32).repeat(a.reps, 1)
    gen = torch.Generator(device=dev); gen.manual_seed(4404)
    iq = torch.empty((a.streams, L, 2), dtype=torch.int16, device=dev)
    for i in range(0, a.streams, 64):
        k = min(64, a.streams - i)
        iq[i:i + k] = (base[None] + 40.0 * torch.randn((k, L, 2), generator=gen, device=dev)).round().clamp(-32768, 32767).to(torch.int16)
    flat = iq.view(-1, 2)
    torch.cuda.synchronize()
    calls = [sora_amd.Rx.captures([(k * L + j * n, n, k) for k in range(a.streams)]) for j in range(a.reps)]
    rx = {m: sora_amd.Rx(a.streams, a.streams * n, sample_rate_mhz=44, max_frames_per_capture=4) for m in (0, 1)}
    rx[1].set_stream_mode(1)

    def run(mode):
        r = rx[mode]
        if mode:
            r.reset()                                                    # every stream from its start
        t_ms = 0.0; frames = 0; whole = True
        for d in calls:
            t0 = time.perf_counter()
            r.wait(r.process_dev(flat, d))
            t_ms += (time.perf_counter() - t0) * 1e3
            frames += sum(x["error_code"] == 1 for x in r.results(with_mpdu=False))
            if mode:
                whole &= bool(np.all(r.stream_consumed(r.ticket(), a.streams) == n))
        return t_ms, frames, whole

    run(1); run(0)                                                       # warm-up (code objects, allocations)
    acc = {0: [], 1: []}; fr = {}; whole = True
    for _ in range(a.rounds):
        for m in (1, 0):
            t, f, w = run(m)
            acc[m].append(t); fr[m] = f; whole &= w
    samples = a.streams * L
    out = {"workload": "%d streams x %d captures of one 500-byte 24 Mbps frame (%d samples @44 MHz, %d resampled each), AWGN, one call in flight"
                       % (a.streams, a.reps, len(c44), n)}
    for m, name in ((1, "stream"), (0, "mode_off")):
        best = min(acc[m])
        out[name] = {"ms_per_call": round(best / a.reps, 3), "ms_per_call_rounds": [round(t / a.reps, 3) for t in acc[m]],
                     "msamples_per_s": round(samples / best / 1e3, 1), "frames_ok": fr[m], "frames_sent": a.streams * a.reps}
    out["stream"]["every_capture_consumed_whole"] = whole
    out["stream_cost_per_sample"] = round(min(acc[1]) / min(acc[0]) - 1.0, 3)
    for r in rx.values():
        r.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
