"""The 802.11b short preamble's price, in the manner of tools/bench_tx11b.py.
TX: 4096 frames x 1500-byte MPDU (1496 bytes + FCS) at 11 and 5.5 Mbps through sora_hip_tx11b_pre, short preamble beside long in one run (and
    sora_hip_tx11b itself beside both), hipEvents over back-to-back calls.
RX: (a) the shapes of bench.py's 802.11b rows -- one long-preamble frame per capture, 1 Mbps x 500 bytes and 11 Mbps x 1500 bytes, AWGN -- with
    sora_rx11b_set_preamble 1 beside 0 on one handle: what the option costs traffic that does not use it;
    (b) the same payloads behind the short preamble (2 Mbps x 500 bytes, 11 Mbps x 1500 bytes) at mode 1, beside their long-preamble twins at
    mode 1: ms per call, and ms per Msample of input, which is what compares batches of different air time.
Every RX figure is the median of `blocks` timed blocks of `calls` back-to-back calls (wall clock around process_dev ... synchronize), the variants
taken in turn inside every block round so that clock drift hits them alike; min and max over the blocks are printed beside it.
usage: python tools/bench_11b_short.py [ncaps [blocks]]   -> one JSON line per row"""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MPDU = 1496


def bench_tx(torch, sora_amd, rate, nframes=4096, reps=20):
    from sora_amd import capi
    L = capi.load()
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(rate)
    blob = torch.from_numpy(rng.integers(0, 256, MPDU).astype(np.uint8)).to(dev)
    moff = torch.zeros(nframes, dtype=torch.int32, device=dev)
    lens = torch.full((nframes,), MPDU, dtype=torch.int32, device=dev)
    rates = torch.full((nframes,), rate, dtype=torch.int32, device=dev)
    per = {k: sora_amd.tx11b_samples(MPDU, rate, k) for k in (0, 1)}
    out = torch.empty((nframes * per[0], 2), dtype=torch.int8, device=dev)
    row = {"row": "tx11b_short_vs_long", "rate_kbps": rate, "workload": "%d frames x %d-byte MPDU (+FCS) at %g Mbps" % (nframes, MPDU, rate / 1000), "reps": reps}
    variants = [("sora_hip_tx11b", None), ("pre_long", 0), ("pre_short", 1)]
    ms = {name: [] for name, _ in variants}
    for _ in range(3):                                                         # the variants in turn, three rounds
        for name, kind in variants:
            k = kind or 0
            ooff = torch.arange(nframes, dtype=torch.int64, device=dev) * per[k]
            kinds = torch.full((nframes,), k, dtype=torch.uint8, device=dev)
            tail = (None, None, nframes, capi._dev_ptr(out), capi._dev_ptr(ooff), capi._stream_ptr(None))
            if kind is None:
                call = lambda: L.sora_hip_tx11b(capi._dev_ptr(blob), capi._dev_ptr(moff), capi._dev_ptr(lens), capi._dev_ptr(rates), *tail)
            else:
                call = lambda: L.sora_hip_tx11b_pre(capi._dev_ptr(blob), capi._dev_ptr(moff), capi._dev_ptr(lens), capi._dev_ptr(rates), capi._dev_ptr(kinds), *tail)
            for _ in range(2):
                assert call() == 0
            e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(); e0.record()
            for _ in range(reps):
                call()
            e1.record(); torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1) / reps)
            assert bool(torch.equal(out[:per[k]], out[(nframes - 1) * per[k]:nframes * per[k]]))
    for name, kind in variants:
        n = per[kind or 0] * nframes
        row[name] = {"ms": round(statistics.median(ms[name]), 4), "ms_min_max": [round(min(ms[name]), 4), round(max(ms[name]), 4)], "samples": n,
                     "msamples_per_s": round(n / statistics.median(ms[name]) / 1e3, 1)}
    return row


def make_batch(torch, sora_amd, rate, mlen, kind, ncaps, dev):
    """ncaps captures of one frame each: 1200 samples of lead, the frame at gain 256, 2800 of tail, noise of sigma 40 added on the device"""
    w, _ = sora_amd.tx11b([np.random.default_rng(11).integers(0, 256, mlen).astype(np.uint8).tobytes()], [rate], preamble=kind)
    n = (len(w) + 1200 + 2800 + 27) // 28 * 28
    base = torch.zeros((n, 2), dtype=torch.float32, device=dev); base[1200:1200 + len(w)] = w.to(torch.float32) * 256.0
    gen = torch.Generator(device=dev); gen.manual_seed(1102)
    iq = torch.empty((ncaps, n, 2), dtype=torch.int16, device=dev)
    for i in range(0, ncaps, 64):
        k = min(64, ncaps - i)
        iq[i:i + k] = (base[None] + 40.0 * torch.randn((k, n, 2), generator=gen, device=dev)).round().clamp(-32768, 32767).to(torch.int16)
    return iq.view(-1, 2), sora_amd.Rx.captures([(i * n, n, i) for i in range(ncaps)]), n


def timed_blocks(rx, variants, blocks, calls):
    """variants: [(name, mode, flat, descs)] -> {name: [ms per call, per block]}"""
    out = {name: [] for name, *_ in variants}
    for _ in range(blocks + 1):                                                # (the first round warms up and is dropped)
        for name, mode, flat, descs in variants:
            rx.set_preamble(mode)
            rx.wait(rx.process_dev(flat, descs))
            t0 = time.perf_counter()
            for _ in range(calls):
                rx.process_dev(flat, descs)
            rx.synchronize()
            out[name].append((time.perf_counter() - t0) / calls * 1e3)
    return {k: v[1:] for k, v in out.items()}


def bench_rx(torch, sora_amd, ncaps, blocks, calls=8):
    dev = torch.device("cuda", 0)
    rows = []
    for rate_long, rate_short, mlen in ((1000, 2000, 500), (11000, 11000, 1500)):
        b_bench = make_batch(torch, sora_amd, rate_long, mlen, 0, ncaps, dev)          # bench.py's row shape
        b_long = b_bench if rate_long == rate_short else make_batch(torch, sora_amd, rate_short, mlen, 0, ncaps, dev)
        b_short = make_batch(torch, sora_amd, rate_short, mlen, 1, ncaps, dev)
        torch.cuda.synchronize()
        rx = sora_amd.Rx11b(ncaps, ncaps * max(b_bench[2], b_long[2], b_short[2]), max_frames_per_capture=4)
        ok = {}
        for name, mode, b in (("bench_long_mode0", 0, b_bench), ("bench_long_mode1", 1, b_bench), ("long_mode1", 1, b_long), ("short_mode1", 1, b_short), ("short_mode0", 0, b_short)):
            rx.set_preamble(mode)
            rx.process_dev(b[0], b[1])
            got = rx.results(with_mpdu=False)
            ok[name] = [sum(r["error_code"] == 1 for r in got), sum(r["error_code"] == 1 and r["flags"] == 2 for r in got)]
        ms = timed_blocks(rx, [("bench_long_mode0", 0, b_bench[0], b_bench[1]), ("bench_long_mode1", 1, b_bench[0], b_bench[1]),
                               ("long_mode1", 1, b_long[0], b_long[1]), ("short_mode1", 1, b_short[0], b_short[1])], blocks, calls)
        med = {k: statistics.median(v) for k, v in ms.items()}
        nsamp = {"bench_long_mode0": b_bench[2], "bench_long_mode1": b_bench[2], "long_mode1": b_long[2], "short_mode1": b_short[2]}
        row = {"row": "rx11b_preamble_mode", "captures": ncaps, "blocks": blocks, "calls_per_block": calls,
               "bench_batch": "%d captures x one %g Mbps frame, %d-byte MPDU, long preamble (%d samples each)" % (ncaps, rate_long / 1000, mlen, b_bench[2]),
               "short_batch": "the same payload at %g Mbps behind the short preamble (%d samples each); long_mode1 is its long-preamble twin (%d samples each)"
                              % (rate_short / 1000, b_short[2], b_long[2]),
               "frames_ok_and_flagged": ok}
        for k in ms:
            row[k] = {"ms": round(med[k], 3), "ms_min_max": [round(min(ms[k]), 3), round(max(ms[k]), 3)], "msamples_per_s": round(ncaps * nsamp[k] / med[k] / 1e3, 1),
                      "ms_per_gsample": round(med[k] / (ncaps * nsamp[k]) * 1e9, 3)}
        row["mode1_over_mode0_on_the_bench_batch"] = round(med["bench_long_mode1"] / med["bench_long_mode0"], 4)
        row["short_over_long_per_sample_at_mode1"] = round(row["short_mode1"]["ms_per_gsample"] / row["long_mode1"]["ms_per_gsample"], 4)
        rows.append(row)
        rx.synchronize(); rx.close()
        del b_bench, b_long, b_short
        torch.cuda.empty_cache()
    return rows


def main():
    import torch
    import sora_amd
    ncaps = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
    blocks = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    for rate in (11000, 5500):
        print(json.dumps(bench_tx(torch, sora_amd, rate)), flush=True)
    good = True
    for row in bench_rx(torch, sora_amd, ncaps, blocks):
        f = row["frames_ok_and_flagged"]
        good &= f["short_mode1"][1] >= 0.95 * ncaps and f["short_mode0"][0] == 0 and f["bench_long_mode1"] == f["bench_long_mode0"]
        print(json.dumps(row), flush=True)
    return 0 if good else 1


if __name__ == "__main__":
    sys.exit(main())
