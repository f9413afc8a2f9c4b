"""Stream mode of the 802.11b receive graph (sora_rx11b_set_stream_mode) against the same samples in plain calls.  The 11b bench batch's
capture (benchlib.rows.bench_11b: one 1 Mbps frame, AWGN) is repeated into STREAMS long streams on the device; PIECE samples of every
stream 'arrive' per call, and the call carries one capture per stream: from where the stream's last call left it (its resume point) to
what has arrived -- a frame cut by a piece is decoded again by the next call, and a frame longer than a piece makes the host's tail grow.
The plain row feeds the same streams in back-to-back pieces of PIECE samples with the mode off (frames cut by a piece are lost there); the
same_captures_mode_off row replays the stream row's captures, call for call, with the mode off: the cost of stream mode itself.
One call in flight in every row (stream mode runs its calls one after the other).  Reports ms per call and the rate in input samples per
second; the stream row also the rate of stream progress (consumed samples), frames reported, and whether that is every frame.
usage: python tools/bench_stream11b.py [--streams 4096] [--piece-calls 2048] [--reps 2]   -> one JSON line"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--piece-calls", type=int, default=2048, help="source calls (28 samples) per piece")
    ap.add_argument("--reps", type=int, default=2, help="captures of the bench batch per stream")
    a = ap.parse_args()
    import torch
    import sora_amd
    from oracle.pyoracle import ReferenceGraph
    dev = torch.device("cuda", 0)
    g = ReferenceGraph()
    if g.available():
        s8 = g.tx11b(np.random.default_rng(11).integers(0, 256, 500).astype(np.uint8).tobytes(), 1000); what = "500-byte MPDU"
    else:
        s8 = np.load(os.path.join(ROOT, "tests", "golden", "refgraph_11b.npz"))["tx_2"]; what = "40-byte MPDU (recorded modulator output)"
    n = (len(s8) + 1200 + 2800 + 27) // 28 * 28                        # the bench batch's capture
    base = np.zeros((n, 2), np.int16); base[1200:1200 + len(s8)] = s8.astype(np.int16) << 8
    L = n * a.reps
    L4 = L + 28 * 4                                                     # a quiet tail: the last frame's Seek ends inside the stream
    b = torch.from_numpy(np.concatenate([base] * a.reps + [np.zeros((L4 - L, 2), np.int16)])).to(dev).to(torch.float32)
    gen = torch.Generator(device=dev); gen.manual_seed(1102)
    iq = torch.empty((a.streams, L4, 2), dtype=torch.int16, device=dev)
    for i in range(0, a.streams, 16):
        k = min(16, a.streams - i)
        iq[i:i + k] = (b[None] + 40.0 * torch.randn((k, L4, 2), generator=gen, device=dev)).round().clamp(-32768, 32767).to(torch.int16)
    flat = iq.view(-1, 2)
    piece = 28 * a.piece_calls
    torch.cuda.synchronize()
    out = {"workload": "%d streams x %d captures of one 1 Mbps frame (%s, %d samples @44 MHz each), AWGN, pieces of %d samples" % (a.streams, a.reps, what, n, piece)}

    def replay(calls):
        """the stream row's captures, call by call, with the mode off: what stream mode itself costs"""
        rx = sora_amd.Rx11b(a.streams, a.streams * L4, max_frames_per_capture=4)
        t_ms = 0.0; submitted = 0
        for descs in calls:
            d = sora_amd.Rx.captures(descs)
            t0 = time.perf_counter()
            rx.wait(rx.process_dev(flat, d))
            t_ms += (time.perf_counter() - t0) * 1e3
            submitted += sum(x[1] for x in descs)
        rx.close()
        return {"calls": len(calls), "ms_per_call": round(t_ms / len(calls), 3), "msamples_per_s": round(submitted / t_ms / 1e3, 1)}

    def run(stream_mode, record=None):
        rx = sora_amd.Rx11b(a.streams, a.streams * L4, max_frames_per_capture=4)
        rx.set_stream_mode(1 if stream_mode else 0)
        pos = [0] * a.streams; arrived = [0] * a.streams
        calls = frames = submitted = 0
        t_ms = 0.0
        while True:
            descs = []
            for k in range(a.streams):
                arrived[k] = min(L4, max(arrived[k], pos[k]) + piece)
                m = (arrived[k] - pos[k]) // 28 * 28
                descs.append((k * L4 + pos[k], m, k))
            if not any(d[1] for d in descs):
                break
            d = sora_amd.Rx.captures(descs)
            if record is not None:
                record.append(descs)
            t0 = time.perf_counter()
            rx.wait(rx.process_dev(flat, d))
            t_ms += (time.perf_counter() - t0) * 1e3
            rows = rx.results(with_mpdu=False)
            frames += sum(r["error_code"] == 1 for r in rows)
            submitted += sum(x[1] for x in descs); calls += 1
            used = rx.stream_consumed(rx.ticket(), a.streams) if stream_mode else [x[1] for x in descs]
            stuck = all(int(u) == 0 for u, x in zip(used, descs) if x[1]) and all(v == L4 for v in arrived)      # (nothing more to come)
            for k in range(a.streams):
                pos[k] += int(used[k])
            if stream_mode and stuck:
                break
        rx.close()
        return {"calls": calls, "ms_per_call": round(t_ms / calls, 3), "msamples_per_s": round(submitted / t_ms / 1e3, 1),
                "stream_msamples_per_s": round(sum(pos) / t_ms / 1e3, 1), "frames_ok": frames, "frames_sent": a.streams * a.reps}

    run(True)                                                           # warm-up (code objects, allocations)
    calls = []
    out["stream"] = run(True, calls)
    out["same_captures_mode_off"] = replay(calls)
    out["plain"] = run(False)
    out["stream"]["every_frame"] = out["stream"]["frames_ok"] == out["stream"]["frames_sent"]
    out["stream_vs_mode_off_per_sample"] = round(out["stream"]["msamples_per_s"] / out["same_captures_mode_off"]["msamples_per_s"], 3)
    out["stream_progress_vs_plain"] = round(out["stream"]["stream_msamples_per_s"] / out["plain"]["msamples_per_s"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
