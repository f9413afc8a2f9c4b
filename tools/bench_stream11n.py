"""Stream mode of the 802.11n 2x2 receive graph (sora_rx11n_set_stream_mode) against the same samples in plain calls.  One two-chain capture
(one MCS 9 frame, AWGN, a gap of quiet on either side) is repeated into STREAMS long two-chain streams on the device; PIECE samples of every
stream 'arrive' per call, and the call carries one capture per stream: from where the stream's last call left it (its resume point) to what
has arrived -- a frame cut by a piece is decoded again by the next call, and a frame longer than a piece makes the host's tail grow.
The plain row feeds the same streams in back-to-back pieces of PIECE samples with the mode off (frames cut by a piece are lost there, or
reported from zero padding); the same_captures_mode_off row replays the stream row's captures, call for call, with the mode off (a capture that starts at a
resume point inside a preamble finds nothing there, so this row does less work); the *_aligned rows do the same with pieces of exactly one
frame period, cut in the quiet gaps, where both modes decode the same frames: the cost of stream mode itself.  One call in flight in every row (stream mode runs its calls one after the other).  Reports ms per call and the rate in
input samples per second (per chain); the stream row also the rate of stream progress (consumed samples), frames reported, and whether that
is every frame.
usage: python tools/bench_stream11n.py [--streams 2048] [--piece-calls 256] [--reps 4]   -> one JSON line"""
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
    ap.add_argument("--streams", type=int, default=2048)
    ap.add_argument("--piece-calls", type=int, default=256, help="source calls (28 samples) per piece")
    ap.add_argument("--reps", type=int, default=4, help="frames per stream")
    a = ap.parse_args()
    import torch
    import sora_amd
    from oracle.pyoracle import ReferenceGraph
    dev = torch.device("cuda", 0)
    g = ReferenceGraph()
    if g.available():
        s0, s1 = g.tx11n(np.random.default_rng(11).integers(0, 256, 500).astype(np.uint8).tobytes(), 9); what = "500-byte MPDU"
    else:
        s0, s1, _ = sora_amd.tx11n([np.random.default_rng(11).integers(0, 256, 500).astype(np.uint8).tobytes()], [9])
        s0, s1 = s0.cpu().numpy(), s1.cpu().numpy(); what = "500-byte MPDU (GPU modulator)"
    n = (len(s0) + 1200 + 2800 + 27) // 28 * 28                        # one frame and its gaps
    base = np.zeros((2, n, 2), np.int16); base[0, 1200:1200 + len(s0)] = s0; base[1, 1200:1200 + len(s1)] = s1
    L = n * a.reps
    L4 = L + 28 * 8                                                     # a quiet tail
    b = torch.from_numpy(np.concatenate([np.tile(base, (1, a.reps, 1)), np.zeros((2, L4 - L, 2), np.int16)], 1)).to(dev).to(torch.float32)
    gen = torch.Generator(device=dev); gen.manual_seed(1102)
    iq = torch.empty((2, a.streams, L4, 2), dtype=torch.int16, device=dev)
    for i in range(0, a.streams, 16):
        k = min(16, a.streams - i)
        for c in range(2):
            iq[c, i:i + k] = (b[c][None] + 20.0 * torch.randn((k, L4, 2), generator=gen, device=dev)).round().clamp(-32768, 32767).to(torch.int16)
    flat0, flat1 = iq[0].reshape(-1, 2), iq[1].reshape(-1, 2)
    piece = 28 * a.piece_calls
    torch.cuda.synchronize()
    out = {"workload": "%d two-chain streams x %d MCS 9 frames (%s, %d samples @40 MHz each), AWGN, pieces of %d samples" % (a.streams, a.reps, what, n, piece),
           "date": time.strftime("%Y-%m-%d")}

    def replay(calls):
        """the stream row's captures, call by call, with the mode off: what stream mode itself costs"""
        rx = sora_amd.Rx11n(a.streams, a.streams * L4, max_frames_per_capture=4)
        t_ms = 0.0; submitted = 0
        for descs in calls:
            d = sora_amd.Rx.captures(descs)
            t0 = time.perf_counter()
            rx.wait(rx.process_dev(flat0, flat1, d))
            t_ms += (time.perf_counter() - t0) * 1e3
            submitted += sum(x[1] for x in descs)
        rx.close()
        return {"calls": len(calls), "ms_per_call": round(t_ms / len(calls), 3), "msamples_per_s": round(submitted / t_ms / 1e3, 1)}

    def run(stream_mode, record=None, piece=piece):
        rx = sora_amd.Rx11n(a.streams, a.streams * L4, max_frames_per_capture=4)
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
            t = rx.process_dev(flat0, flat1, d)
            rx.wait(t)
            t_ms += (time.perf_counter() - t0) * 1e3
            rows = rx.results(ticket=t)
            frames += sum(r["error_code"] == 1 for r in rows)
            submitted += sum(x[1] for x in descs); calls += 1
            used = rx.stream_consumed(t, a.streams) if stream_mode else [x[1] for x in descs]
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
    # A capture that starts at a resume point inside a frame's preamble finds nothing with the mode off (a fresh graph has no energy history),
    # so the replay above decodes far fewer frames than the stream row.  Pieces of exactly one frame period cut only in the quiet gaps:
    # both modes then decode the same frames from the same captures, and the ratio is the cost of the mode itself.
    calls_al = []
    out["stream_aligned"] = run(True, calls_al, piece=n)
    out["same_captures_mode_off_aligned"] = replay(calls_al)
    out["stream_vs_mode_off_per_sample_aligned"] = round(out["stream_aligned"]["msamples_per_s"] / out["same_captures_mode_off_aligned"]["msamples_per_s"], 3)
    out["stream_progress_vs_plain"] = round(out["stream"]["stream_msamples_per_s"] / out["plain"]["msamples_per_s"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
