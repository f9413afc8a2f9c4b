"""Stream mode of the 40 MHz HT receive handle (sora_ht40_set_stream_mode) against the same captures with the mode off.  The capture of the HT40
bench row (benchlib/rows.py bench_ht40: one HT-mixed MCS 14 frame, a 1500-byte PSDU per stream, 2x2 cross-talk, a gap on either side) is
repeated REPS times into each of STREAMS two-chain streams on the device, AWGN per stream.  PIECE samples of every stream 'arrive' per call,
and the call carries one capture per stream: from where the stream's last call left it (its resume point) to what has arrived -- a frame a
piece cuts is found again by the next call, when it is whole.  One call in flight (stream mode runs its calls one after the other).
  stream                   the calls above, in stream mode: ms per call, input samples per second (per chain), frames reported, and whether
                           every frame was reported exactly once
  same_captures_mode_off   the very same captures, call for call, with the mode off.  A capture that starts at a resume point in front of a
                           detection has no energy history with the mode off and finds nothing there, and a cut frame raises no event, so
                           this row runs the same front end over the same samples but decodes fewer data fields
  *_aligned                the same pair with pieces of exactly one frame period, cut in the gaps, where both modes find and decode the same
                           frames from the same captures: the cost of the mode itself
The two rows of a pair alternate ROUNDS times in one process; the figures are the medians over the rounds.
usage: python tools/bench_stream_ht40.py [--streams 4096] [--piece-calls 128] [--reps 3] [--rounds 3]   -> one JSON line"""
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
    ap.add_argument("--piece-calls", type=int, default=128, help="source calls (28 samples) per piece")
    ap.add_argument("--reps", type=int, default=3, help="frames per stream")
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    import torch
    import sora_amd
    from oracle import py_ht40 as m
    if sora_amd.device_count() <= 0:
        raise SystemExit("no HIP device: nothing to measure")
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(40)
    ps = [m.add_fcs(rng.integers(0, 256, 1496, dtype=np.uint8).tobytes()) for _ in range(2)]
    x, nsym, pre = m.tx_frame(ps, 14)
    y = (np.array([[1.0, 0.3j], [0.25, 0.9 * np.exp(0.7j)]]) @ x) * 250.0
    lead, sigma = 400, 12.0
    n = (lead + y.shape[1] + 600 + 27) // 28 * 28                        # one frame and its gaps: the bench row's capture
    base = np.zeros((2, n, 2), np.float32); base[:, lead:lead + y.shape[1], 0] = y.real; base[:, lead:lead + y.shape[1], 1] = y.imag
    L = n * a.reps
    L4 = L + 28 * 8                                                     # a noise-only tail
    b = torch.from_numpy(np.concatenate([np.tile(base, (1, a.reps, 1)), np.zeros((2, L4 - L, 2), np.float32)], 1)).to(dev)
    gen = torch.Generator(device=dev); gen.manual_seed(4041)
    iq = torch.empty((2, a.streams, L4, 2), dtype=torch.int16, device=dev)
    for i in range(0, a.streams, 64):
        k = min(64, a.streams - i)
        for c in range(2):
            iq[c, i:i + k] = (b[c][None] + sigma * torch.randn((k, L4, 2), generator=gen, device=dev)).round().clamp(-32768, 32767).to(torch.int16)
    flat0, flat1 = iq[0].reshape(-1, 2), iq[1].reshape(-1, 2)
    piece = 28 * a.piece_calls
    torch.cuda.synchronize()
    # a call's capture is shorter than a piece and the tail in front of it, so it holds two whole frames at the most
    rx = sora_amd.RxHt40(2 * a.streams, 2 * a.streams * 2 * (nsym * 648 + 64))
    rx.wait_for_producer = False
    out = {"workload": "%d two-chain 40 MHz streams x %d HT-mixed MCS 14 frames (1500-byte PSDU per stream, %d data symbols, %d samples per frame period), "
                       "AWGN, pieces of %d samples, one call in flight" % (a.streams, a.reps, nsym, n, piece), "date": time.strftime("%Y-%m-%d")}

    def timed_call(d):
        t0 = time.perf_counter()
        t = rx.process_captures_dev(flat0, flat1, d, max_frames_per_capture=2)
        rx.wait(t)                                                      # (ends in a synchronise of the call's stream)
        return t, (time.perf_counter() - t0) * 1e3

    def replay(calls):
        """the stream row's captures, call by call, with the mode off"""
        rx.set_stream_mode(0)
        t_ms = 0.0; submitted = 0; frames = 0
        for descs in calls:
            t, ms = timed_call(sora_amd.Rx.captures(descs))
            t_ms += ms; submitted += sum(x[1] for x in descs)
            frames += sum(r["error_code"] == 1 for r in rx.results(with_mpdu=False, ticket=t)) // 2
        return {"calls": len(calls), "ms_per_call": t_ms / len(calls), "msamples_per_s": submitted / t_ms / 1e3, "frames_ok": frames}

    def run(piece, record=None):
        rx.set_stream_mode(0); rx.set_stream_mode(1)                    # every stream afresh
        pos = [0] * a.streams; arrived = [0] * a.streams
        seen = np.zeros(a.streams, np.int64); ends = set(); twice = 0
        calls = submitted = 0
        t_ms = 0.0
        while True:
            descs = []
            for k in range(a.streams):
                arrived[k] = min(L4, max(arrived[k], pos[k]) + piece)
                descs.append((k * L4 + pos[k], (arrived[k] - pos[k]) // 28 * 28, k))
            if not any(d[1] for d in descs):
                break
            if record is not None:
                record.append(descs)
            t, ms = timed_call(sora_amd.Rx.captures(descs))
            t_ms += ms; submitted += sum(x[1] for x in descs); calls += 1
            for r in rx.results(with_mpdu=False, ticket=t):
                if r["error_code"] == 1 and r["stream"] == 0:
                    key = (r["capture_id"], pos[r["capture_id"]] + r["end_sample"])
                    twice += key in ends; ends.add(key); seen[r["capture_id"]] += 1
            used = rx.stream_consumed(t, a.streams)
            stuck = all(int(u) == 0 for u, x in zip(used, descs) if x[1]) and all(v == L4 for v in arrived)      # (nothing more to come)
            for k in range(a.streams):
                pos[k] += int(used[k])
            if stuck:
                break
        return {"calls": calls, "ms_per_call": t_ms / calls, "msamples_per_s": submitted / t_ms / 1e3, "stream_msamples_per_s": sum(pos) / t_ms / 1e3,
                "frames_ok": int(seen.sum()), "frames_sent": a.streams * a.reps, "every_frame_exactly_once": bool((seen == a.reps).all()) and twice == 0}

    def pair(piece):
        on, off = [], []
        run(piece)                                                      # warm-up (code objects, allocations of this shape)
        for _ in range(a.rounds):
            calls = []
            on.append(run(piece, calls)); off.append(replay(calls))
        med = lambda rows, f: float(np.median([r[f] for r in rows]))
        s = dict(on[0], ms_per_call=round(med(on, "ms_per_call"), 3), msamples_per_s=round(med(on, "msamples_per_s"), 1),
                 stream_msamples_per_s=round(med(on, "stream_msamples_per_s"), 1), every_frame_exactly_once=all(r["every_frame_exactly_once"] for r in on),
                 ms_per_call_rounds=[round(r["ms_per_call"], 3) for r in on])
        o = dict(off[0], ms_per_call=round(med(off, "ms_per_call"), 3), msamples_per_s=round(med(off, "msamples_per_s"), 1),
                 ms_per_call_rounds=[round(r["ms_per_call"], 3) for r in off])
        return s, o, round(s["msamples_per_s"] / o["msamples_per_s"], 3)

    out["stream"], out["same_captures_mode_off"], out["stream_vs_mode_off_per_sample"] = pair(piece)
    out["stream_aligned"], out["same_captures_mode_off_aligned"], out["stream_vs_mode_off_per_sample_aligned"] = pair(n)
    rx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
