"""The 802.11n 2x2 receive handle per MCS (sora_rx11n_set_mcs_max at 14): for each of MCS 8..14 a batch of two-chain captures of one 1500-byte frame
(1496 bytes + FCS) from the GPU modulator, through a 2x2 channel with 0.1 cross-talk, noise of sigma 20 added on the device.  Reports, per trellis form
(k_viterbi11n, k_viterbi16_11n, the window-parallel k_viterbi16w_11n + k_win_redo_11n), ms per call with one call in flight and ms per frame, and with eight
calls in flight for the two serial forms.  Inside the run the rows and MPDU bytes of the first captures are compared with tests/rx11n_ext_model.py (the
reference's graph with the SIG parser's one comparison moved), and every capture's MPDU with the bytes that were sent.
usage: python tools/bench_rx11n_mcs.py [captures] [reps]   -> one JSON line per MCS"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
MPDU = 1496                           # without FCS
NAMES = {64: "k_viterbi11n", 16: "k_viterbi16_11n", 1: "k_viterbi16w_11n"}
CHECKED = 16                          # captures compared with the model, row for row


def bench_mcs(torch, sora_amd, model, mcs, ncaps, reps):
    dev = torch.device("cuda", 0)
    mp = np.random.default_rng(mcs).integers(0, 256, MPDU).astype(np.uint8).tobytes()
    o0, o1, _ = sora_amd.tx11n([mp], [mcs])
    s0 = o0.to(torch.float32); s1 = o1.to(torch.float32)
    n = (len(s0) + 800 + 1200 + 27) // 28 * 28
    base = torch.zeros((2, n, 2), dtype=torch.float32, device=dev)
    base[0, 800:800 + len(s0)] = s0 + 0.1 * s1; base[1, 800:800 + len(s0)] = s1 + 0.1 * s0
    gen = torch.Generator(device=dev); gen.manual_seed(1100 + mcs)
    iq = torch.empty((2, ncaps, n, 2), dtype=torch.int16, device=dev)
    for i in range(0, ncaps, 64):
        k = min(64, ncaps - i)
        for c in range(2):
            iq[c, i:i + k] = (base[c][None] + 20.0 * torch.randn((k, n, 2), generator=gen, device=dev)).round().clamp(-32768, 32767).to(torch.int16)
    descs = [(i * n, n, i) for i in range(ncaps)]
    f0 = iq[0].view(-1, 2); f1 = iq[1].view(-1, 2)
    rx = sora_amd.Rx11n(ncaps, ncaps * n, max_frames_per_capture=4)
    rx.set_mcs_max(14)
    one = {}; eight = {}; tables = {}
    for lanes in (64, 16, 1):
        rx.set_trellis(lanes); rx.set_depth(1)
        tables[lanes] = rx.results(ticket=rx.process_dev(f0, f1, descs))
        for _ in range(2):
            rx.wait(rx.process_dev(f0, f1, descs))
        t0 = time.perf_counter()
        for _ in range(reps):
            rx.wait(rx.process_dev(f0, f1, descs))
        one[NAMES[lanes]] = (time.perf_counter() - t0) / reps * 1e3
    for lanes in (64, 16):
        rx.set_trellis(lanes); rx.set_depth(8)
        for _ in range(8):
            rx.process_dev(f0, f1, descs)
        rx.synchronize()
        t0 = time.perf_counter()
        for _ in range(4 * reps):
            rx.process_dev(f0, f1, descs)
        rx.synchronize()
        eight[NAMES[lanes]] = (time.perf_counter() - t0) / (4 * reps) * 1e3
    rx.close()
    key = lambda r: (r["capture_id"], r["end_sample"], r["error_code"], r["rate_kbps"], r["length"], r["crc32"], r["mpdu"])
    same_forms = [key(r) for r in tables[64]] == [key(r) for r in tables[16]] == [key(r) for r in tables[1]]
    sent = mp + model.fcs(mp)
    ok = sum(r["error_code"] == 1 and r["rate_kbps"] == mcs and r["mpdu"] == sent for r in tables[64])
    h0 = iq[0, :CHECKED].cpu().numpy(); h1 = iq[1, :CHECKED].cpu().numpy()
    want = [dict(e, capture_id=i) for i in range(min(CHECKED, ncaps)) for e in model.rx11n(h0[i], h1[i], mcs_max=14)]
    got = [r for r in tables[64] if r["capture_id"] < CHECKED]
    model_ok = [key(r) for r in got] == [key(r) for r in want]
    return {"row": "rx11n_mcs", "mcs": mcs, "workload": "%d two-chain captures x one MCS %d frame, %d-byte MPDU (+FCS), %d samples @40 MHz per chain each, 2x2 cross-talk, AWGN"
            % (ncaps, mcs, MPDU, n), "ms_one_call_in_flight": {k: round(v, 3) for k, v in one.items()},
            "us_per_frame_one_call_in_flight": {k: round(v * 1e3 / ncaps, 3) for k, v in one.items()},
            "ms_eight_calls_in_flight": {k: round(v, 3) for k, v in eight.items()}, "us_per_frame_eight_calls_in_flight": {k: round(v * 1e3 / ncaps, 3) for k, v in eight.items()},
            "frames": ncaps, "frames_ok_with_the_sent_bytes": ok, "trellis_forms_same_table": same_forms, "captures_compared_with_model": min(CHECKED, ncaps),
            "equals_model": model_ok, "reps": reps}


def main():
    import torch
    import sora_amd
    import rx11n_ext_model as model
    ncaps = int(sys.argv[1]) if len(sys.argv) > 1 else 2048
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    bad = 0
    for mcs in range(8, 15):
        r = bench_mcs(torch, sora_amd, model, mcs, ncaps, reps)
        print(json.dumps(r), flush=True)
        bad += not (r["equals_model"] and r["trellis_forms_same_table"])
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
