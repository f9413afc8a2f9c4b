"""The joint coding of the 40 MHz HT 2x2 pair (sora_hip_tx_ht40_joint, sora_ht40_set_coding) beside the per-stream coding, one run on one
box: 4096 frames per call at MCS 14 and at MCS 8, as
  joint        one 1500-byte PSDU per frame (1496 bytes + FCS),
  split_750    per-stream frames of 2 x 750-byte PSDUs: the same payload in (nearly) the same number of symbols,
  split_1500   per-stream frames of 2 x 1500-byte PSDUs: twice the payload, twice the symbols.
Per row the transmitter (hipEvents over back-to-back calls) and the descriptor form of the receiver on what the transmitter sent (identity channel at the level the
receiver's tests use, zero forcing; wall clock over back-to-back sora_ht40_process_dev calls, eight in flight, then a synchronize), with every row of the last call
checked to be FRAME_OK.  Every row runs in a process of its own under `timeout -k 10`; the first one that fails ends the run.
usage: python tools/bench_ht40_joint.py [frames] [reps]   -> one JSON line per row"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ROW_TIMEOUT_S = 300
GAIN = 250.0 * 128.0 / 16384.0        # tests/test_gpu_tx_ht40.py: the level at which the receiver's own tests decode
MCS2 = {8: (1, 0), 9: (2, 0), 10: (2, 2), 11: (4, 0), 12: (4, 2), 13: (6, 1), 14: (6, 2)}


def bench(kind, mcs, nframes, reps):
    import torch
    import sora_amd
    from sora_amd import capi
    dev = torch.device("cuda")
    L = capi.load()
    joint = kind == "joint"
    mpdu = {"joint": 1496, "split_750": 746, "split_1500": 1496}[kind]
    nb, cr = MCS2[mcs]
    per = sora_amd.tx_ht40_joint_samples(mpdu, mcs) if joint else sora_amd.tx_ht40_samples(mpdu, mcs)
    nsym = (per - 1600) // 160
    nm = nframes if joint else 2 * nframes
    lens = torch.full((nframes,), mpdu, dtype=torch.int32, device=dev)
    mcsv = torch.full((nframes,), mcs, dtype=torch.int32, device=dev)
    moff = torch.arange(nm, dtype=torch.int32, device=dev) * mpdu
    blob = torch.randint(0, 256, (nm * mpdu,), dtype=torch.uint8, device=dev)
    ooff = torch.arange(nframes, dtype=torch.int64, device=dev) * per
    out0 = torch.zeros((nframes * per + 256, 2), dtype=torch.int16, device=dev); out1 = torch.zeros_like(out0)
    fn = L.sora_hip_tx_ht40_joint if joint else L.sora_hip_tx_ht40
    call = lambda: fn(capi._dev_ptr(blob), capi._dev_ptr(moff), capi._dev_ptr(lens), capi._dev_ptr(mcsv), None, nframes,
                      capi._dev_ptr(out0), capi._dev_ptr(out1), capi._dev_ptr(ooff), capi._stream_ptr(None))
    for _ in range(3):
        assert call() == 0
    e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(); e0.record()
    for _ in range(reps):
        call()
    e1.record(); torch.cuda.synchronize()
    tx_ms = e0.elapsed_time(e1) / reps
    # the receiver's descriptor form on those frames
    scale = lambda o: torch.clamp(torch.round(o.float() * GAIN), -32768, 32767).to(torch.int16)
    iq0, iq1 = scale(out0), scale(out1)
    del out0, out1
    descs = sora_amd.RxHt40.frames([(f * per + 1280, nb, cr, mpdu + 4, 0 if joint else mpdu + 4, 0, 0.0, f) for f in range(nframes)])
    rx = sora_amd.RxHt40(nframes, nframes * 2 * (nsym * 108 * nb + 64))
    rx.set_coding(sora_amd.HT40_CODING_JOINT if joint else sora_amd.HT40_CODING_PER_STREAM)
    for _ in range(3):
        rx.process_dev(iq0, iq1, descs)
    rx.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        rx.process_dev(iq0, iq1, descs)
    rx.synchronize()
    rx_ms = (time.perf_counter() - t0) * 1e3 / reps
    rows = rx.results(with_mpdu=False)
    want_rows = nframes * (1 if joint else 2)
    ok = len(rows) == want_rows and all(r["error_code"] == 1 for r in rows)
    rx.close()
    payload = nframes * (mpdu + 4) * (1 if joint else 2)
    return {"row": "ht40_%s" % kind, "mcs": mcs, "frames": nframes, "psdu_bytes_per_frame": (mpdu + 4) * (1 if joint else 2), "data_symbols_per_frame": nsym,
            "tx_ms": round(tx_ms, 4), "rx_descriptor_ms": round(rx_ms, 4), "tx_us_per_frame": round(tx_ms * 1e3 / nframes, 3), "rx_us_per_frame": round(rx_ms * 1e3 / nframes, 3),
            "tx_payload_gbit_s": round(payload * 8 / tx_ms / 1e6, 2), "rx_payload_gbit_s": round(payload * 8 / rx_ms / 1e6, 2), "rows": len(rows), "all_frame_ok": ok, "reps": reps}


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--row":                            # one row, in this process
        out = bench(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5]))
        print(json.dumps(out), flush=True)
        return 0 if out["all_frame_ok"] else 2
    nframes = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    for mcs in (14, 8):
        for kind in ("joint", "split_750", "split_1500"):
            rc = subprocess.run(["timeout", "-k", "10", str(ROW_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--row", kind, str(mcs), str(nframes), str(reps)]).returncode
            if rc != 0:
                print(json.dumps({"row": "ht40_%s" % kind, "mcs": mcs, "failed": rc}), flush=True)
                return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
