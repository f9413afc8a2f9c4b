"""tests/cxx/rx11a_front_chain.cpp -- a C++ host that runs one capture through carrier sense, T11aLTS, the SIGNAL symbol and the parser with the six 802.11a front-end
adapters of include/sora_brick.hpp (THip11aDCRemoveEx, THip11aCCA, THip11aDCEstimator, THip11aDataSymbol, THip11aViterbiSig, THip11aPLCPParser) -- built and run on the
GPU: its detection point, CFO estimate and parsed SIGNAL fields equal the receive handle's row for the same capture."""
import os

import numpy as np
import pytest

import scan_captures as sc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NDBPS = {6000: 24, 9000: 36, 12000: 48, 18000: 72, 24000: 96, 36000: 144, 48000: 192, 54000: 216}


def test_rx11a_front_chain_host(oracle, tmp_path):
    import torch
    import sora_amd
    from test_gpu_hosts import build, run
    # a capture whose lead holds time-outs and a DC step in front of the frame: the loop's feedback and both Resets are on the way to the detection
    cap = sc.families(oracle)["dc_steps"][1]
    rx = sora_amd.Rx(1, len(cap), sample_rate_mhz=40, max_frames_per_capture=8)
    rows = rx.results(ticket=rx.process_dev(torch.from_numpy(cap).cuda(), [(0, len(cap), 0)]))
    rx.close()
    assert len(rows) == 1 and rows[0]["error_code"] == 0x1 and rows[0]["start_sample"] > 21 * 4 * 8
    path = tmp_path / "capture.i16"
    np.ascontiguousarray(cap[::2]).tofile(str(path))
    out = run([build("g++", "-std=c++17", os.path.join(ROOT, "tests", "cxx", "rx11a_front_chain.cpp"), "rx11a_front_chain"), str(path)])
    f = dict(l.split("=", 1) for l in out.split() if "=" in l)
    r = rows[0]
    assert f["detected"] == "1" and int(f["start"]) == r["start_sample"] and int(f["cfo_est"]) == r["cfo_est"], (f, r)
    assert int(f["error_code"], 16) == 0 and int(f["rate_kbps"]) == r["rate_kbps"] and int(f["length"]) == r["length"], (f, r)
    assert int(f["total_symbols"]) == r["nsym"] + 1 == int(f["remain_symbols"]) and int(f["plcp_state"]) == 1, (f, r)
    assert int(f["code_rate"]) == {54000: 2}[r["rate_kbps"]]
    assert r["nsym"] == (8 * r["length"] + 22 + NDBPS[r["rate_kbps"]] - 1) // NDBPS[r["rate_kbps"]]
