"""Short-GI frames composed from the EXISTING stage entry points (sora_amd.rx_ht40_by_stages; no new stage kernel: per data symbol freq_comp11n over 18 bursts at
offset + 320 + 144 d, then data_symbol_ht40 from 16 samples earlier, whose samples 32..159 are the symbol's 128 useful ones) against the handle's
one kernel: every soft byte, row and PSDU byte and the exported weights, in both codings, long and short frames in one batch; and against tests/ht40_gi_model.py, which
adds what the handle does not export: the tracked phase theta and the detected symbols.  The model's own composition (tests/ht40_stage_model.by_stages through the same
rx_ht40_stages) is held to ht40_gi_model here too and, without a GPU, in tests/test_ht40_gi_models_cpu.py."""
import numpy as np
import pytest

from ht40_gi_cases import ROW_SHORT_GI, SHORT, bank as make_bank, capacity, descs as describe, models, place
import ht40_stage_model as sm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import torch
    import sora_amd
    if sora_amd.device_count() <= 0:
        pytest.skip("no HIP device")
    return torch, sora_amd


@pytest.fixture(scope="module", params=[0, 1], ids=["per_stream", "joint"])
def case(request):
    """nine frames of the shared bank: every n_bpsc and detector, N_SYM 1, 2 and one of 40, both kinds next to each other"""
    joint = request.param
    frames = make_bank(joint)
    pick = [f for f in frames if f["nsym"] <= 2][:8] + [next(f for f in frames if f["nsym"] >= 40 and f["gi"])]
    assert {f["gi"] for f in pick} == {0, 1} and {f["nb"] for f in pick if f["gi"]} == {1, 2, 4, 6}
    iq, offs = place(np.random.default_rng(5500 + joint), pick, (1, 2, 3, 0))
    return joint, pick, iq, describe(pick, offs)


def test_by_stages_equals_the_handle_and_the_model(env, case):
    torch, sora = env
    joint, frames, iq, descs = case
    d0, d1 = torch.from_numpy(iq[0].copy()).cuda(), torch.from_numpy(iq[1].copy()).cuda()
    rx = sora.RxHt40(len(descs), capacity(frames))
    rx.set_coding(joint)
    w = torch.zeros((len(descs), 4, 128, 2), dtype=torch.int16, device="cuda")
    t = rx.process_dev(d0, d1, descs, w)
    rows = rx.results(ticket=t)
    soft = [rx.soft(f, 0, ticket=t) if joint else [rx.soft(f, s, ticket=t) for s in range(2)] for f in range(len(descs))]
    rx.close()
    w = w.cpu().numpy()
    r = sora.rx_ht40_by_stages(d0, d1, descs, joint)
    gw = r["weights"].cpu().numpy()
    assert np.array_equal(gw[:, :, sm.OCC], w[:, :, sm.OCC])
    assert len(r["rows"]) == len(rows) == (1 if joint else 2) * len(descs)
    for g, h in zip(r["rows"], rows):
        assert (g["error_code"], g["length"], g["crc32"], g["nsym"], g["mpdu"]) == (h["error_code"], h["length"], h["crc32"], h["nsym"], h["mpdu"]), (g["frame"], g["stream"])
        assert h["stream"] == g["stream"] and h["capture_id"] == descs[g["frame"]][7]
        short = bool(descs[g["frame"]][2] & SHORT)
        assert g["short_gi"] == h["short_gi"] == short and h["flags"] == (ROW_SHORT_GI if short else 0), g["frame"]
        assert g["error_code"] == 1, (g["frame"], hex(g["error_code"]))       # clean frames
    want = models(joint, iq, descs, w)
    for f in range(len(descs)):
        if joint:
            assert np.array_equal(r["soft"][f], soft[f]) and np.array_equal(soft[f], want[f].soft), f
        else:
            for s in range(2):
                assert np.array_equal(r["soft"][f][s], soft[f][s]) and np.array_equal(soft[f][s], want[f].soft[s]), (f, s)
        assert np.array_equal(r["theta"][f], want[f].theta), (f, r["theta"][f], want[f].theta)
        assert np.array_equal(r["xs"][f][:, :, sm.OCC], want[f].xs[:, :, sm.OCC]), f          # (the 114 occupied carriers: the stages zero the weights of the 14 others)


def test_the_models_composition_equals_the_gi_model(case):
    """tests/ht40_stage_model.by_stages through the same rx_ht40_stages, on the model's own zero-forcing and MMSE weights: soft bytes, theta, detected symbols, rows"""
    joint, frames, iq, descs = case
    r = sm.by_stages(iq, descs, joint)
    want = models(joint, iq, descs, np.asarray(r["weights"]))
    per = 1 if joint else 2
    for f in range(len(descs)):
        got_soft = [r["soft"][f]] if joint else r["soft"][f]
        want_soft = [want[f].soft] if joint else want[f].soft
        for a, b in zip(got_soft, want_soft):
            assert np.array_equal(a, b), f
        assert np.array_equal(r["theta"][f], want[f].theta) and np.array_equal(r["xs"][f], want[f].xs), f
        for s in range(per):
            g = r["rows"][per * f + s]
            ws = want[f] if joint else want[f].streams[s]
            assert (g["error_code"], g["crc32"], g["mpdu"]) == (ws.error_code, ws.crc32, ws.psdu), (f, s)
            assert g["short_gi"] == bool(descs[f][2] & SHORT)
