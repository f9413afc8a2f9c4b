"""The 40 MHz HT data field with the short guard interval (SORA_HT40_SHORT_GI on a descriptor's code rate; k_ht40_frame_gi, k_ht40_frame_joint_gi; DESIGN.md section 7
g4) held BIT FOR BIT to tests/ht40_gi_model.py from the detection weights on: every soft byte (sora_ht40_soft_of), every row field and every PSDU byte, in both codings,
for every n_bpsc under both detectors, at cfo 0, a small one and one whose phase index n cfo wraps 65536 many times inside the frame, N_SYM 1, 2 and about 40, offsets at
odd residues, long and short frames interleaved so that the four waves of a workgroup differ in kind -- and a call without any flagged frame (the kernels without the
option) beside them.  The weights are the handle's own exported d_weights, as in tests/test_gpu_ht40_soft.py.  Behind every frame lie at least 16 nsym + 64 samples of
random filler inside the allocation: a wrong pitch reads wrong data, never outside the buffer."""
import numpy as np
import pytest

from ht40_gi_cases import CFOS, ROW_SHORT_GI, SHORT, bank as make_bank, capacity, descs as describe, models, place
from ht40_soft_check import assert_is_the_joint_model, assert_is_the_model

pytestmark = pytest.mark.gpu



@pytest.fixture(scope="module")
def env():
    import torch
    import sora_amd
    if sora_amd.device_count() <= 0:
        pytest.skip("no HIP device")
    return torch, sora_amd


@pytest.fixture(scope="module", params=[0, 1], ids=["per_stream", "joint"])
def bank(request):
    return request.param, make_bank(request.param)


def _call(env, joint, iq, descs, frames):
    torch, sora = env
    rx = sora.RxHt40(len(descs), capacity(frames))
    rx.set_coding(joint)
    w = torch.zeros((len(descs), 4, 128, 2), dtype=torch.int16, device="cuda")
    t = rx.process_dev(torch.from_numpy(iq[0].copy()).cuda(), torch.from_numpy(iq[1].copy()).cuda(), descs, w)
    rows = rx.results(ticket=t)
    soft = [rx.soft(f, 0, ticket=t) if joint else [rx.soft(f, s, ticket=t) for s in range(2)] for f in range(len(descs))]
    rx.close()
    return {"rows": rows, "soft": soft, "w": w.cpu().numpy()}


def _check(joint, got, want, descs, what):
    plain = [d[:2] + (d[2] & ~SHORT,) + d[3:] for d in descs]
    (assert_is_the_joint_model if joint else assert_is_the_model)(got, want, plain, what)
    per = 1 if joint else 2
    for f, d in enumerate(descs):
        for r in got["rows"][per * f:per * f + per]:
            assert r["flags"] == (ROW_SHORT_GI if d[2] & SHORT else 0) and r["short_gi"] == bool(d[2] & SHORT), (what, f, r["flags"])
            assert r["rate_kbps"] == 10 * d[1] + (d[2] & ~SHORT), (what, f)


def test_mixed_kinds_every_soft_byte_row_and_psdu(env, bank):
    joint, frames = bank
    rng = np.random.default_rng(5200 + joint)
    short = [f for f in frames if f["gi"]]
    assert {(f["nb"], f["nv"] > 0) for f in short} == {(nb, z) for nb in (1, 2, 4, 6) for z in (False, True)}
    assert {f["cfo"] for f in short} == set(CFOS) and {1, 2} <= {f["nsym"] for f in short} and max(f["nsym"] for f in short) >= 30
    assert all(len({f["gi"] for f in frames[g:g + 4]}) == 2 for g in range(0, len(frames), 4))        # every workgroup holds both kinds
    assert max(abs(f["cfo"]) * (320 + 144 * f["nsym"]) for f in short) > 20 * 65536                     # the phase index wraps inside the frame
    iq, offs = place(rng, frames, (1, 3, 0, 2, 1))
    assert {o % 4 for o, f in zip(offs, frames) if f["gi"]} == {0, 1, 2, 3}
    descs = describe(frames, offs)
    got = _call(env, joint, iq, descs, frames)
    want = models(joint, iq, descs, got["w"])
    _check(joint, got, want, descs, "mixed kinds")
    for f, fr in enumerate(frames):                                        # clean frames: the model, and so the GPU, decodes them
        if joint:
            assert want[f].error_code == 1 and want[f].psdu == fr["ps"][0], f
        else:
            assert [want[f].streams[s].psdu for s in range(2)] == fr["ps"] and all(want[f].streams[s].error_code == 1 for s in range(2)), f


def test_a_call_without_a_flagged_frame_and_small_batches(env, bank):
    joint, frames = bank
    rng = np.random.default_rng(5300 + joint)
    longs = [f for f in frames if not f["gi"]][:6]
    iq, offs = place(rng, longs, (2, 1, 3))
    descs = describe(longs, offs)
    assert not any(d[2] & SHORT for d in descs)
    got = _call(env, joint, iq, descs, longs)
    _check(joint, got, models(joint, iq, descs, got["w"]), descs, "no flagged frame")
    # one short frame alone, and five frames: a workgroup and one frame more, the last wave of the first workgroup and the only wave of the second short
    shorts = [f for f in frames if f["gi"]]
    for pick in ([shorts[0]], [frames[0], frames[1], frames[3], shorts[4], shorts[5]]):
        iq, offs = place(rng, pick, (1, 2, 3))
        descs = describe(pick, offs)
        got = _call(env, joint, iq, descs, pick)
        _check(joint, got, models(joint, iq, descs, got["w"]), descs, "batch of %d" % len(pick))


def test_a_short_frame_read_at_the_long_pitch_is_not_the_short_frame(env, bank):
    """the flag matters: the same samples described without it give other soft bytes (the model's long reading of them: the filler keeps that reading in bounds)"""
    joint, frames = bank
    rng = np.random.default_rng(5400 + joint)
    pick = [f for f in frames if f["gi"] and f["nsym"] >= 2][:3]
    iq, offs = place(rng, pick, (1, 2, 3))
    descs = describe(pick, offs, flagged=False)
    got = _call(env, joint, iq, descs, pick)
    want = models(joint, iq, descs, got["w"])
    _check(joint, got, want, descs, "short frames described as long")
    flagged = models(joint, iq, describe(pick, offs), got["w"])
    for f in range(len(pick)):
        a = want[f].soft if joint else want[f].soft[0]; b = flagged[f].soft if joint else flagged[f].soft[0]
        assert not np.array_equal(a, b), f


def test_other_bits_on_the_code_rate_are_still_refused(env):
    torch, sora = env
    z = torch.zeros((4096, 2), dtype=torch.int16, device="cuda")
    rx = sora.RxHt40(4, 4 * (2 * 108 * 6 + 64))
    for cr in (3, 0x103, 0x200, 0x201, 0x180, 0x101 | 0x80000000, 0x1100):
        with pytest.raises(sora.SoraError) as e:
            rx.process_dev(z, z, [(0, 2, cr, 30, 30, 0, 0.0, 0)])
        assert e.value.code == -1, hex(cr)
    t = rx.process_dev(z, z, [(0, 2, 0x101, 30, 30, 0, 0.0, 9)])          # ... and the flag alone is accepted
    rows = rx.results(ticket=t)
    assert len(rows) == 2 and all(r["flags"] == ROW_SHORT_GI and r["capture_id"] == 9 and r["rate_kbps"] == 21 for r in rows)
    rx.close()
