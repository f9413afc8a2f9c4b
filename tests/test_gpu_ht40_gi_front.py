"""The front end of the 40 MHz HT receiver with sora_ht40_set_guard (k_scan_ht40_gi, k_ht40_plan's flag, the host's event collection) on raw
captures, held to tests/ht40_front_gi_model.py record for record (sora_ht40_found_of): a20, mcs (with SORA_HT40_SHORT_GI on a recorded short-GI frame), ht_len, nsym, cfo,
end_sample, error_code and the event count, no tolerance; noise_var within the rounding of its single-precision sum, as tests/test_gpu_ht40_front.py states it.
  * SORA_HT40_GUARD_LONG on captures that hold short-GI frames equals the EXISTING model (tests/ht40_front_model.py): the bit is not looked at;
  * SORA_HT40_GUARD_SIGNALLED on the existing capture families equals the existing model;
  * SORA_HT40_GUARD_SIGNALLED on short-GI captures (tests/ht40_gi_captures.py): a short extent that ends on the capture's last sample, the same 28 samples shorter, a
    frame that fits only because it is short, a second frame behind a short one, a header failure with bit 31 set, more events than row slots;
  * the plan by equivalence: the records, translated by the stated rule with the flag on the code rate, fed to the descriptor call give the raw call's rows and bytes
    (that call is held to tests/ht40_gi_model.py bit for bit in tests/test_gpu_ht40_gi_soft.py);
  * the whole call on loop-back captures of tx_ht40(..., gi=...), long and short frames mixed in one capture, through a channel, noise and a carrier offset: all
    FRAME_OK with the sent bytes -- at a level and noise at which the float64 receiver (oracle/ht40_rx_f64.py; per-stream coding, the one it knows) decodes every frame,
    the short ones re-spaced, on the CPU."""
import functools

import numpy as np
import pytest

from oracle import ht40_rx_f64 as rx64
from oracle import py_ht40 as m
import ht40_front_captures as fc
import ht40_front_model as fm
import ht40_gi_captures as gc
import tx_ht40_gi_model as TG
import tx_ht40_model as T
from test_gpu_ht40_front import E_PLCP, case_set, check_records, dev, raw_call

pytestmark = pytest.mark.gpu
ROW_TRUNCATED, ROW_SHORT_GI, SHORT = 1, 4, 0x100
GAIN = 250.0 * 128.0 / T.A


@pytest.fixture(scope="module")
def env():
    import torch
    import sora_amd
    if sora_amd.device_count() <= 0:
        pytest.skip("no HIP device")
    return torch, sora_amd


@functools.lru_cache(maxsize=None)
def gi_set(joint):
    from oracle.pyoracle import Oracle
    caps = gc.build(joint, Oracle())
    iq, descs = fc.layout(caps)
    return caps, iq, descs


def guarded_call(env, f0, f1, descs, mf, joint, mode):
    _, sora = env
    rx = sora.RxHt40(256, 1 << 21)
    if joint:
        rx.set_coding(sora.HT40_CODING_JOINT)
    assert rx.set_guard(mode) == 0 and rx.set_guard() == mode
    return raw_call(env, f0, f1, descs, mf, joint, rx=rx)


@pytest.mark.parametrize("joint", [False, True], ids=["per-stream", "joint"])
def test_mode_0_does_not_look_at_the_bit(env, joint):
    caps, iq, descs = gi_set(joint)
    want = [fm.front(c.iq[0], c.iq[1], flags=fm.OWN | (fm.JOINT if joint else 0)) for c in caps]
    f0, f1 = dev(env, iq)
    rx, t, got = guarded_call(env, f0, f1, descs, gc.MAX_EVENTS, joint, 0)
    rows = rx.results(ticket=t); rx.close()
    check_records([c.name for c in caps], got, want, gc.MAX_EVENTS, "mode 0 on short-GI captures")
    assert sum(len(g) for g in got) >= 20 and not any(r["flags"] & ROW_SHORT_GI for r in rows) and not any(r["mcs"] & SHORT for g in got for r in g)


def test_mode_1_on_the_existing_families_is_the_existing_model(env):
    for joint in (False, True):
        caps, iq, descs, want = case_set(joint)
        f0, f1 = dev(env, iq)
        rx, t, got = guarded_call(env, f0, f1, descs, fc.MAX_EVENTS, joint, 1)
        rows = rx.results(ticket=t); rx.close()
        check_records([c.name for c in caps], got, want, fc.MAX_EVENTS, "mode 1 on the existing families")
        assert sum(len(g) for g in got) > len(caps) // 2 and not any(r["flags"] & ROW_SHORT_GI for r in rows)


@pytest.mark.parametrize("joint", [False, True], ids=["per-stream", "joint"])
def test_mode_1_on_short_gi_captures_records_rows_and_the_plan(env, joint):
    torch, sora = env
    caps, iq, descs = gi_set(joint)
    mf = gc.MAX_EVENTS
    want = gc.want_records(caps, joint, True)
    by = {t: [i for i, c in enumerate(caps) if t in c.tags] for t in ("exact", "short28", "only_short", "two", "gate", "slots", "long")}
    assert all(by.values()), by
    # what the cases are there for, stated on the model's events before the library is asked
    for i in by["exact"] + by["only_short"]:
        assert len(want[i]) == 1 and want[i][0]["short_gi"] and want[i][0]["error_code"] == 0
        assert fm.front(caps[i].iq[0], caps[i].iq[1], flags=fm.OWN | (fm.JOINT if joint else 0)) == [], "the long extent passes the capture's end"
    e = want[by["exact"][0]][0]
    assert 2 * (e["a20"] + 240 + 72 * e["nsym"]) == len(caps[by["exact"][0]].iq[0]) == e["end_sample"]
    assert want[by["short28"][0]] == [] and len(caps[by["short28"][0]].iq[0]) == e["end_sample"] - 28
    assert all(len(want[i]) == 2 and not want[i][0]["error_code"] and not want[i][1]["error_code"] for i in by["two"])
    assert [w["error_code"] for w in want[by["gate"][0]]] == [E_PLCP] and len(want[by["slots"][0]]) > mf and want[by["slots"][0]][mf - 1]["short_gi"]
    f0, f1 = dev(env, iq)
    rx, t, got = guarded_call(env, f0, f1, descs, mf, joint, 1)
    check_records([c.name for c in caps], got, want, mf, "mode 1 on short-GI captures")
    raw = rx.results(ticket=t)
    # ---- the rows, as far as the front end decides them
    jpf = 1 if joint else 2
    exp = []
    for d, ev in zip(descs, want):
        for i, e in enumerate(ev[:mf]):
            flag = ROW_TRUNCATED if (i + 1 == mf and len(ev) > mf) else 0
            if e["error_code"]:
                exp.append((d[2], 0, e["end_sample"], E_PLCP, 0, 0, flag))
            else:
                exp += [(d[2], s, e["end_sample"], None, e["mcs"] & ~SHORT, e["nsym"], flag | (ROW_SHORT_GI if e["short_gi"] else 0)) for s in range(jpf)]
    assert len(raw) == len(exp)
    for r, e in zip(raw, exp):
        assert (r["capture_id"], r["stream"], r["end_sample"], None if e[3] is None else r["error_code"], r["rate_kbps"], r["nsym"], r["flags"]) == e, (r, e)
        assert r["short_gi"] == bool(e[6] & ROW_SHORT_GI)
    assert any(r["flags"] == ROW_TRUNCATED | ROW_SHORT_GI for r in raw) and any(r["flags"] == 0 and r["error_code"] == 1 for r in raw)
    # ---- the same rows through page-locked delivery
    buf = sora.HostResults(2 * len(descs) * mf, 1 << 20)
    t2 = rx.process_captures_dev(f0, f1, descs, max_frames_per_capture=mf)
    rx.deliver_async(t2, buf); rx.wait(t2)
    key = lambda r: (r["capture_id"], r["start_sample"], r["end_sample"], r["error_code"], r["rate_kbps"], r["length"], r["nsym"], r["crc32"], r["flags"], r["mpdu"])
    assert [key(r) for r in buf.results()] == [key(r) for r in raw]
    buf.close()
    # ---- the plan by equivalence: records -> descriptors with the flag on the code rate -> the descriptor call
    fdescs = []
    for d, g in zip(descs, got):
        for r in g:
            if r["error_code"] == 0:
                x = fm.descriptor(d[0], dict(r, mcs=r["mcs"] & ~SHORT), float(r["noise_var"]), joint, d[2])
                # a short-GI frame is taken 16 samples later than a20 says (its timing lies 21..28 samples inside the LONG guard interval), as far as the capture reaches
                adv = min(16, d[1] - (2 * r["a20"] + 480 + 144 * r["nsym"])) if r["mcs"] & SHORT else 0
                assert adv >= 0
                fdescs.append((x[0] + adv, x[1], x[2] | (r["mcs"] & SHORT)) + x[3:])
    assert sum(1 for x in fdescs if x[2] & SHORT) >= 20 and sum(1 for x in fdescs if not x[2] & SHORT) >= 3
    td = rx.process_dev(f0, f1, fdescs)
    rows = rx.results(ticket=td)
    rx.close()
    framed = [r for r in raw if r["error_code"] != E_PLCP]
    assert len(framed) == len(rows) == jpf * len(fdescs)
    for a, b in zip(framed, rows):
        assert (a["stream"], a["error_code"], a["length"], a["crc32"], a["nsym"], a["capture_id"], a["mpdu"], a["flags"] & ROW_SHORT_GI) == \
               (b["stream"], b["error_code"], b["length"], b["crc32"], b["nsym"], b["capture_id"], b["mpdu"], b["flags"]), (a["capture_id"], a["stream"])
    assert any(x[0] - (d[0] + 2 * r["a20"] + 160) == 0 and x[2] & SHORT for x, (d, r) in
               zip(fdescs, [(d, r) for d, g in zip(descs, got) for r in g if r["error_code"] == 0]))                  # "ends on the last sample": no room to move
    # ... and these are clean frames: the sent bytes come back (but where the capture ends on the extent's last sample: it cuts the frame's own last 21..28 samples)
    k = 0
    for c, ev in zip(caps, want):
        sound = [s for s in c.sent if s["sound"]]
        for e, s in zip([e for e in ev[:mf] if not e["error_code"]], sound):
            for st in range(jpf):
                if "exact" not in c.tags:
                    assert framed[k]["error_code"] == 1 and framed[k]["mpdu"] == s["psdus"][st], (c.name, st, hex(framed[k]["error_code"]))
                k += 1
    assert k == len(framed)


def test_set_guard_answers_and_refuses(env):
    _, sora = env
    rx = sora.RxHt40(4, 1 << 14)
    assert rx.set_guard() == 0 and rx.set_guard(1) == 0 and rx.set_guard(-5) == 1 and rx.set_guard(0) == 1 and rx.set_guard() == 0
    with pytest.raises(sora.SoraError) as e:
        rx.set_guard(2)
    assert e.value.code == -1 and rx.set_guard() == 0
    rx.close()


# ------------------------------------------------------------------ the whole call on the transmitter's frames
def loopback(env, rng, specs, cfo_step, joint):
    """specs: per capture [(mcs, len, gi)].  One tx_ht40 / tx_ht40_joint batch, mixed on the GPU as tests/test_gpu_tx_ht40.py::_loopback_captures mixes it: per frame H with
    random phases x GAIN, a carrier offset, a lead of 300..900 zero samples; per capture 800 trailing zeros, noise of sigma 8, int16, whole 28-sample bursts.
    -> (iq0, iq1 CUDA int16, descs, truth per capture [(mcs, gi, psdus, first sample in the capture, nsym)])"""
    torch, sora = env
    flat = [f for cap in specs for f in cap]
    mp = [[rng.integers(0, 256, ln, dtype=np.uint8).tobytes() for _ in range(1 if joint else 2)] for _, ln, _ in flat]
    mcs = [f[0] for f in flat]; gi = [f[2] for f in flat]
    if joint:
        o0, o1, off = sora.tx_ht40_joint([p[0] for p in mp], mcs, [int(rng.integers(1, 128)) for _ in flat], gi=gi)
    else:
        o0, o1, off = sora.tx_ht40([p[0] for p in mp], [p[1] for p in mp], mcs, [(int(rng.integers(1, 128)), int(rng.integers(1, 128))) for _ in flat], gi=gi)
    x = torch.stack([torch.complex(o[:, 0].double(), o[:, 1].double()) for o in (o0, o1)])
    gen = torch.Generator(device="cuda"); gen.manual_seed(int(rng.integers(1 << 30)))
    parts, descs, truth, pos, k = [], [], [], 0, 0
    for ci, cap in enumerate(specs):
        segs, want, at = [], [], 0
        for f_mcs, ln, f_gi in cap:
            ph = rng.uniform(0, 2 * np.pi, 4)
            H = np.array([[1.0 * np.exp(1j * ph[0]), 0.3 * np.exp(1j * ph[1])], [0.25 * np.exp(1j * ph[2]), 0.9 * np.exp(1j * ph[3])]]) * GAIN
            xf = x[:, off[k]:off[k + 1]]
            y = torch.stack([complex(H[r, 0]) * xf[0] + complex(H[r, 1]) * xf[1] for r in range(2)])
            if cfo_step:
                y = y * torch.exp(1j * 2 * np.pi * cfo_step / 65536.0 * torch.arange(y.shape[1], device="cuda", dtype=torch.float64))[None]
            lead = int(rng.integers(300, 900))
            segs += [torch.zeros((2, lead), dtype=torch.complex128, device="cuda"), y]
            nsym = (y.shape[1] - 1600) // (144 if f_gi else 160)
            want.append((f_mcs, f_gi, [m.add_fcs(p) for p in mp[k]], at + lead, nsym)); at += lead + y.shape[1]; k += 1
        y = torch.cat(segs + [torch.zeros((2, 800), dtype=torch.complex128, device="cuda")], dim=1)
        y = torch.view_as_real(y) + 8.0 * torch.randn(y.shape + (2,), generator=gen, device="cuda", dtype=torch.float64)
        y = torch.clamp(torch.round(y), -32768, 32767).to(torch.int16)
        n = y.shape[1] // 28 * 28
        parts.append(y[:, :n]); descs.append((pos, n, 100 + ci)); truth.append(want); pos += n
    iq = torch.cat(parts, dim=1)
    return iq[0].contiguous(), iq[1].contiguous(), descs, truth


@pytest.mark.parametrize("joint", [False, True], ids=["per-stream", "joint"])
@pytest.mark.parametrize("cfo_step", [0.0, 21.0])
def test_loopback_of_mixed_kinds_through_the_raw_capture_receiver(env, cfo_step, joint):
    torch, sora = env
    rng = np.random.default_rng(717 + int(cfo_step) + joint)
    specs = [[(mcs, int(rng.integers(40, 300)), (mcs + 1) & 1), (8 + (mcs + 3) % 7, int(rng.integers(40, 200)), mcs & 1)] + ([(8 + (mcs + 5) % 7, 64, 1)] if mcs % 2 else [])
             for mcs in range(8, 15)]
    iq0, iq1, descs, truth = loopback(env, rng, specs, cfo_step, joint)
    rx = sora.RxHt40(64, 1 << 20)
    rx.set_coding(int(joint)); rx.set_guard(1)
    t = rx.process_captures_dev(iq0, iq1, descs, max_frames_per_capture=4)
    res = rx.results(ticket=t)
    rx.close()
    per = {}
    for r in res:
        per.setdefault(r["capture_id"], []).append(r)
    jpf = 1 if joint else 2
    for ci, want in enumerate(truth):
        got = per.get(100 + ci, [])
        exp = [(mcs, s, ps[s], gi) for mcs, gi, ps, _, _ in want for s in range(jpf)]
        assert len(got) == len(exp), (cfo_step, ci, [(hex(r["error_code"]), r["rate_kbps"], r["stream"]) for r in got])
        for r, e in zip(got, exp):
            assert (r["error_code"], r["rate_kbps"], r["stream"], r["mpdu"], r["flags"]) == (1, e[0], e[1], e[2], ROW_SHORT_GI if e[3] else 0), \
                   (cfo_step, ci, hex(r["error_code"]), r["rate_kbps"], r["stream"], r["flags"])
    if not joint:
        # the level and the noise are ones at which the float64 receiver decodes every frame too, the short ones re-spaced (back to front, so that positions hold)
        h0, h1 = iq0.cpu().numpy(), iq1.cpu().numpy()
        for d, want in zip(descs, truth):
            cap = np.stack([h0[d[0]:d[0] + d[1]], h1[d[0]:d[0] + d[1]]])
            for mcs, gi, ps, at, nsym in reversed(want):
                if gi:
                    cap = TG.respace(cap, nsym, at + 1280)
            frames = rx64.receive(cap)
            assert [(f.sig_ok, f.mcs, f.fcs_ok, f.psdu) for f in frames] == [(True, mcs, [True, True], ps) for mcs, _, ps, _, _ in want], (cfo_step, d[2])
