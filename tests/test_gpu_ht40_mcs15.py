"""MCS 15 / code rate 5/6 on the 40 MHz HT receive handle (sora_ht40_set_mcs_max(15)) held to tests/ht40_mcs15_model.py.

Descriptor calls: every soft byte (sora_ht40_soft_of), every row field and every PSDU byte, in both codings, long and short guard interval, N_BPSC 1 and 6 at rate
5/6, frames of 1, 2 and 12 symbols, cfo 0 / 37 / -511, and a rate-5/6 frame in every position of a four-frame workgroup beside frames of rates 0..2 (the job table's
fourth list beside the other three).  The weights are the handle's own exported d_weights, as in tests/test_gpu_ht40_soft.py.  A default handle still refuses rate 3.

Raw captures: the front end's records (sora_ht40_found_of), the rows and the delivery against the front model with the gate as a parameter -- on the existing
capture families with the gate at 14 (today's results: MCS 15 in HT-SIG is a header failure) and at 15 (the same captures; `gate mcs15` is now a recorded frame), and on
captures that hold real MCS 15 frames, which must come out FRAME_OK with the bytes that were sent; the raw-capture call's rows equal the descriptor call's on the
translated records, which is held to the data-field model byte for byte; one MCS 15 capture fed in pieces in stream mode equals the one-call result."""
import functools

import numpy as np
import pytest

import ht40_front_captures as fc
import ht40_front_model as fm
import ht40_gi_cases as C
import ht40_mcs15_model as M
import ht40_soft_check as sc
from test_gpu_ht40_front import E_PLCP, check_records, check_rows_against_the_front_model, dev, raw_call

pytestmark = pytest.mark.gpu
CR_56, SHORT = 3, 0x100


@pytest.fixture(scope="module")
def env():
    import torch
    import sora_amd
    if sora_amd.device_count() <= 0:
        pytest.skip("no HIP device")
    return torch, sora_amd


# ------------------------------------------------------------------ descriptor calls
def make_frame(rng, nb, cr, nsym, gi, joint, cfo, nv, longer=0, sigma=6.0):
    with M.rate56():
        lens = C.lengths(rng, nb, cr, nsym, joint, longer)
        assert C.symbols(lens, nb, cr, joint) == nsym
        seg, ps = C.frame(rng, nb, cr, lens, gi, joint, sigma, cfo)
    return {"seg": seg, "nb": nb, "cr": cr, "lens": lens, "gi": gi, "cfo": cfo, "nv": nv, "ps": ps, "nsym": nsym}


@functools.lru_cache(maxsize=None)
def bank(joint):
    """sixteen frames, four workgroups: group g holds a rate-5/6 frame at position g (N_BPSC 1 / 6, 1 / 2 / 12 symbols, long / short, cfo 0 / 37 / -511, both detectors)
    and frames of rates 0..2 around it; then four more rate-5/6 frames that fill a workgroup of their own (the fourth list alone: N_BPSC 2 and 4 too)"""
    rng = np.random.default_rng(1500 + joint)
    out = []
    five = [(1, 1, 0, 0, 0.0), (6, 2, 1, 37, 3000.0), (6, 12, 0, -511, 0.0), (1, 12, 1, 37, 3000.0)]      # (nb, nsym, gi, cfo, noise_var)
    for g in range(4):
        for p in range(4):
            if p == g:
                nb, nsym, gi, cfo, nv = five[g]
                out.append(make_frame(rng, nb, CR_56, nsym, gi, joint, cfo, nv, longer=g & 1))
            else:
                nb = (2, 4, 6, 1)[(p + g) % 4]; cr = (p + 2 * g) % 3
                out.append(make_frame(rng, nb, cr, (2, 3, 2)[(p + g) % 3], (p + g) & 1, joint, (0, 37, -511)[(p + g) % 3], (0.0, 3000.0)[p & 1], longer=p & 1))
    for nb, nsym, gi, cfo in ((2, 2, 0, -511), (4, 1, 1, 0), (6, 1, 0, 37), (6, 2, 1, 0)):
        out.append(make_frame(rng, nb, CR_56, nsym, gi, joint, cfo, 0.0, longer=nb & 1))
    assert {out[4 * g + p]["cr"] == CR_56 for g in range(4) for p in range(4) if p == g} == {True}
    assert all({f["cr"] for f in out[4 * g:4 * g + 4]} >= {CR_56} and len({f["cr"] for f in out[4 * g:4 * g + 4]}) >= 3 for g in range(4))
    return out


def call(env, joint, iq, descs, frames, gate=15):
    torch, sora = env
    rx = sora.RxHt40(len(descs), C.capacity(frames))
    rx.set_coding(joint)
    if gate != 14:
        assert rx.set_mcs_max(gate) == 14
    w = torch.zeros((len(descs), 4, 128, 2), dtype=torch.int16, device="cuda")
    t = rx.process_dev(torch.from_numpy(iq[0].copy()).cuda(), torch.from_numpy(iq[1].copy()).cuda(), descs, w)
    rows = rx.results(ticket=t)
    soft = [rx.soft(f, 0, ticket=t) if joint else [rx.soft(f, s, ticket=t) for s in range(2)] for f in range(len(descs))]
    rx.close()
    return {"rows": rows, "soft": soft, "w": w.cpu().numpy()}


def models(joint, iq, descs, w):
    out = []
    for f, d in enumerate(descs):
        r = M.model(iq, d[0], d[1], d[2] & ~SHORT, d[3] if joint else (d[3], d[4]), d[5], w[f], gi=1 if d[2] & SHORT else 0, joint=bool(joint))
        out.append(C.JointWant(r) if joint else r)
    return out


def check(joint, got, want, descs, what):
    plain = [d[:2] + (d[2] & ~SHORT,) + d[3:] for d in descs]
    (sc.assert_is_the_joint_model if joint else sc.assert_is_the_model)(got, want, plain, what)
    per = 1 if joint else 2
    for f, d in enumerate(descs):
        for r in got["rows"][per * f:per * f + per]:
            assert r["flags"] == (C.ROW_SHORT_GI if d[2] & SHORT else 0) and r["rate_kbps"] == 10 * d[1] + (d[2] & ~SHORT), (what, f, r["flags"], r["rate_kbps"])


@pytest.mark.parametrize("joint", [0, 1], ids=["per_stream", "joint"])
def test_descriptor_calls_every_soft_byte_row_and_psdu(env, joint):
    frames = bank(joint)
    rng = np.random.default_rng(1510 + joint)
    iq, offs = C.place(rng, frames, (1, 3, 0, 2, 1))
    descs = C.descs(frames, offs)
    assert sum((d[2] & ~SHORT) == CR_56 for d in descs) == 8 and any(d[2] == (CR_56 | SHORT) for d in descs)
    got = call(env, joint, iq, descs, frames)
    want = models(joint, iq, descs, got["w"])
    check(joint, got, want, descs, "mixed rates")
    for f, fr in enumerate(frames):                                       # clean frames: the model, and so the GPU, decodes them
        if joint:
            assert want[f].error_code == 1 and want[f].psdu == fr["ps"][0], (f, fr["nb"], fr["cr"])
        else:
            assert [want[f].streams[s].psdu for s in range(2)] == fr["ps"] and all(want[f].streams[s].error_code == 1 for s in range(2)), (f, fr["nb"], fr["cr"])


@pytest.mark.parametrize("joint", [0, 1], ids=["per_stream", "joint"])
def test_small_batches_a_lone_rate_56_frame_an_odd_fourth_list_and_frames_that_fail(env, joint):
    frames = bank(joint)
    rng = np.random.default_rng(1520 + joint)
    five = [f for f in frames if f["cr"] == CR_56]
    noisy = make_frame(rng, 6, CR_56, 2, 0, joint, 0, 0.0, sigma=150.0)      # 64-QAM 5/6 at sigma 150 fails its FCS: rows and bytes of a FAILED frame are compared too
    for pick in ([five[0]], [five[1], five[4], noisy], [frames[1], five[2], frames[2], five[5], five[6]]):
        iq, offs = C.place(rng, pick, (1, 2, 3))
        descs = C.descs(pick, offs)
        got = call(env, joint, iq, descs, pick)
        check(joint, got, models(joint, iq, descs, got["w"]), descs, "batch of %d" % len(pick))
        if any(f is noisy for f in pick):
            assert any(r["error_code"] == 0x80000006 for r in got["rows"]), [hex(r["error_code"]) for r in got["rows"]]


def test_the_gate_and_a_default_handle(env):
    torch, sora = env
    z = torch.zeros((4096, 2), dtype=torch.int16, device="cuda")
    rx = sora.RxHt40(4, 4 * (2 * 108 * 6 + 64))
    assert rx.set_mcs_max() == 14 and rx.set_mcs_max(0) == 14 and rx.set_mcs_max(-3) == 14
    for cr in (CR_56, CR_56 | SHORT):
        with pytest.raises(sora.SoraError) as e:
            rx.process_dev(z, z, [(0, 6, cr, 30, 30, 0, 0.0, 0)])
        assert e.value.code == -1
    for bad in (13, 16, 1, 10):
        with pytest.raises(sora.SoraError) as e:
            rx.set_mcs_max(bad)
        assert e.value.code == -1 and "sora_ht40_set_mcs_max" in str(e.value)
    assert rx.set_mcs_max() == 14
    assert rx.set_mcs_max(15) == 14 and rx.set_mcs_max() == 15
    t = rx.process_dev(z, z, [(0, 6, CR_56 | SHORT, 30, 30, 0, 0.0, 9), (400, 1, CR_56, 30, 29, 0, 0.0, 10)])
    rows = rx.results(ticket=t)
    assert [(r["capture_id"], r["rate_kbps"], r["flags"], r["nsym"]) for r in rows] == [(9, 63, C.ROW_SHORT_GI, 1)] * 2 + [(10, 13, 0, -(-(16 + 240 + 6) // 90))] * 2
    for cr in (4, 4 | SHORT, 0x203):                                       # ... and nothing above it
        with pytest.raises(sora.SoraError):
            rx.process_dev(z, z, [(0, 6, cr, 30, 30, 0, 0.0, 0)])
    assert rx.set_mcs_max(14) == 15
    with pytest.raises(sora.SoraError):
        rx.process_dev(z, z, [(0, 6, CR_56, 30, 30, 0, 0.0, 0)])
    rx.close()
    assert sora.ht40_symbols(100, 90, 6, CR_56) == -(-(16 + 800 + 6) // 540) and sora.ht40_symbols_joint(4000, 6, CR_56) == 0
    assert sora.ht40_symbols(100, 90, 1, CR_56) == -(-(16 + 800 + 6) // 90) and sora.ht40_symbols(100, 90, 6, 4) == 0


# ------------------------------------------------------------------ raw captures
def mcs15_frame(rng, length, joint):
    with M.rate56():
        return fc.frame(rng, 15, length, joint)


@functools.lru_cache(maxsize=None)
def case_set(joint):
    """the existing families (a representative third, with `gate mcs15` among them) and captures that hold real MCS 15 frames: lengths on both sides of a symbol step,
    one and twelve symbols, a carrier offset, an MCS 15 frame between frames of other rates -> (captures, iq, descriptors)"""
    caps = fc.build(joint, full=False)
    assert any(c.name == "gate mcs15" for c in caps)
    rng = np.random.default_rng(1530 + joint)
    nd = 1080 if joint else 540
    step = (nd - 22) // 8                                                  # the longest PSDU of one symbol
    for name, L, kw in (("mcs15 len%d" % step, step, {}), ("mcs15 len%d" % (step + 1), step + 1, {}), ("mcs15 len4 cfo", 4 if not joint else 5, {"cfo_step": -37.25}),
                        ("mcs15 twelve symbols", (12 * nd - 22) // 8, {"H": fc.H_UNIT})):
        x, nsym, ps = mcs15_frame(rng, L, joint)
        pair = fc.gauss(fc.cat(fc.quiet(400), fc.through(x, kw.get("H", fc.H_MIX), kw.get("cfo_step", 0.0)), fc.quiet(600)), rng, 6.0)
        caps.append(fc.Cap(name, "mcs15", fc.each(fc.whole, pair), [{"mcs": 15, "length": L, "nsym": nsym, "htstf": 400 + fc.PRE - 160, "psdus": ps, "sound": True}], {"mcs15"}))
    parts, sent, pos = [fc.quiet(300)], [], 300
    for i, mcs in enumerate((14, 15, 9, 15)):
        L = 40 + 10 * i
        x, nsym, ps = mcs15_frame(rng, L, joint) if mcs == 15 else fc.frame(rng, mcs, L, joint)
        sent.append({"mcs": mcs, "length": L, "nsym": nsym, "htstf": pos + fc.PRE - 160, "psdus": ps, "sound": True})
        parts += [fc.through(x), fc.quiet(300)]; pos += x.shape[1] + 300
    caps.append(fc.Cap("four frames, two of them mcs15", "mcs15", fc.each(fc.whole, fc.gauss(fc.cat(*parts, fc.quiet(28 * 40)), rng, 6.0)), sent, {"mcs15"}))
    iq, descs = fc.layout(caps)
    return caps, iq, descs


def front_events(caps, joint, gate):
    return [M.front(c.iq[0], c.iq[1], mcs_max=gate, joint=joint) for c in caps]


def gated_call(env, f0, f1, descs, mf, joint, gate, max_soft=1 << 22):
    _, sora = env
    rx = sora.RxHt40(256, max_soft)
    if joint:
        rx.set_coding(sora.HT40_CODING_JOINT)
    if gate != 14:
        rx.set_mcs_max(gate)
    return raw_call(env, f0, f1, descs, mf, joint, rx=rx)


@pytest.mark.parametrize("joint", [False, True], ids=["per-stream", "joint"])
def test_raw_captures_with_the_gate_at_14_are_todays_results(env, joint):
    caps, iq, descs = case_set(joint)
    want = front_events(caps, joint, 14)
    f0, f1 = dev(env, iq)
    rx, t, got = gated_call(env, f0, f1, descs, fc.MAX_EVENTS, joint, 14)
    check_records([c.name for c in caps], got, want, fc.MAX_EVENTS, "gate 14")
    rows = rx.results(ticket=t)
    check_rows_against_the_front_model(rows, descs, want, fc.MAX_EVENTS, joint, "gate 14")
    rx.close()
    by = {c.name: w for c, w in zip(caps, want)}
    assert by["gate mcs15"][0]["error_code"] == E_PLCP and all(w and w[0]["error_code"] == E_PLCP for c, w in zip(caps, want) if c.family == "mcs15" and len(c.sent) == 1)
    assert not any(r["rate_kbps"] == 15 for r in rows)


@pytest.mark.parametrize("joint", [False, True], ids=["per-stream", "joint"])
def test_raw_captures_with_the_gate_at_15_records_rows_delivery_and_the_plan(env, joint):
    torch, sora = env
    caps, iq, descs = case_set(joint)
    mf = fc.MAX_EVENTS
    want = front_events(caps, joint, 15)
    want14 = front_events(caps, joint, 14)
    changed = [c.name for c, a, b in zip(caps, want, want14) if a != b]
    assert "gate mcs15" in changed and all(n == "gate mcs15" or n.startswith(("mcs15", "four frames")) for n in changed), changed
    f0, f1 = dev(env, iq)
    rx, t, got = gated_call(env, f0, f1, descs, mf, joint, 15)
    check_records([c.name for c in caps], got, want, mf, "gate 15")
    raw = rx.results(ticket=t)
    check_rows_against_the_front_model(raw, descs, want, mf, joint, "gate 15")
    # delivery: the same rows and bytes through sora_ht40_deliver_async
    key = lambda r: (r["capture_id"], r["stream"], r["end_sample"], r["error_code"], r["rate_kbps"], r["length"], r["nsym"], r["crc32"], r["flags"], r["mpdu"])
    buf = sora.HostResults(2 * mf * len(descs), 1 << 20)
    t2 = rx.process_captures_dev(f0, f1, descs, max_frames_per_capture=mf)
    rx.deliver_async(t2, buf); rx.wait(t2)
    assert [key(r) for r in buf.results()] == [key(r) for r in raw]
    buf.close()
    # the real MCS 15 frames come out FRAME_OK with the bytes that were sent
    jpf = 1 if joint else 2
    n15 = 0
    for c, d in zip(caps, descs):
        if c.family != "mcs15":
            continue
        rows = [r for r in raw if r["capture_id"] == d[2]]
        assert len(rows) == jpf * len(c.sent), (c.name, len(rows))
        for i, s in enumerate(c.sent):
            for k in range(jpf):
                r = rows[jpf * i + k]
                assert (r["error_code"], r["rate_kbps"], r["length"], r["mpdu"]) == (1, s["mcs"], s["length"], s["psdus"][k]), (c.name, i, k, hex(r["error_code"]))
                n15 += s["mcs"] == 15
    assert n15 >= 6 * jpf
    # the plan, by equivalence: the records -> descriptors by the stated rule, the descriptor call on the same buffers gives the raw-capture call's rows and bytes ...
    fdescs = [M.descriptor(d[0], r, float(r["noise_var"]), joint, d[2]) for d, g in zip(descs, got) for r in g if r["error_code"] == 0]
    assert sum(d[2] == CR_56 for d in fdescs) >= 7
    w = torch.zeros((len(fdescs), 4, 128, 2), dtype=torch.int16, device="cuda")
    td = rx.process_dev(f0, f1, fdescs, w)
    rows = rx.results(ticket=td)
    soft = [rx.soft(f, 0, ticket=td) if joint else [rx.soft(f, s, ticket=td) for s in range(2)] for f in range(len(fdescs))]
    rx.close()
    framed = [r for r in raw if r["error_code"] != E_PLCP]
    assert len(framed) == len(rows) == jpf * len(fdescs)
    for a, b in zip(framed, rows):
        nb, cr = (6, CR_56) if a["rate_kbps"] == 15 else fm.MCS2[a["rate_kbps"]]
        assert (a["stream"], a["error_code"], a["length"], a["crc32"], a["nsym"], 10 * nb + cr, a["capture_id"], a["mpdu"]) == \
               (b["stream"], b["error_code"], b["length"], b["crc32"], b["nsym"], b["rate_kbps"], b["capture_id"], b["mpdu"]), (a["capture_id"], a["stream"])
    # ... and that descriptor call is the data-field model's, every soft byte, row field and PSDU byte (`gate mcs15`: a frame that fails, compared too)
    got_d = {"rows": rows, "soft": soft, "w": w.cpu().numpy()}
    check(joint, got_d, models(joint, iq, fdescs, got_d["w"]), fdescs, "translated records")


def test_an_mcs15_capture_fed_in_pieces_leaves_the_uncut_captures_records_and_rows(env):
    _, sora = env
    caps, _, _ = case_set(False)
    c = next(c for c in caps if c.name == "four frames, two of them mcs15")
    want = M.front(c.iq[0], c.iq[1], mcs_max=15)
    assert len(want) == 4 and [e["mcs"] for e in want] == [14, 15, 9, 15] and all(e["error_code"] == 0 for e in want)
    n = len(c.iq[0])
    f0, f1 = dev(env, np.stack(c.iq))
    uncut, tu, ref = gated_call(env, f0, f1, [(0, n, 3)], 8, False, 15, max_soft=1 << 18)
    check_records([c.name], ref, [want], 8, "uncut")
    key = lambda r: (r["stream"], r["error_code"], r["rate_kbps"], r["length"], r["nsym"], r["crc32"], r["mpdu"])
    ref_rows = [key(r) for r in uncut.results(ticket=tu)]
    uncut.close()
    assert len(ref_rows) == 8 and all(k[1] == 1 for k in ref_rows)
    htstf = [s["htstf"] for s in c.sent]
    for cuts in ((28 * 40, 28 * ((htstf[1] + 400) // 28), 28 * ((htstf[1] + 1700) // 28)), (28 * ((htstf[1] - 600) // 28), 28 * ((htstf[3] + 200) // 28))):
        rx = sora.RxHt40(8, 1 << 18)
        assert rx.set_stream_mode(1) == 0 and rx.set_mcs_max(15) == 14
        pos, got, rows = 0, [], []
        for end in cuts + (n,):
            t = rx.process_captures_dev(f0[pos:], f1[pos:], [(0, end - pos, 3)], max_frames_per_capture=8)
            rx.wait(t)
            for r in rx.found(0, ticket=t):                                # a20 and end_sample count from the piece's first sample
                got.append(dict(r, a20=r["a20"] + pos // 2, end_sample=r["end_sample"] + pos))
            rows += [key(r) for r in rx.results(ticket=t)]
            used = int(rx.stream_consumed(t, 1)[0])
            assert used % 28 == 0 and used <= end - pos
            pos += used
        rx.close()
        check_records([c.name], [got], [want], 8, "cut at %r" % (cuts,))
        assert rows == ref_rows, cuts
