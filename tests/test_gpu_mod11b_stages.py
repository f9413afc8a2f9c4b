"""The stage entry points of the 802.11b modulation graph on the GPU (-m gpu): every stage against tests/mod11b_model.py bit for bit, output AND state record, over
batches of independent streams whose lengths sit on the kernels' edges (one lane's run, one workgroup pass T and its neighbours, several passes, the longest PPDU),
whose offsets are odd and begin on and off 16-byte boundaries, and whose records enter in every state the bricks distinguish.  Output buffers are pre-filled and
compared whole: what lies between and behind the streams stays as it was.  Each stateful stage is also run over one stream as two calls, and the composition
mod11b_by_stages is held to the fused transmitter."""
import os
import re

import numpy as np
import pytest

import mod11b_model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = int(re.search(r"constexpr int kMod11bT = (\d+);", open(os.path.join(ROOT, "sora_amd", "csrc", "kernels.h")).read()).group(1))
LENGTHS = [1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T + 3, 4120]                   # 4120: the longest PPDU (24 + 4092 + 4)
FILL = 0x5A
BYTES = np.random.default_rng(1301).integers(0, 256, 70000).astype(np.uint8)     # the streams' bytes: slices of one array
SPREADERS = {"dbpsk": (88, "dbpsk_spread11b"), "dqpsk": (44, "dqpsk_spread11b"), "cck5": (16, "cck5_encode11b"), "cck11": (8, "cck11_encode11b")}


@pytest.fixture(scope="module")
def sora():
    import sora_amd
    sora_amd.load()
    return sora_amd


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def i32(v):
    return dev(np.asarray(v, np.int32))


def batches():
    """-> [(name, lengths)]: one stream at every edge length; three; 65 of mixed lengths with one of 0"""
    mixed = [LENGTHS[(5 * f) % len(LENGTHS)] if f % 9 else [1, 2, 3, 7, 15, 16, 17, 33][f // 9] for f in range(65)]
    mixed[41] = 0
    return [("1 x %d" % n, [n]) for n in LENGTHS] + [("3", [T + 1, 65, 2 * T + 3]), ("65", mixed)]


def layout(lengths, out_per_unit, elem_bytes, seed):
    """input offsets (odd) and output offsets in elements: odd ones, and ones that fall on and off a 16-byte boundary -> (first, out_first, input size, output size)"""
    rng = np.random.default_rng(seed)
    per16 = 16 // elem_bytes
    first, out_first, at, oat = [], [], 1, 0
    for f, n in enumerate(lengths):
        at += int(rng.integers(0, 3)) * 2 + (1 - at % 2)                         # odd
        first.append(at); at += n
        oat += int(rng.integers(1, 5))
        kind = (f + seed) % 3
        if kind == 0: oat = -(-oat // per16) * per16                             # on a boundary
        elif kind == 1: oat += 1 - oat % 2                                       # odd
        else: oat = -(-oat // per16) * per16 + (per16 // 2 if per16 > 2 else 1)  # off it, even where the element allows
        out_first.append(oat); oat += n * out_per_unit
    return first, out_first, at + 5, oat + 37


def mod_states(n, seed):
    """[n, 4] records: every last_phase and is_even, some with bits set above the ones the bricks read, sentinels in the reserved words"""
    rng = np.random.default_rng(seed)
    s = np.zeros((n, 4), np.int32)
    s[:, 0] = np.arange(n) % 4 + 4 * (np.arange(n) % 5 == 4)                     # (the low two bits are read)
    s[:, 1] = (np.arange(n) // 4) % 2 + 2 * (np.arange(n) % 7 == 6)              # (the low bit is read)
    s[:, 2:] = rng.integers(1, 1 << 30, (n, 2))
    return s


def spread_model(kind, data, rec):
    """-> (chips, record after)"""
    rec = rec.copy()
    if len(data) == 0:
        return np.zeros((0, 2), np.int8), rec
    if kind == "dbpsk": c, rec[0] = M.dbpsk_spread(data, int(rec[0]))
    elif kind == "dqpsk": c, rec[0] = M.dqpsk_spread(data, int(rec[0]))
    elif kind == "cck5": c, rec[0] = M.cck5_encode(data, int(rec[0]))
    else: c, rec[0], rec[1] = M.cck11_encode(data, int(rec[0]), int(rec[1]))
    return c, rec


@pytest.mark.parametrize("kind", sorted(SPREADERS))
def test_spreaders_equal_the_models_output_and_record(sora, kind):
    cpb, fn = SPREADERS[kind]
    for bi, (name, lengths) in enumerate(batches()):
        first, out_first, nin, nout = layout(lengths, cpb, 2, bi)
        x = BYTES[:nin]
        state = mod_states(len(lengths), bi)
        if len(lengths) == 1:
            state[0, 0] = bi % 4; state[0, 1] = bi // 4 % 2                      # (ten single streams: every phase and parity comes by)
        want = np.full((nout, 2), FILL, np.int8); wstate = state.copy()
        for f, n in enumerate(lengths):
            c, wstate[f] = spread_model(kind, bytes(x[first[f]:first[f] + n]), state[f])
            want[out_first[f]:out_first[f] + n * cpb] = c
        out = dev(np.full((nout, 2), FILL, np.int8)); d_state = dev(state)
        getattr(sora, fn)(dev(x), i32(first), i32(lengths), i32(out_first), d_state, out)
        got = out.cpu().numpy()
        assert np.array_equal(got, want), (kind, name, np.flatnonzero((got != want).any(axis=1))[:8])
        assert np.array_equal(d_state.cpu().numpy(), wstate), (kind, name)


def test_dbpsk_reads_one_bit_of_last_phase(sora):
    """1 like 3 and 2 like 0: four streams of the same bytes"""
    n = 65
    x = dev(BYTES[:n]); out = dev(np.zeros((4 * 88 * n, 2), np.int8)); state = dev(np.array([[p, 0, 0, 0] for p in range(4)], np.int32))
    sora.dbpsk_spread11b(x, i32([0] * 4), i32([n] * 4), i32([88 * n * p for p in range(4)]), state, out)
    o = out.cpu().numpy().reshape(4, -1); s = state.cpu().numpy()
    assert np.array_equal(o[1], o[3]) and np.array_equal(o[2], o[0]) and not np.array_equal(o[0], o[1])
    assert np.array_equal(s[1], s[3]) and np.array_equal(s[2], s[0]) and set(s[:, 0]) <= {0, 3}


def test_sc741_equals_the_model_output_and_register(sora):
    regs = [0x6C, 0x1B, 0x00, 0x7F, 0x80 | 0x1B]                                 # (the last: only seven bits are read)
    for bi, (name, lengths) in enumerate(batches()):
        first, out_first, nin, nout = layout(lengths, 1, 1, 100 + bi)
        x = BYTES[:nin]
        reg = np.array([regs[(f + bi) % len(regs)] for f in range(len(lengths))], np.int32)
        want = np.full(nout, FILL, np.uint8); wreg = reg.copy()
        for f, n in enumerate(lengths):
            if n:
                o, wreg[f] = M.sc741(bytes(x[first[f]:first[f] + n]), int(reg[f]))
                want[out_first[f]:out_first[f] + n] = np.frombuffer(o, np.uint8)
        out = dev(np.full(nout, FILL, np.uint8)); d_reg = dev(reg)
        sora.sc741_11b(dev(x), i32(first), i32(lengths), i32(out_first), d_reg, out)
        got = out.cpu().numpy()
        assert np.array_equal(got, want), (name, np.flatnonzero(got != want)[:8])
        assert np.array_equal(d_reg.cpu().numpy(), wreg), name


def shaper_inputs():
    rng = np.random.default_rng(1302)
    unit = np.array([(1, 0), (0, 1), (-1, 0), (0, -1)], np.int8)[rng.integers(0, 4, 70000)]
    full = rng.integers(-128, 128, (70000, 2)).astype(np.int8)
    full[::97] = (-128, 127); full[50::89] = (127, -128); full[0] = (-128, -128)
    return {"unit": unit, "full": full}


def shaper_records(n, seed):
    """the zero record, one a previous call left, and random ones"""
    rng = np.random.default_rng(seed)
    left = M.quick_shape_loop(rng.integers(-128, 128, (9, 2)).astype(np.int8), np.zeros((4, 4, 2), np.int16))[1]
    recs = np.zeros((n, 4, 4, 2), np.int16)
    for f in range(n):
        if f % 3 == 1: recs[f] = left
        elif f % 3 == 2: recs[f] = rng.integers(-32768, 32768, (4, 4, 2))
    return recs


@pytest.mark.parametrize("chips", ["unit", "full"])
def test_pulse_shaper_equals_the_model_output_and_record(sora, chips):
    src = shaper_inputs()[chips]
    for bi, (name, lengths) in enumerate(batches()):
        flush = [(f + bi) % 2 for f in range(len(lengths))]                      # on and off in one call
        first, out_first, nin, _ = layout(lengths, 1, 2, 200 + bi)
        _, out_first, _, nout = layout([n + 5 * fl for n, fl in zip(lengths, flush)], 4, 4, 300 + bi)
        x = src[:nin]
        recs = shaper_records(len(lengths), bi + (3 if len(lengths) == 1 else 0))
        if len(lengths) == 1:
            recs[0] = shaper_records(3, bi)[bi % 3]
        want = np.full((nout, 2), FILL * 257, np.int16); wrecs = recs.copy()
        for f, n in enumerate(lengths):
            if n or flush[f]:
                o, wrecs[f] = M.pulse_shape(x[first[f]:first[f] + n], recs[f], bool(flush[f]))
                want[out_first[f]:out_first[f] + len(o)] = o
        out = dev(np.full((nout, 2), FILL * 257, np.int16)); d_rec = dev(recs.reshape(len(lengths), 32).view(np.int32))
        sora.pulse_shape11b(dev(x), i32(first), i32(lengths), i32(out_first), d_rec, out, flush=dev(np.asarray(flush, np.uint8)))
        got = out.cpu().numpy()
        assert np.array_equal(got, want), (chips, name, np.flatnonzero((got != want).any(axis=1))[:8])
        assert np.array_equal(d_rec.cpu().numpy().view(np.int16).reshape(-1, 4, 4, 2), wrecs), (chips, name)


def test_pulse_shaper_without_a_flush_table(sora):
    x = shaper_inputs()["full"][:T + 1]
    want, wrec = M.pulse_shape(x, np.zeros((4, 4, 2), np.int16))
    out = dev(np.zeros((4 * (T + 1), 2), np.int16)); rec = dev(np.zeros((1, 16), np.int32))
    sora.pulse_shape11b(dev(x), i32([0]), i32([T + 1]), i32([0]), rec, out)
    assert np.array_equal(out.cpu().numpy(), want) and np.array_equal(rec.cpu().numpy().view(np.int16).reshape(4, 4, 2), wrec)


# ---- one stream as two calls
N_CUT = 2 * T + 3
CUTS = [1, 777, T, N_CUT - 1]                                                    # 777: an odd byte (TCCK11Encode's parity)


@pytest.mark.parametrize("stage", ["sc741"] + sorted(SPREADERS))
def test_a_byte_stream_as_two_calls_is_the_stream_in_one(sora, stage):
    cpb, fn = SPREADERS.get(stage, (1, "sc741_11b"))
    x = dev(BYTES[3:3 + N_CUT])

    def run(parts, rec):
        import torch
        out = torch.full((N_CUT * cpb + 8, 2) if stage != "sc741" else (N_CUT + 8,), FILL, dtype=torch.int8 if stage != "sc741" else torch.uint8, device="cuda")
        d_rec = dev(rec)
        for a, n in parts:
            getattr(sora, fn)(x, i32([a]), i32([n]), i32([3 + a * cpb]), d_rec, out)
        return out.cpu().numpy(), d_rec.cpu().numpy()

    for rec in ([np.array([0x6C], np.int32), np.array([0x1B], np.int32)] if stage == "sc741" else [np.array([[p, p & 1, 7, 9]], np.int32) for p in range(4)]):
        whole, wrec = run([(0, N_CUT)], rec)
        if stage == "sc741":
            o, r = M.sc741(bytes(BYTES[3:3 + N_CUT]), int(rec[0]))
            assert np.array_equal(whole[3:3 + N_CUT], np.frombuffer(o, np.uint8)) and wrec[0] == r
        else:
            c, r = spread_model(stage, bytes(BYTES[3:3 + N_CUT]), rec[0])
            assert np.array_equal(whole[3:3 + N_CUT * cpb], c) and np.array_equal(wrec[0], r)
        for cut in CUTS:
            got, grec = run([(0, cut), (cut, N_CUT - cut)], rec)
            assert np.array_equal(got, whole) and np.array_equal(grec, wrec), (stage, rec, cut)


def test_a_chip_stream_as_two_calls_is_the_stream_in_one(sora):
    import torch
    x = dev(shaper_inputs()["full"][5:5 + N_CUT])
    for rec in shaper_records(3, 7):
        def run(parts):
            out = torch.full((4 * (N_CUT + 5) + 9, 2), FILL, dtype=torch.int16, device="cuda")
            d_rec = dev(rec.reshape(1, 32).view(np.int32))
            for a, n, fl in parts:
                sora.pulse_shape11b(x, i32([a]), i32([n]), i32([1 + 4 * a]), d_rec, out, flush=dev(np.asarray([fl], np.uint8)))
            return out.cpu().numpy(), d_rec.cpu().numpy()
        whole, wrec = run([(0, N_CUT, 1)])
        o, r = M.pulse_shape(x.cpu().numpy(), rec, True)
        assert np.array_equal(whole[1:1 + len(o)], o) and np.array_equal(wrec.view(np.int16).reshape(4, 4, 2), r)
        for cut in CUTS:
            got, grec = run([(0, cut, 0), (cut, N_CUT - cut, 1)])
            assert np.array_equal(got, whole) and np.array_equal(grec, wrec), cut
        got, grec = run([(0, N_CUT, 0), (N_CUT, 0, 1)])                          # Flush as a call of its own
        assert np.array_equal(got, whole) and np.array_equal(grec, wrec)


# ---- TBB11bSrc
def test_ppdu_equals_the_model_and_leaves_a_refused_frame_alone(sora):
    import tx11b_model as txm
    rng = np.random.default_rng(1303)
    frames = [(rate, kind, ln) for kind in (0, 1) for rate in (1000, 2000, 5500, 11000) for ln in (1, 37, 1500, 4092)]    # (1000, short) is refused: four of them
    frames += [(3000, 0, 37), (2000, 2, 37), (2000, 0, 0), (11000, 0, 4093)]
    mp = [rng.integers(0, 256, ln).astype(np.uint8) for _, _, ln in frames]
    off = np.cumsum([0] + [len(m) + 1 for m in mp])[:-1]                        # (MPDUs at any byte offset)
    blob = np.zeros(int(off[-1]) + 4200, np.uint8)
    for o, m in zip(off, mp):
        blob[o:o + len(m)] = m
    room = [24 + ln + 4 for _, _, ln in frames]
    out_first = np.cumsum([3] + [r + 1 + f % 2 for f, r in enumerate(room)])[:-1]   # odd, even, on and off boundaries as they come
    want = np.full(int(out_first[-1]) + room[-1] + 16, FILL, np.uint8)
    accepted = 0
    for f, (rate, kind, ln) in enumerate(frames):
        if txm.samples(ln, rate, kind):
            b = np.frombuffer(M.ppdu(bytes(mp[f]), rate, kind), np.uint8)
            assert len(b) == (24 if kind == 0 else 15) + ln + 4
            want[out_first[f]:out_first[f] + len(b)] = b; accepted += 1
        assert sora.tx11b_samples(ln, rate, kind) == txm.samples(ln, rate, kind)
    assert accepted == 28 and len({o % 16 for o in out_first}) > 8
    out = dev(np.full(len(want), FILL, np.uint8))
    sora.ppdu11b(dev(blob), i32(off), i32([ln for _, _, ln in frames]), i32([r for r, _, _ in frames]), dev(np.asarray([k for _, k, _ in frames], np.uint8)), out, i32(out_first))
    got = out.cpu().numpy()
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]


# ---- the composition
def test_the_stages_composed_are_the_fused_transmitter(sora):
    rng = np.random.default_rng(1304)
    frames = [(1000, 0, 1), (2000, 0, 2), (5500, 0, 37), (11000, 0, 150), (2000, 1, 1), (5500, 1, 301), (11000, 1, 700), (1000, 0, 1500), (2000, 1, 1500), (5500, 0, 1500),
              (11000, 1, 1500), (11000, 0, 13)]
    mp = [rng.integers(0, 256, ln).astype(np.uint8).tobytes() for _, _, ln in frames]
    rates = [r for r, _, _ in frames]; kinds = [k for _, k, _ in frames]; phase_in = [f % 4 for f in range(len(frames))]
    want, woff, wphase = sora.tx11b(mp, rates, phase_in=phase_in, return_phase=True, preamble=kinds)
    got, off, phase = sora.mod11b_by_stages(mp, rates, phase_in=phase_in, preamble=kinds)
    assert off == woff and phase == wphase
    g, w = got.cpu().numpy(), want.cpu().numpy()
    assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), np.flatnonzero((g != w).any(axis=1))[:8]
    got, off, phase = sora.mod11b_by_stages(mp[:4], rates[:4])                   # no preamble table, no phase_in: sora_hip_tx11b's frames
    want, woff, wphase = sora.tx11b(mp[:4], rates[:4], return_phase=True)
    assert off == woff and phase == wphase and np.array_equal(got.cpu().numpy(), want.cpu().numpy())
