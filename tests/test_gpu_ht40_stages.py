"""The 40 MHz HT receiver's stage entry points on the GPU (sora_hip_*_ht40, k_ht40_stages.hip), each held BIT FOR BIT to the per-brick model tests/ht40_stage_model.py
(itself held to oracle/ht40_data_model.py without a GPU in tests/test_ht40_stage_model_cpu.py): outputs, the theta words of the record, the record's other words and
every output word a stage does not own.  Shapes are the smallest that reach every path: 1, 3, 4, 5 and 67 symbols per call (a 32-lane group, a wave and a workgroup
partly filled), first samples 0, 1, 2, 3, 5, 63, 65 and a last symbol that ends the buffer, buffers that are and are not 16-byte aligned, frame-index tables that repeat
and skip, inputs at the rails, constants, zeros and uniform noise at 30 and 32767.  The composition sora_amd.rx_ht40_by_stages equals the handle (sora_ht40_process_dev)
in every soft byte, row field, PSDU byte and occupied-carrier weight, for both codings, frames that fail their FCS included."""
import numpy as np
import pytest

from oracle import ht40_data_model as dm
from oracle import py_ht40 as m
import ht40_joint_model as J
import ht40_stage_model as sm
from ht40_soft_check import soft_capacity, joint_soft_capacity
from test_ht40_data_model import send, H0

pytestmark = pytest.mark.gpu
COUNTS = (1, 3, 4, 5, 67)
SENTINEL = 0x5A5A
REST = np.setdiff1d(np.arange(128), sm.OCC)


@pytest.fixture(scope="module")
def env():
    import torch
    import sora_amd
    if sora_amd.device_count() <= 0:
        pytest.skip("no HIP device")
    return torch, sora_amd


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def i32(torch, a):
    return dev(torch, np.asarray(a, np.int64).astype(np.uint32).view(np.int32))


def levels(rng, shape):
    """one int16 array of `shape` (first axis = symbols / frames) whose rows cycle through: uniform noise at 30, at 32767, the two rails at random, +rail, -rail, a
    constant, zeros"""
    out = np.zeros(shape, np.int16)
    for i in range(shape[0]):
        k = i % 7
        if k == 0: out[i] = rng.integers(-30, 31, shape[1:])
        elif k == 1: out[i] = rng.integers(-32767, 32768, shape[1:])
        elif k == 2: out[i] = np.array([-32768, 32767], np.int16)[rng.integers(0, 2, shape[1:])]
        elif k == 3: out[i] = 32767
        elif k == 4: out[i] = -32768
        elif k == 5: out[i] = 1234
    return out


def misaligned(torch, a, elems=1):
    """the same values in a device buffer that starts 4 bytes (one sample) behind a 16-byte boundary; a byte array: 1 byte behind a 4-byte boundary"""
    a = np.ascontiguousarray(a)
    pad = elems if a.dtype == np.uint8 else 2 * elems
    buf = torch.zeros(a.size + pad, dtype=dev(torch, a.reshape(-1)[:1]).dtype, device="cuda")
    buf[pad:] = dev(torch, a.reshape(-1))
    out = buf[pad:].reshape(a.shape)
    assert out.data_ptr() % (4 if a.dtype == np.uint8 else 16) != 0
    return out


# ------------------------------------------------------------------ data_symbol_ht40
def test_data_symbol(env):
    torch, sora = env
    rng = np.random.default_rng(1)
    firsts = [0, 1, 2, 3, 5, 63, 65]; nsyms = [1, 2, 3, 12, 1, 2, 3]
    pos = 0; first = []
    for f, n in zip(firsts, nsyms):
        pos = (pos + 63) // 64 * 64 + f; first.append(pos); pos += 160 * n
    total = first[-1] + 160 * nsyms[-1]                                          # the last symbol ends the buffer
    x = [levels(rng, (total, 2)), rng.integers(-32768, 32768, (total, 2)).astype(np.int16)]
    out_first = np.array([20, 0, 2, 5, 19, 17, 21]); nout = 25                 # out of order, no two frames on one symbol, symbol 24 nobody's
    owned = np.concatenate([np.arange(o, o + n) for o, n in zip(out_first, nsyms)])
    assert len(set(owned.tolist())) == len(owned) == 24 and owned.max() == 23
    for mis in (0, 1):
        d = [misaligned(torch, c, mis) if mis else dev(torch, c) for c in x]
        o = [torch.full((nout * 128, 2), SENTINEL, dtype=torch.int16, device="cuda") for _ in range(2)]
        sora.data_symbol_ht40(d[0], d[1], i32(torch, first), i32(torch, nsyms), i32(torch, out_first), o[0], o[1])
        for c in range(2):
            want = np.full((nout * 128, 2), SENTINEL, np.int16)
            for a, n, of in zip(first, nsyms, out_first):
                want[128 * of:128 * (of + n)] = sm.data_symbol(x[c][a:a + 160 * n], n)
            assert np.array_equal(o[c].cpu().numpy(), want), (mis, c)
    # max_nsym bounds nothing away when it is the maximum; a count of 0 among the frames writes nothing
    o = [torch.full((nout * 128, 2), SENTINEL, dtype=torch.int16, device="cuda") for _ in range(2)]
    d = [dev(torch, c) for c in x]
    sora.data_symbol_ht40(d[0], d[1], i32(torch, first), i32(torch, [0] * 7), i32(torch, out_first), o[0], o[1], max_nsym=12)
    assert (o[0].cpu().numpy() == SENTINEL).all() and (o[1].cpu().numpy() == SENTINEL).all()


# ------------------------------------------------------------------ mimo_est_ht40
@pytest.fixture(scope="module")
def ltfs():
    """67 frames' HT-LTF pairs after the FFT: levels, and frames with equal chains (a singular channel matrix on every carrier) and an all-zero frame"""
    rng = np.random.default_rng(2)
    l0 = levels(rng, (67, 256, 2)); l1 = levels(rng, (67, 256, 2))[::-1].copy()
    l0[8:16] = rng.integers(-3000, 3001, (8, 256, 2)); l1[8:16] = rng.integers(-3000, 3001, (8, 256, 2))     # (the channel of a real frame: well-conditioned)
    l1[16] = l0[16]                                                            # singular: both chains alike
    l0[17] = 0; l1[17] = 0
    return l0, l1


@pytest.mark.parametrize("n", COUNTS)
def test_mimo_est(env, ltfs, n):
    torch, sora = env
    l0, l1 = ltfs[0][:n], ltfs[1][:n]
    nvs = {"null": None, "zero": np.zeros(n, np.float32), "3000": np.full(n, 3000.0, np.float32), "mixed": np.array([0.0, 3000.0, 0.4, 1e9, 7.5] * 14, np.float32)[:n]}
    differing = 0
    for name, nv in nvs.items():
        h, w = sora.mimo_est_ht40(dev(torch, l0), dev(torch, l1), dev(torch, nv) if nv is not None else None)
        _, w2 = sora.mimo_est_ht40(dev(torch, l0), dev(torch, l1), dev(torch, nv) if nv is not None else None, want_h=False)
        h, w, w2 = h.cpu().numpy(), w.cpu().numpy(), w2.cpu().numpy()
        assert np.array_equal(w, w2)
        assert not h[:, :, REST].any() and not w[:, :, REST].any()             # the 14 bins outside the occupied carriers: defined, 0
        for f in range(n):
            s2 = 0.0 if nv is None else float(nv[f])
            wh, ww = sm.mimo_est(l0[f], l1[f], s2)
            assert np.array_equal(h[f], wh), (name, f)
            if s2 == 0.0:
                assert np.array_equal(w[f], ww), (name, f)                     # TMimoChannelEst's own inverse: bit for bit
            else:
                differing += int(np.sum(w[f] != ww))
                assert np.abs(w[f].astype(int) - ww.astype(int)).max() <= 1, (name, f)
    print("mimo_est_ht40, n = %d: MMSE weights that differ from the float32 numpy restatement: %d" % (n, differing))
    assert differing == 0, differing
    if n >= 17:
        sat = int(np.sum(np.abs(w.astype(int)) >= 32767))
        assert sat > 0                                                         # quiet and singular frames: saturated weights are part of the comparison


# ------------------------------------------------------------------ mimo_comp_ht40
@pytest.mark.parametrize("n", COUNTS)
def test_mimo_comp(env, n):
    torch, sora = env
    rng = np.random.default_rng(3 + n)
    w = np.stack([rng.integers(-32768, 32768, (4, 128, 2)), rng.integers(-600, 601, (4, 128, 2)), np.full((4, 128, 2), -32768), rng.integers(-40, 41, (4, 128, 2)),
                  np.zeros((4, 128, 2))]).astype(np.int16)
    y0 = levels(rng, (n, 128, 2)); y1 = levels(rng, (n + 3, 128, 2))[3:]
    idx = np.array([4, 1, 1, 0, 2] * 14)[:n]                                    # repeats frames, skips frame 3
    cases = [(idx, False), (None, False), (idx, True)]
    nsat = 0
    for index, mis in cases:
        up = (lambda a: misaligned(torch, a, 1)) if mis else (lambda a: dev(torch, a))
        x0, x1 = sora.mimo_comp_ht40(up(w), up(y0), up(y1), i32(torch, index) if index is not None else None)
        x0, x1 = x0.cpu().numpy(), x1.cpu().numpy()
        for s in range(n):
            a, b = sm.mimo_comp(w[index[s] if index is not None else 0], y0[s], y1[s])
            assert np.array_equal(x0[s], a) and np.array_equal(x1[s], b), (s, mis)
            nsat += int(np.sum(np.abs(a.astype(int)) >= 32767))
    assert nsat > 0                                                            # saturated detected symbols are part of the comparison


# ------------------------------------------------------------------ pilot_track_ht40
def model_track(x0, x1, first, nsym, state):
    st = state.copy(); th = np.full(len(x0), SENTINEL, np.int16)
    for f, (a, k) in enumerate(zip(first, nsym)):
        for s in range(a, a + k):
            st[f, 16:] = sm._w16(st[f, 16:].astype(np.int64) + sm.pilot_inc(x0[s], x1[s])).astype(np.int16)
            th[s] = st[f, 16]
    return st, th


def test_pilot_track(env):
    torch, sora = env
    rng = np.random.default_rng(4)
    nsyms = [1, 2, 3, 12, 0, 5, 67]; gaps = [0, 1, 2, 3, 5, 0, 1]
    first = []; pos = 0
    for n, g in zip(nsyms, gaps):
        pos += g; first.append(pos); pos += n
    total = pos                                                                 # the last frame's last symbol ends the buffer
    x0 = levels(rng, (total, 128, 2)); x1 = rng.integers(-32768, 32768, (total, 128, 2)).astype(np.int16)
    x0[first[3]:first[3] + 12] = rng.integers(-32768, 32768, (12, 128, 2))
    state = rng.integers(-32768, 32768, (len(nsyms), 24)).astype(np.int16)      # theta words that differ from one another; the other sixteen words must stand
    want_st, want_th = model_track(x0, x1, first, nsyms, state)
    for nfr in (1, 3, 4, 5, 7):
        st = dev(torch, state[:nfr])
        th = torch.full((total,), SENTINEL, dtype=torch.int16, device="cuda")
        lib = sora.load()
        from sora_amd.capi import _check, _dev_ptr
        d = [dev(torch, x0), dev(torch, x1), i32(torch, first[:nfr]), i32(torch, nsyms[:nfr])]
        _check(lib.sora_hip_pilot_track_ht40(_dev_ptr(d[0]), _dev_ptr(d[1]), _dev_ptr(d[2]), _dev_ptr(d[3]), _dev_ptr(st), _dev_ptr(th), nfr, None))
        torch.cuda.synchronize()
        ws, wt = model_track(x0, x1, first[:nfr], nsyms[:nfr], state[:nfr])
        assert np.array_equal(st.cpu().numpy(), ws) and np.array_equal(th.cpu().numpy(), wt), nfr
        assert np.array_equal(ws[:, :16], state[:nfr, :16])
    # without the theta output: the same record
    st = dev(torch, state)
    assert sora.pilot_track_ht40(dev(torch, x0), dev(torch, x1), i32(torch, first), i32(torch, nsyms), st, want_theta=False) is None
    assert np.array_equal(st.cpu().numpy(), want_st)
    # the 3-symbol frame cut into two calls at every symbol boundary gives what one call gives
    a = first[2]
    for cut in (0, 1, 2, 3):
        st = dev(torch, state[2:3])
        t1 = sora.pilot_track_ht40(dev(torch, x0), dev(torch, x1), i32(torch, [a]), i32(torch, [cut]), st).cpu().numpy()
        t2 = sora.pilot_track_ht40(dev(torch, x0), dev(torch, x1), i32(torch, [a + cut]), i32(torch, [3 - cut]), st).cpu().numpy()
        assert np.array_equal(st.cpu().numpy(), want_st[2:3]), cut
        assert np.array_equal(np.concatenate([t1[a:a + cut], t2[a + cut:a + 3]]), want_th[a:a + 3]), cut


# ------------------------------------------------------------------ demap_ht40, deinterleave_ht40, stream_join_ht40
@pytest.fixture(scope="module")
def symbols():
    rng = np.random.default_rng(5)
    x = levels(rng, (67, 128, 2))
    x[7:40] = rng.integers(-140, 141, (33, 128, 2))                             # around the tables' range: every step of every table, and the limit at +-128
    return x


@pytest.mark.parametrize("nb", [1, 2, 4, 6])
def test_demap_deinterleave_join(env, symbols, nb):
    torch, sora = env
    rng = np.random.default_rng(6 + nb)
    want_all = np.stack([sm.demap(s, nb) for s in symbols])                     # computed once per modulation, shared by every count
    raw = rng.integers(0, 256, (67, 108 * nb)).astype(np.uint8)                 # the de-interleaver and the de-parser move bytes: any byte values
    raw1 = rng.integers(0, 256, (67, 108 * nb)).astype(np.uint8)
    perm = [dm.permutation(nb, 0).astype(np.int64), dm.permutation(nb, 1).astype(np.int64)]
    for n in COUNTS:
        for mis in (0, 1):
            up = (lambda a: misaligned(torch, a, 1)) if mis else (lambda a: dev(torch, a))
            got = sora.demap_ht40(up(symbols[:n]), nb).cpu().numpy()
            assert got.shape == (n, 108 * nb) and np.array_equal(got, want_all[:n]), (n, mis)
            for iss in range(2):
                got = sora.deinterleave_ht40(up(raw[:n]), nb, iss).cpu().numpy()
                assert np.array_equal(got, raw[:n][:, perm[iss]]), (n, mis, iss)
            got = sora.stream_join_ht40(up(raw[:n]), up(raw1[:n]), nb).cpu().numpy()
            assert np.array_equal(got, sm.stream_join(raw[:n], raw1[:n], nb)), (n, mis)
    # outputs that do not start on a 4- / 16-byte boundary
    out = torch.full((1 + 5 * 216 * nb,), 0xEE, dtype=torch.uint8, device="cuda")
    sora.stream_join_ht40(dev(torch, raw[:5]), dev(torch, raw1[:5]), nb, out=out[1:].reshape(5, 216 * nb))
    assert int(out[0]) == 0xEE and np.array_equal(out[1:].cpu().numpy().reshape(5, -1), sm.stream_join(raw[:5], raw1[:5], nb))
    from sora_amd.capi import _check, _dev_ptr
    for fn, src, want in (("demap", symbols[:5], want_all[:5]), ("deint", raw[:5], raw[:5][:, perm[1]])):
        out = torch.full((3 + 5 * 108 * nb + 1,), 0xEE, dtype=torch.uint8, device="cuda")
        if fn == "demap":
            _check(sora.load().sora_hip_demap_ht40(_dev_ptr(dev(torch, src)), out.data_ptr() + 3, nb, 5, None))
        else:
            _check(sora.load().sora_hip_deinterleave_ht40(_dev_ptr(dev(torch, src)), out.data_ptr() + 3, nb, 1, 5, None))
        o = out.cpu().numpy()
        assert (o[:3] == 0xEE).all() and o[-1] == 0xEE and np.array_equal(o[3:-1].reshape(5, -1), want), fn


# ------------------------------------------------------------------ downsample_ht40, noise_var_ht40
def test_downsample(env):
    torch, sora = env
    rng = np.random.default_rng(7)
    ns = [1, 2, 3, 4, 5, 8, 9, 67, 1030]; m0 = [0, 1, 0, 1, 1, 0, 7, 2, 5]; offs = [0, 1, 2, 3, 5, 63, 65, 4, 0]
    first = []; pos = 0
    for n, o in zip(ns, offs):
        pos = (pos + 63) // 64 * 64 + o; first.append(pos); pos += 2 * n - 1
    total = pos                                                                 # the last stream's last kept sample is the buffer's last sample
    x = [levels(rng, (total, 2)), rng.integers(-32768, 32768, (total, 2)).astype(np.int16)]
    x[0][first[-1]:first[-1] + 200] = -32768
    out_first = np.concatenate([[0], np.cumsum(np.array(ns) + 1)])[:-1] + 1     # one sentinel sample in front of and between the streams
    nout = int(out_first[-1] + ns[-1] + 1)
    for mis in (0, 1):
        d = [misaligned(torch, c, mis) if mis else dev(torch, c) for c in x]
        o = [torch.full((nout, 2), SENTINEL, dtype=torch.int16, device="cuda") for _ in range(2)]
        sora.downsample_ht40(d[0], d[1], i32(torch, first), i32(torch, ns), i32(torch, m0), i32(torch, out_first), o[0], o[1])
        for c in range(2):
            want = np.full((nout, 2), SENTINEL, np.int16)
            for a, n, p, of in zip(first, ns, m0, out_first):
                want[of:of + n] = sm.downsample(x[c][a:], n, p)
            assert np.array_equal(o[c].cpu().numpy(), want), (mis, c)
    # a stream cut into two calls at an odd and at an even m gives what one call gives
    a, n = first[-1], ns[-1]
    whole = sm.downsample(x[0][a:], n, 5)
    assert (whole[0:100:2] == 32767).all() and (whole[1:100:2] == -32768).all()         # m0 = 5: the even m are the odd samples, negated: -(-32768) = 32767
    for cut in (1, 2, 515, 516):
        d = [dev(torch, c) for c in x]
        o = [torch.full((n, 2), SENTINEL, dtype=torch.int16, device="cuda") for _ in range(2)]
        sora.downsample_ht40(d[0], d[1], i32(torch, [a]), i32(torch, [cut]), i32(torch, [5]), i32(torch, [0]), o[0], o[1])
        sora.downsample_ht40(d[0], d[1], i32(torch, [a + 2 * cut]), i32(torch, [n - cut]), i32(torch, [5 + cut]), i32(torch, [cut]), o[0], o[1])
        assert np.array_equal(o[0].cpu().numpy(), whole), cut
        assert np.array_equal(o[1].cpu().numpy(), sm.downsample(x[1][a:], n, 5)), cut


@pytest.mark.parametrize("n", COUNTS)
def test_noise_var(env, n):
    torch, sora = env
    rng = np.random.default_rng(8)
    l0 = levels(rng, (67, 128, 2))[:n]; l1 = levels(rng, (70, 128, 2))[3:3 + n]
    if n > 2:
        l0[2, :64] = 32767; l0[2, 64:] = -32768                                 # the largest S a frame can have
        l1[2, :64] = -32768; l1[2, 64:] = 32767
    S, nv = sora.noise_var_ht40(dev(torch, l0), dev(torch, l1))
    S, nv = S.cpu().numpy(), nv.cpu().numpy()
    want = [sm.noise_S(a, b) for a, b in zip(l0, l1)]
    assert S.tolist() == want
    assert nv.dtype == np.float32 and nv.tobytes() == np.array([sm.noise_var(s) for s in want], np.float32).tobytes()
    if n > 2:
        assert want[2] == 2 * 52 * 2 * 65535 ** 2


# ------------------------------------------------------------------ the composition against the handle
def handle_call(env, iq, descs, coding=0):
    torch, sora = env
    joint = coding == 1
    rx = sora.RxHt40(len(descs), joint_soft_capacity(descs) if joint else soft_capacity(sora, descs))
    rx.set_coding(coding)
    w = torch.zeros((len(descs), 4, 128, 2), dtype=torch.int16, device="cuda")
    t = rx.process_dev(dev(torch, iq[0]), dev(torch, iq[1]), descs, w)
    rows = rx.results(ticket=t)
    soft = [rx.soft(f, 0, ticket=t) if joint else [rx.soft(f, s, ticket=t) for s in range(2)] for f in range(len(descs))]
    rx.close()
    return rows, soft, w.cpu().numpy()


def assert_equals_handle(env, iq, descs, coding=0):
    torch, sora = env
    rows, soft, w = handle_call(env, iq, descs, coding)
    r = sora.rx_ht40_by_stages(dev(torch, iq[0]), dev(torch, iq[1]), descs, coding)
    gw = r["weights"].cpu().numpy()
    assert np.array_equal(gw[:, :, sm.OCC], w[:, :, sm.OCC])                    # MMSE and zero forcing: the handle's exported weights, bit for bit
    assert len(r["rows"]) == len(rows)
    for g, h in zip(r["rows"], rows):
        assert (g["error_code"], g["length"], g["crc32"], g["nsym"], g["mpdu"]) == (h["error_code"], h["length"], h["crc32"], h["nsym"], h["mpdu"]), (g["frame"], g["stream"])
        assert h["stream"] == g["stream"] and h["capture_id"] == (descs[g["frame"]][7] if len(descs[g["frame"]]) > 7 else g["frame"])
    for f in range(len(descs)):
        if coding == 1:
            assert np.array_equal(r["soft"][f], soft[f]), f
        else:
            for s in range(2):
                assert np.array_equal(r["soft"][f][s], soft[f][s]), (f, s)
    return r, rows, gw


def batch(rng, specs):
    """specs: [(nb, cr, lens, sigma, cfo_step, noise_var)] -> (iq, descs, psdus): frames one behind the other at offsets of every residue, the last one ending the buffer"""
    parts, descs, psdus, pos = [], [], [], 0
    for i, (nb, cr, lens, sigma, cfo_step, nv) in enumerate(specs):
        lead = (0, 1, 2, 3, 5, 63, 65)[i % 7]
        iq, ps, _, nsym = send(rng, nb, cr, lens, sigma, cfo_step=cfo_step, lead=lead)
        descs.append((pos + lead, nb, cr, lens[0], lens[1], int(round(-cfo_step)), nv, 100 + i))
        parts.append(iq); psdus.append(ps); pos += iq.shape[1]
    return np.concatenate(parts, axis=1), descs, psdus


@pytest.mark.parametrize("nv", [0.0, 3000.0])
def test_composition_equals_the_handle_per_stream(env, nv):
    rng = np.random.default_rng(11 + int(nv))
    specs = [(1, 0, (4, 4), 3.0, 0.0, nv), (2, 0, (30, 11), 3.0, 37.0, nv), (2, 2, (25, 40), 3.0, -511.0, nv), (4, 0, (77, 20), 3.0, 0.0, nv), (4, 2, (60, 61), 3.0, 0.0, nv),
             (6, 1, (39, 120), 3.0, -4096.0, nv), (6, 2, (90, 33), 6.0, 0.0, nv), (6, 2, (80, 81), 150.0, 0.0, nv), (1, 0, (75, 60), 2.0, 0.0, nv)]
    iq, descs, psdus = batch(rng, specs)
    descs.append(descs[4][:3] + (59,) + descs[4][4:7] + (200,))                 # frame 4 once more, stream 0 described one byte short (the same two symbols): its FCS fails
    r, rows, gw = assert_equals_handle(env, iq, descs)
    codes = [x["error_code"] for x in r["rows"]]
    print("64-QAM 3/4 at sigma 150: error codes", [hex(c) for c in codes[14:16]])
    assert 0x80000006 in codes[14:16] and codes[18:20] == [0x80000006, 1]       # frames that fail their FCS are compared all the same, PSDU bytes included
    assert all(c == 1 for c in codes[:2 * 7]) and [x["mpdu"] for x in r["rows"][:2]] == psdus[0]
    assert sorted({x["nsym"] for x in r["rows"]})[0] == 1 and max(x["nsym"] for x in r["rows"]) >= 12
    # the stages against the model, the weights included: zero forcing is so_ht40_zf_weights, MMSE within +-1 LSB of float64
    want = sm.by_stages(iq, descs)
    for f, d in enumerate(descs):
        assert np.array_equal(r["theta"][f], want["theta"][f]), f
        assert np.array_equal(r["xs"][f], want["xs"][f]), f
        assert np.array_equal(gw[f], np.asarray(want["weights"][f])) and np.array_equal(r["h"].cpu().numpy()[f], np.asarray(want["h"][f])), f
        if nv == 0.0:
            assert np.array_equal(gw[f][:, sm.OCC], dm.zf_weights(iq, d[0], d[5])[:, sm.OCC]), f
        else:
            f64 = sm.mmse_solve(np.asarray(want["h"][f])[:, sm.OCC], float(np.float32(nv)), np.float64)
            ok = np.abs(f64.astype(int)).max(axis=(0, 2)) <= 32000
            assert ok.any() and np.abs(gw[f][:, sm.OCC][:, ok].astype(int) - f64[:, ok].astype(int)).max() <= 1, f


def test_mistuned_descriptor_and_quiet_ltfs_in_front_of_full_scale_data(env):
    """theta across +-32768 (sent with step 37, described as 0), and a frame whose HT-LTFs are 200 times quieter and whose data is 40 times louder than sent: weights and detected symbols at the rails"""
    rng = np.random.default_rng(37)
    a, psa, _, na = send(rng, 1, 0, (75, 60), 2.0, cfo_step=37.0, lead=3)
    b, psb, _, nb_ = send(rng, 4, 0, (50, 41), 2.0, lead=0)
    b = b.copy(); b[:, :320] //= 200
    b[:, 320:] = np.clip(b[:, 320:].astype(np.int64) * 40, -32768, 32767).astype(np.int16)
    iq = np.concatenate([a, b], axis=1)
    descs = [(3, 1, 0, 75, 60, 0, 0.0), (a.shape[1], 4, 0, 50, 41, 0, 0.0)]
    for nv in (0.0, 2.0):
        ds = [d[:6] + (nv,) for d in descs]
        r, rows, gw = assert_equals_handle(env, iq, ds)
        th = r["theta"][0].astype(int)
        assert np.any(np.diff(th) < -30000) and th.max() > 26000 and th.min() < -26000, th
        assert r["rows"][0]["mpdu"] == psa[0] and r["rows"][1]["mpdu"] == psa[1]
        want = sm.by_stages(iq, ds)
        nsat_w = int(np.sum(np.abs(np.asarray(want["weights"][1])[:, sm.OCC].astype(int)) >= 32767))
        nsat_x = int(np.sum(np.abs(want["xs"][1][:, :, sm.OCC].astype(int)) >= 32767))
        assert nsat_w > 0 and nsat_x > 0, (nsat_w, nsat_x)
        for f in range(2):
            assert np.array_equal(r["theta"][f], want["theta"][f]) and np.array_equal(r["xs"][f], want["xs"][f]) and np.array_equal(gw[f], np.asarray(want["weights"][f])), (nv, f)
            for s in range(2):
                assert np.array_equal(r["soft"][f][s], want["soft"][f][s])


@pytest.mark.parametrize("nv", [0.0, 3000.0])
def test_composition_equals_the_handle_joint(env, nv):
    rng = np.random.default_rng(21 + int(nv))
    parts, descs, pos = [], [], 0
    for i, (mcs, length, sigma) in enumerate([(8, 5, 3.0), (9, 37, 3.0), (11, 200, 3.0), (13, 90, 3.0), (14, 301, 6.0), (14, 250, 150.0)]):
        nbp, cr = m.MCS2[mcs]
        psdu = m.add_fcs(rng.integers(0, 256, length - 4, dtype=np.uint8).tobytes())
        x, nsym = J.tx_joint(psdu, nbp, cr, seed=int(rng.integers(1, 128)))
        lead = (0, 1, 2, 3, 5, 63)[i]
        iq = m.channel(x, H0, sigma, rng, lead=lead)
        descs.append((pos + lead, nbp, cr, length, 0, 0, nv, 7 + i)); parts.append(iq); pos += iq.shape[1]
    iq = np.concatenate(parts, axis=1)
    descs.append(descs[2][:3] + (199,) + descs[2][4:7] + (200,))                # frame 2 once more, described one byte short (the same four symbols): its FCS fails
    r, rows, gw = assert_equals_handle(env, iq, descs, coding=1)
    codes = [x["error_code"] for x in r["rows"]]
    print("joint, 64-QAM 3/4 at sigma 150: error code", hex(codes[5]))
    assert codes[:5] == [1, 1, 1, 1, 1] and codes[6] == 0x80000006
    want = sm.by_stages(iq, descs, coding=1)
    for f in range(len(descs)):
        assert np.array_equal(r["soft"][f], want["soft"][f]) and np.array_equal(r["theta"][f], want["theta"][f]), f


# ------------------------------------------------------------------ the front end's composition against the handle's first record
def test_front_composition_equals_the_handles_first_record(env):
    """captures of tests/ht40_front_captures.py that hold one frame behind a lead (every MCS, a noise floor) and one header failure of each cause, in one buffer at
    offsets that are multiples of 4: a20, mcs, ht_len, nsym, cfo, end_sample and error_code exactly; noise_var within the bound tests/test_gpu_ht40_front.py states for the
    handle's single-precision sum, |noise_var - S / 416| <= 2^-19 S / 416, with S the stage's exact integer; the descriptor by k_ht40_plan's rule"""
    torch, sora = env
    import ht40_front_captures as fc
    import ht40_front_model as fm
    caps = [c for c in fc.build(False, full=False) if c.family in ("plain", "gate") and "cut" not in c.name]
    assert len([c for c in caps if c.family == "gate"]) >= 9
    iq, descs = fc.layout(caps)
    d0, d1 = dev(torch, iq[0]), dev(torch, iq[1])
    rx = sora.RxHt40(256, 1 << 21)
    t = rx.process_captures_dev(d0, d1, descs, max_frames_per_capture=fc.MAX_EVENTS)
    rx.wait(t)
    found = [rx.found(c, ticket=t) for c in range(len(descs))]
    rx.close()
    got = sora.rx_ht40_front_by_stages(d0, d1, [(o, n) for o, n, _ in descs])
    codes = set()
    for cap, d, g, f in zip(caps, descs, got, found):
        assert f and g is not None, cap.name
        h = f[0]
        assert {k: int(g[k]) for k in ("a20", "mcs", "ht_len", "nsym", "cfo", "end_sample", "error_code")} == \
               {k: int(h[k]) for k in ("a20", "mcs", "ht_len", "nsym", "cfo", "end_sample", "error_code")}, cap.name
        exact = g["S"] / 416.0
        assert abs(float(h["noise_var"]) - exact) <= 2.0 ** -19 * exact and g["noise_var"] == np.float32(exact), (cap.name, h["noise_var"], exact)
        if h["error_code"] == 0:
            assert g["descriptor"][:6] == fm.descriptor(d[0], h, 0.0)[:6], cap.name
        codes.add(h["error_code"])
    assert codes == {0, 0x80000005}
