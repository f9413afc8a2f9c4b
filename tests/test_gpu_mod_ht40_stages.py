"""GPU parity of the 40 MHz HT modulation graph's stage entry points (sora_amd/csrc/k_mod_ht40.hip) against the per-stage numpy models of tests/mod_ht40_model.py
(pinned to the three frame models by tests/test_mod_ht40_model_cpu.py), bit for bit, every output buffer pre-filled with a sentinel and compared whole; of their
composition against the fused transmitters; and of the transmit bricks against the receive stages that already exist, with no channel in between.

T = 32: the byte-wide stages, the mapper and the SIG mapper take tiles of 32 symbols (frames), the IFFT 32 symbols per workgroup; the pilot stage passes of 8."""
import numpy as np
import pytest

import mod_ht40_model as M

pytestmark = pytest.mark.gpu

T = 32
NSYMS = (1, 2, T - 1, T, T + 1, 257)                 # one symbol, two, the edges of a tile either side, several workgroups
NB = (1, 2, 4, 6)


@pytest.fixture(scope="module")
def env():
    import torch
    import sora_amd
    sora_amd.load()
    assert torch.cuda.is_available()
    return torch, sora_amd


def dev(torch, a, dt=None):
    return torch.from_numpy(np.ascontiguousarray(a, dt)).cuda()


def i32(torch, a):
    return dev(torch, np.asarray(a, np.int64).astype(np.int32))


def into(torch, rows, shape, dtype, fill):
    """a buffer of `rows` + 3 rows pre-filled with `fill`: (tensor, the numpy image of what it held)"""
    img = np.full((rows + 3,) + shape, fill, dtype)
    return dev(torch, img), img


@pytest.fixture(scope="module")
def cases():
    """per n_bpsc: coded symbols, the parser's outputs, rows of any bytes, the interleaved rows, the mapped carriers -- computed once"""
    rng = np.random.default_rng(40)
    n = max(NSYMS)
    out = {}
    for nb in NB:
        coded = rng.integers(0, 256, (n, 27 * nb)).astype(np.uint8)
        rows = rng.integers(0, 256, (n, M.row_bytes(nb))).astype(np.uint8)      # (for BPSK with the unused half byte set: the stages do not read it)
        inter = {iss: M.interleave(rows, nb, iss) for iss in (0, 1)}
        out[nb] = dict(coded=coded, parsed=M.stream_parse(coded, nb), rows=rows, inter=inter, car=M.map40(rows, nb))
    return out


@pytest.fixture(scope="module")
def symbols():
    """bins and time samples of max(NSYMS) symbols, the first two at the rails -- computed once"""
    rng = np.random.default_rng(41)
    n = max(NSYMS)
    car = rng.integers(-32768, 32768, (n, 108, 2)).astype(np.int16)
    bins = rng.integers(-12000, 12001, (n, 128, 2)).astype(np.int16)
    bins[0] = 32767; bins[1] = -32768
    bins[2, :, 0] = 32767; bins[2, :, 1] = -32768
    t = rng.integers(-32768, 32768, (n, 128, 2)).astype(np.int16)
    t[0] = 32767; t[1] = -32768
    return dict(car=car, piloted=M.add_pilot(car), bins=bins, time=M.ifft(bins), t=t)


@pytest.mark.parametrize("nb", NB)
def test_stream_parse(env, cases, nb):
    torch, sora = env
    c = cases[nb]
    for n in NSYMS:
        o0, img0 = into(torch, n, (M.row_bytes(nb),), np.uint8, 0xA5)
        o1, img1 = into(torch, n, (M.row_bytes(nb),), np.uint8, 0x5A)
        sora.stream_parse_ht40(dev(torch, c["coded"][:n]), nb, out=(o0, o1))
        img0[:n] = c["parsed"][0][:n]; img1[:n] = c["parsed"][1][:n]             # bytes behind the last symbol stay as they were
        assert np.array_equal(o0.cpu().numpy(), img0) and np.array_equal(o1.cpu().numpy(), img1), n
    if nb == 1:
        assert not (c["parsed"][0][:, 13] & 0xF0).any() and not (c["parsed"][1][:, 13] & 0xF0).any()


@pytest.mark.parametrize("iss", [0, 1])
@pytest.mark.parametrize("nb", NB)
def test_interleave(env, cases, nb, iss):
    torch, sora = env
    c = cases[nb]
    for n in NSYMS:
        o, img = into(torch, n, (M.row_bytes(nb),), np.uint8, 0xC3)
        sora.interleave_ht40(dev(torch, c["rows"][:n]), nb, iss, out=o)
        img[:n] = c["inter"][iss][:n]
        assert np.array_equal(o.cpu().numpy(), img), n


@pytest.mark.parametrize("iss", [0, 1])
@pytest.mark.parametrize("nb", NB)
def test_interleave_stream_on_a_table_of_frames(env, nb, iss):
    """frames of 1, 2, 0, 3 and 33 symbols whose coded streams begin at odd byte offsets; at BPSK a symbol is 13.5 bytes, so odd symbols start mid-byte; rows 3, 4 and 8
    belong to no frame and keep their sentinel, and so does everything behind the last frame"""
    torch, sora = env
    rng = np.random.default_rng([nb, iss, 42])
    nsym, first = [1, 2, 0, 3, 33], [0, 1, 3, 5, 9]
    ncb = 108 * nb
    streams = [rng.integers(0, 256, (k * ncb + 7) // 8 + 2).astype(np.uint8) for k in nsym]
    off, blob = [], np.zeros(0, np.uint8)
    for f, s in enumerate(streams):
        blob = np.concatenate([blob, rng.integers(0, 256, 1 + 2 * f).astype(np.uint8)])   # offsets 1, 4+.., never all aligned
        off.append(len(blob)); blob = np.concatenate([blob, s])
    assert any(o % 16 for o in off) and any(o % 2 for o in off)
    o, img = into(torch, 42, (M.row_bytes(nb),), np.uint8, 0x3C)
    sora.interleave_ht40_stream(dev(torch, blob), i32(torch, off), i32(torch, first), i32(torch, nsym), nb, iss, o)
    for f, s in enumerate(streams):
        img[first[f]:first[f] + nsym[f]] = M.interleave_stream(s, nsym[f], nb, iss)
    got = o.cpu().numpy()
    assert np.array_equal(got, img), np.flatnonzero((got != img).any(axis=1))
    assert (got[[3, 4, 8]] == 0x3C).all() and (got[42:] == 0x3C).all()


@pytest.mark.parametrize("nb", [1, 6])
def test_interleave_stream_at_the_tile_edges(env, cases, nb):
    """one frame of T - 1, T, T + 1 and 257 symbols: the stream form on back-to-back bits is the row form on the same bits"""
    torch, sora = env
    ncb = 108 * nb
    bits = np.unpackbits(cases[nb]["rows"], axis=-1, bitorder="little")[:, :ncb]
    for n in NSYMS[2:]:
        stream = np.packbits(bits[:n].reshape(-1), bitorder="little")
        o, img = into(torch, n, (M.row_bytes(nb),), np.uint8, 0x3C)
        sora.interleave_ht40_stream(dev(torch, stream), i32(torch, [0]), i32(torch, [0]), i32(torch, [n]), nb, 1, o)
        img[:n] = cases[nb]["inter"][1][:n]                                      # (BPSK: the rows' unused half byte is not part of the stream, and neither form reads it)
        assert np.array_equal(img[:n], M.interleave_stream(stream, n, nb, 1))
        assert np.array_equal(o.cpu().numpy(), img), n


@pytest.mark.parametrize("nb", NB)
def test_map(env, cases, nb):
    torch, sora = env
    c = cases[nb]
    for n in NSYMS:
        o, img = into(torch, n, (108, 2), np.int16, 0x1234)
        sora.map_ht40(dev(torch, c["rows"][:n]), nb, out=o)
        img[:n] = c["car"][:n]
        assert np.array_equal(o.cpu().numpy(), img), n
    d = {1: 6144, 2: 6144, 4: 4000, 6: 2214}[nb]
    assert set(np.unique(np.abs(c["car"][..., 0]))) == {d * k for k in range(1, 2 ** max(nb // 2, 1), 2)}
    assert nb > 1 or not c["car"][..., 1].any()                                  # BPSK is on I alone


def test_sig_map(env):
    torch, sora = env
    x = np.random.default_rng(43).integers(0, 256, (T + 1, 18)).astype(np.uint8)
    x[0] = 0; x[1] = 0xFF
    want = M.sig_map(x)
    for n in (1, T - 1, T, T + 1):
        o, img = into(torch, n, (3, 128, 2), np.int16, 0x2BCD)
        sora.sig_map_ht40(dev(torch, x[:n]), out=o)
        img[:n] = want[:n]
        assert np.array_equal(o.cpu().numpy(), img), n
    assert (np.count_nonzero(want.reshape(-1, 128, 2).any(axis=-1), axis=-1) == 104).all()   # 2 x (48 carriers + 4 pilots)


def test_add_pilot(env, symbols):
    torch, sora = env
    for n in NSYMS:
        o, img = into(torch, n, (128, 2), np.int16, 0x0BAD)
        sora.add_pilot_ht40(dev(torch, symbols["car"][:n]), i32(torch, [0]), i32(torch, [n]), out=o)
        img[:n] = symbols["piloted"][:n]
        assert np.array_equal(o.cpu().numpy(), img), n
    # a table of frames: symbols 3, 4 and 20 belong to no frame, one frame has no symbol
    first, nsym = [0, 5, 5, 21], [3, 0, 15, 17]
    o, img = into(torch, 38, (128, 2), np.int16, 0x0BAD)
    sora.add_pilot_ht40(dev(torch, symbols["car"][:38]), i32(torch, first), i32(torch, nsym), out=o)
    for f, k in zip(first, nsym):
        img[f:f + k] = symbols["piloted"][f:f + k]
    assert np.array_equal(o.cpu().numpy(), img)
    assert (np.count_nonzero(symbols["piloted"][5:].any(axis=-1), axis=-1) <= 114).all()


def test_ifft(env, symbols):
    """random bins, and every bin at +32767, at -32768 and at (+32767, -32768): symbols 0, 1 and 2"""
    torch, sora = env
    for n in NSYMS:
        o, img = into(torch, n, (128, 2), np.int16, 0x0FED)
        sora.ifft_ht40(dev(torch, symbols["bins"][:n]), out=o)
        img[:n] = symbols["time"][:n]
        assert np.array_equal(o.cpu().numpy(), img), n


@pytest.mark.parametrize("gi", [0, 1])
def test_add_gi(env, symbols, gi):
    """random samples, and every sample at +32767 (symbol 0) and at -32768 (symbol 1)"""
    torch, sora = env
    want = M.add_gi(symbols["t"], gi)
    assert want.shape[1] == (144 if gi else 160)
    for n in NSYMS:
        o, img = into(torch, n, (want.shape[1], 2), np.int16, 0x0ACE)
        sora.add_gi_ht40(dev(torch, symbols["t"][:n]), gi, out=o)
        img[:n] = want[:n]
        assert np.array_equal(o.cpu().numpy(), img), n


@pytest.fixture(scope="module")
def one_frame(env):
    torch, sora = env
    a, b = bytes(range(40)), bytes(range(40, 80))
    o0, o1, _ = sora.tx_ht40([a], [b], [11])
    return o0.cpu().numpy(), o1.cpu().numpy()


@pytest.mark.parametrize("field", [0, 1])
def test_preamble(env, one_frame, field):
    torch, sora = env
    sl = slice(0, 640) if field == 0 else slice(1120, 1600)
    model = M.preamble(field)
    for ch in (0, 1):
        assert np.array_equal(one_frame[ch][sl], model[ch]), ch                  # the model's fixed fields are the fused frame's
    for n in (1, 3):
        p = sora.preamble_ht40(field, n)
        for ch in (0, 1):
            got = p[ch].cpu().numpy()
            assert got.shape == (n, sl.stop - sl.start, 2)
            assert all(np.array_equal(got[k], one_frame[ch][sl]) for k in range(n)), (n, ch)


def _frames():
    out = []
    for mcs in range(8, 15):
        for ln in (1, 37, 333):
            rng = np.random.default_rng([mcs, ln])
            out.append((mcs, bytes(rng.integers(0, 256, ln).astype(np.uint8)), bytes(rng.integers(0, 256, ln).astype(np.uint8))))
    rng = np.random.default_rng(3996)
    out.append((13, bytes(rng.integers(0, 256, 3996).astype(np.uint8)), bytes(rng.integers(0, 256, 3996).astype(np.uint8))))
    return out


def _same(sora, got, want):
    assert got[2] == want[2]                                                     # the offsets
    for ch in (0, 1):
        g, w = got[ch].cpu().numpy(), want[ch].cpu().numpy()
        assert g.shape == w.shape and np.array_equal(g, w), (ch, np.flatnonzero((g != w).any(axis=1))[:8] if g.shape == w.shape else (g.shape, w.shape))


@pytest.mark.parametrize("gi", ["none", "long", "short", "mixed"])
@pytest.mark.parametrize("joint", [False, True])
def test_by_stages_is_the_fused_transmitter(env, joint, gi):
    """MCS 8..14 x 1, 37 and 333 bytes and one frame of 3996 bytes at MCS 13, in one batch: both chains, sample for sample"""
    torch, sora = env
    fr = _frames()
    mcs, a, b = [f[0] for f in fr], [f[1] for f in fr], [f[2] for f in fr]
    g = {"none": None, "long": [0] * len(fr), "short": [1] * len(fr), "mixed": [(k * 5 // 3) & 1 for k in range(len(fr))]}[gi]
    if joint:
        _same(sora, sora.mod_ht40_by_stages(a, None, mcs, gi=g), sora.tx_ht40_joint(a, mcs, gi=g))
    else:
        _same(sora, sora.mod_ht40_by_stages(a, b, mcs, gi=g), sora.tx_ht40(a, b, mcs, gi=g))


@pytest.mark.parametrize("joint", [False, True])
def test_by_stages_takes_the_transmitters_seeds(env, joint):
    torch, sora = env
    seeds = [0x00, 0x01, 0x5B, 0xFF]
    mcs = [9, 12, 8, 14]
    a = [bytes(np.random.default_rng([s, 1]).integers(0, 256, 61 + s % 7).astype(np.uint8)) for s in seeds]
    b = [bytes(np.random.default_rng([s, 2]).integers(0, 256, 61 + s % 7).astype(np.uint8)) for s in seeds]
    if joint:
        _same(sora, sora.mod_ht40_by_stages(a, None, mcs, seeds=seeds), sora.tx_ht40_joint(a, mcs, seeds=seeds))
        _same(sora, sora.mod_ht40_by_stages(a, None, mcs, seeds=None, gi=[1, 0, 1, 0]), sora.tx_ht40_joint(a, mcs, seeds=None, gi=[1, 0, 1, 0]))
    else:
        pairs = [(s, s ^ 0x36) for s in seeds]
        _same(sora, sora.mod_ht40_by_stages(a, b, mcs, seeds=pairs), sora.tx_ht40(a, b, mcs, seeds=pairs))
        _same(sora, sora.mod_ht40_by_stages(a, b, mcs, seeds=None, gi=[1, 0, 1, 0]), sora.tx_ht40(a, b, mcs, seeds=None, gi=[1, 0, 1, 0]))


@pytest.mark.parametrize("iss", [0, 1])
def test_transmit_bricks_loop_through_the_receive_stages(env, cases, iss):
    """interleave_ht40 -> map_ht40 -> add_pilot_ht40 -> (the unit change below) -> demap_ht40 -> deinterleave_ht40 at 64-QAM gives back the hard bits of the
    interleaver's input: two stage families that exist apart, checked against each other with no channel in between.  The transmitter's unit is A = 16384 per HT-LTF
    carrier, the demapper's is 128: the carriers are divided by 128 with rounding, which is no channel (2214 k / 128 = 17.3 k, the demapper's level)."""
    torch, sora = env
    nb, n = 6, T + 1
    rows = dev(torch, cases[nb]["rows"][:n])
    bins = sora.add_pilot_ht40(sora.map_ht40(sora.interleave_ht40(rows, nb, iss), nb), i32(torch, [0]), i32(torch, [n]))
    x = ((bins.to(torch.int32) + 64) >> 7).to(torch.int16)
    soft = sora.deinterleave_ht40(sora.demap_ht40(x, nb), nb, iss).cpu().numpy()
    assert soft.shape == (n, 108 * nb) and soft.max() <= 7
    want = np.unpackbits(cases[nb]["rows"][:n], axis=-1, bitorder="little")[:, :108 * nb]
    assert np.array_equal((soft >= 4).astype(np.uint8), want)
