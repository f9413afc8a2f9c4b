"""GPU parity of the 802.11n modulation graphs' stage entry points (sora_amd/csrc/k_mod11n.hip) against the per-brick numpy models of tests/mod11n_model.py
(pinned to the recorded and the compiled reference modulator by tests/test_mod11n_model.py), bit for bit; and of their composition against the fused transmitter."""
import os

import numpy as np
import pytest

import mod11n_model as M

pytestmark = pytest.mark.gpu

NSYMS = (1, 2, 13, 31, 32, 33, 257)                  # one symbol, two, a part of a tile, the edges of a tile of 32 symbols either side, several workgroups
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
    """per n_bpsc: coded symbols, the parser's outputs (for BPSK also with the unused half byte set to ones), the interleaved symbols -- computed once"""
    rng = np.random.default_rng(7)
    n = max(NSYMS)
    out = {}
    for nb in NB:
        coded = rng.integers(0, 256, (n, 13 * nb)).astype(np.uint8)
        parsed = M.stream_parse(coded, nb)
        rows = [rng.integers(0, 256, (n, M.row_bytes(nb))).astype(np.uint8), parsed[1].copy()]   # the interleaver's and the mapper's input: any bytes, and a real stream
        if nb == 1:
            rows[1][:, 6] |= 0xF0                                                # the parser leaves it 0; the bricks behind it take what they get
        inter = {(k, iss): M.interleave(r, nb, iss) for k, r in enumerate(rows) for iss in (0, 1)}
        out[nb] = dict(coded=coded, parsed=parsed, rows=rows, inter=inter)
    return out


@pytest.mark.parametrize("nb", NB)
def test_stream_parse(env, cases, nb):
    torch, sora = env
    c = cases[nb]
    for n in NSYMS:
        o0, img0 = into(torch, n, (M.row_bytes(nb),), np.uint8, 0xA5)
        o1, img1 = into(torch, n, (M.row_bytes(nb),), np.uint8, 0x5A)
        sora.stream_parse11n(dev(torch, c["coded"][:n]), nb, out=(o0, o1))
        img0[:n] = c["parsed"][0][:n]; img1[:n] = c["parsed"][1][:n]             # bytes behind the last symbol stay as they were
        assert np.array_equal(o0.cpu().numpy(), img0) and np.array_equal(o1.cpu().numpy(), img1), n
    a, b = sora.stream_parse11n(dev(torch, c["coded"]), nb)
    assert np.array_equal(a.cpu().numpy(), c["parsed"][0]) and np.array_equal(b.cpu().numpy(), c["parsed"][1])


@pytest.mark.parametrize("iss", [0, 1])
@pytest.mark.parametrize("nb", NB)
def test_interleave(env, cases, nb, iss):
    torch, sora = env
    c = cases[nb]
    for k, x in enumerate(c["rows"]):
        want = c["inter"][(k, iss)]
        for n in NSYMS:
            o, img = into(torch, n, (M.row_bytes(nb),), np.uint8, 0xC3)
            sora.interleave11n(dev(torch, x[:n]), nb, iss, out=o)
            img[:n] = want[:n]
            assert np.array_equal(o.cpu().numpy(), img), (k, n)
    if nb == 1:                                                                  # the bits behind the symbol's 52 land on positions that are taken (the table is built over whole bytes)
        assert not np.array_equal(c["inter"][(1, iss)], M.interleave(c["parsed"][1], 1, iss))


@pytest.mark.parametrize("nb", NB)
def test_map(env, cases, nb):
    torch, sora = env
    c = cases[nb]
    for k in (0, 1):
        x = c["inter"][(k, 0)] if k == 0 else c["rows"][1]                       # (for BPSK rows[1] has the unused half byte set: the 52 carriers do not see it)
        for mod in (0, 10720):
            want = M.map11n(x, nb, mod)
            for n in NSYMS:
                o, img = into(torch, n, (52, 2), np.int16, 0x1234)
                sora.map11n(dev(torch, x[:n]), nb, mod, out=o)
                img[:n] = want[:n]
                assert np.array_equal(o.cpu().numpy(), img), (k, mod, n)
    if nb == 1:
        clean = c["rows"][1].copy(); clean[:, 6] &= 0x0F
        assert np.array_equal(M.map11n(clean, 1), M.map11n(c["rows"][1], 1))


def test_sig_map(env):
    torch, sora = env
    x = np.random.default_rng(11).integers(0, 256, (65, 18)).astype(np.uint8)
    x[0] = 0; x[1] = 0xFF
    want = M.sig_map(x)
    for n in (1, 2, 31, 32, 33, 65):                                             # the edges of a tile of 32 frames either side
        assert np.array_equal(sora.sig_map11n(dev(torch, x[:n])).cpu().numpy(), want[:n]), n


@pytest.mark.parametrize("iss", [0, 1])
def test_add_pilot(env, iss):
    torch, sora = env
    rng = np.random.default_rng(30 + iss)
    nsym = [1, 2, 3, 4, 5, 126, 127, 128, 129, 509] + [1, 17, 16, 15, 33, 5, 2]  # the sign wrap at 127, the pattern's period 4, their joint period 508; a ragged batch
    first = np.cumsum([0] + [n + (i % 3) for i, n in enumerate(nsym[:-1])]) + 2  # symbols no frame owns lie between
    total = int(first[-1] + nsym[-1] + 3)
    car = rng.integers(-32768, 32768, (total, 52, 2)).astype(np.int16)
    o, want = into(torch, total - 3, (64, 2), np.int16, 0x0BAD)
    for f, n in zip(first, nsym):
        want[f:f + n] = M.add_pilot(car[f:f + n], iss)
    sora.add_pilot11n(dev(torch, car), i32(torch, first), i32(torch, nsym), iss, out=o)
    got = o.cpu().numpy()
    bad = np.flatnonzero((got != want).any(axis=(1, 2)))
    assert len(bad) == 0, bad[:10]                                               # (symbols outside every frame: untouched)
    p = want[first[9]:first[9] + 509][:, [43, 57, 7, 21], 0]                     # the long frame's pilots: four patterns (a sign flip is a rotation by two), repeating after 508 symbols
    assert len({tuple(r) for r in p}) == 4 and np.array_equal(p[0], p[508]) and not np.array_equal(p[:127], p[127:254])
    # one table entry that continues its frame from position 125, beside one from 0; the wrapper's own zeroed buffer
    pos0 = [125, 0]
    got = sora.add_pilot11n(dev(torch, car[:40]), i32(torch, [0, 20]), i32(torch, [20, 20]), iss, pos0=i32(torch, pos0)).cpu().numpy()
    assert np.array_equal(got[:20], M.add_pilot(car[:20], iss, 125)) and np.array_equal(got[20:], M.add_pilot(car[20:40], iss, 0))
    assert np.array_equal(M.add_pilot(car[:145], iss)[125:], M.add_pilot(car[125:145], iss, 125))


NSYM_T = (1, 7, 8, 9, 31, 32, 33, 257)               # a group of 8 symbols' edges, the IFFT workgroup's 32 either side, several workgroups


@pytest.fixture(scope="module")
def time_cases():
    """bins for TIFFTxOnly: random at three scales, every bin at a rail, single tones; and the transforms (computed once, shared by the CSD and GI tests as inputs)"""
    rng = np.random.default_rng(40)
    n = max(NSYM_T)
    x = np.zeros((n, 64, 2), np.int16)
    x[:64] = rng.integers(-300, 301, (64, 64, 2)); x[64:128] = rng.integers(-31000, 31001, (64, 64, 2)); x[128:n - 67] = rng.integers(-32768, 32768, (n - 195, 64, 2))
    x[n - 67] = 32767; x[n - 66] = -32767
    x[n - 65] = np.where(rng.integers(0, 2, (64, 2)) == 1, 32767, -32767)        # every bin at full scale: a saturation or wrap difference shows
    for b in range(64):                                                          # a single tone per bin
        x[n - 64 + b, b] = (32767, -32767) if b & 1 else (-32767, 32767)
    return x, M.ifft_only(x)


def test_ifft_only(env, time_cases):
    torch, sora = env
    x, want = time_cases
    got = sora.ifft_only11n(dev(torch, x)).cpu().numpy()
    bad = np.flatnonzero((got != want).any(axis=(1, 2)))
    assert len(bad) == 0, bad[:10]
    for n in NSYM_T:
        got = sora.ifft_only11n(dev(torch, x[len(x) - n:])).cpu().numpy()        # (the tail holds the full-scale and single-tone symbols)
        assert np.array_equal(got, want[len(x) - n:]), n
        got = sora.ifft_only11n(dev(torch, x[64:64 + n])).cpu().numpy()
        assert np.array_equal(got, want[64:64 + n]), n


@pytest.mark.parametrize("ncsd", [1, 2, 4, 31])
def test_csd(env, time_cases, ncsd):
    torch, sora = env
    rng = np.random.default_rng(50 + ncsd)
    for n in NSYM_T:
        x = rng.integers(-32768, 32768, (n, 128, 2)).astype(np.int16)
        x[0] = np.where(rng.integers(0, 2, (128, 2)) == 1, 32767, -32767)
        got = sora.csd11n(dev(torch, x), ncsd).cpu().numpy()
        assert np.array_equal(got, M.csd(x, ncsd)), n
        assert np.array_equal(got, np.roll(x, 4 * ncsd, axis=1))
    t = time_cases[1]
    assert np.array_equal(sora.csd11n(dev(torch, t), ncsd).cpu().numpy(), M.csd(t, ncsd))
    d = dev(torch, t[:1])
    assert sora.load().sora_hip_csd11n(d.data_ptr(), d.data_ptr(), ncsd, 1, None) == -1      # in place: refused
    assert np.array_equal(d.cpu().numpy(), t[:1])


def test_add_gi(env, time_cases):
    torch, sora = env
    rng = np.random.default_rng(60)
    for n in NSYM_T:
        x = rng.integers(-32768, 32768, (n, 128, 2)).astype(np.int16)
        x[n // 2] = np.where(rng.integers(0, 2, (128, 2)) == 1, 32767, -32767)
        assert np.array_equal(sora.add_gi11n(dev(torch, x)).cpu().numpy(), M.add_gi(x)), n
    t = time_cases[1]
    assert np.array_equal(sora.add_gi11n(dev(torch, t)).cpu().numpy(), M.add_gi(t))


@pytest.mark.parametrize("field", [0, 1])
def test_preamble(env, field):
    torch, sora = env
    z = np.load(os.path.join(M.GOLD, "refgraph_11n.npz"))
    sl = slice(0, 640) if field == 0 else slice(1120, 1600)
    for k in range(4):                                                           # the recorded frames agree on their fixed fields
        assert np.array_equal(z["tx%d_0" % k][sl], M.preamble(field)[0]) and np.array_equal(z["tx%d_1" % k][sl], M.preamble(field)[1])
    for n in (1, 3):
        g0, g1 = sora.preamble11n(field, n)
        g0, g1 = g0.cpu().numpy(), g1.cpu().numpy()
        assert g0.shape == g1.shape == (n, sl.stop - sl.start, 2)
        assert (g0 == M.preamble(field)[0][None]).all() and (g1 == M.preamble(field)[1][None]).all(), n
    with pytest.raises(sora.SoraError):
        sora.preamble11n(2, 1)


def batch():
    """MCS 8..14 x lengths 1, 37, 150, 151, 700 (150 B at MCS 10 and 1 B at MCS 14: the reference's extra symbol) and 7 B at MCS 8; non-default seeds among them"""
    out = []
    for mcs in range(8, 15):
        for j, ln in enumerate((1, 37, 150, 151, 700)):
            seed = (0xAB, 0x00, 0x01, 0x5B, 0xFF)[(mcs + j) % 5]
            out.append((bytes(np.random.default_rng([mcs, ln]).integers(0, 256, ln).astype(np.uint8)), mcs, seed))
    out.append((bytes(range(7)), 8, 0x5B))
    return out


def test_chain_of_stages_equals_the_fused_transmitter(env):
    torch, sora = env
    fr = batch()
    mp, mcs, seeds = [f[0] for f in fr], [f[1] for f in fr], [f[2] for f in fr]
    assert {0x00, 0x01, 0x5B, 0xFF} <= set(seeds)
    for ln, m in ((150, 10), (7, 8), (1, 14)):                                   # the reference's extra-symbol cases are in the batch
        assert any(len(p) == ln and k == m for p, k in zip(mp, mcs)) and sora.tx11n_samples(ln, m) > 1600 + 160 * -(-((ln + 4) * 8 + 22) // M.MCS[m][2])
    b0, b1, boff = sora.tx11n(mp, mcs, seeds)
    b0, b1 = b0.cpu().numpy(), b1.cpu().numpy()
    plan = sora.Mod11nStages(mp, mcs, seeds)
    assert plan.offsets == boff
    for rep in range(2):                                                         # a second run of the same plan gives the same
        a0, a1 = plan.run()
        torch.cuda.synchronize()
        a0, a1 = a0.cpu().numpy(), a1.cpu().numpy()
        assert a0.shape == b0.shape and a1.shape == b1.shape
        for f in range(len(fr)):
            s = slice(boff[f], boff[f + 1])
            assert np.array_equal(a0[s], b0[s]) and np.array_equal(a1[s], b1[s]), (rep, fr[f][1], len(fr[f][0]), fr[f][2])
    c0, c1, coff = sora.mod11n_by_stages(mp, mcs, seeds)
    assert coff == boff and np.array_equal(c0.cpu().numpy(), b0) and np.array_equal(c1.cpu().numpy(), b1)
    for f in (0, 12, 35):                                                        # ... and the model's composition: MCS 8 / 1 B, MCS 10 / 150 B, the 7-byte MCS 8 frame
        w0, w1 = M.compose(mp[f], mcs[f], seeds[f])
        assert np.array_equal(b0[boff[f]:boff[f + 1]], w0) and np.array_equal(b1[boff[f]:boff[f + 1]], w1), f


def test_chain_of_one_frame_and_default_seeds(env):
    """batches in which some modulation's run of symbols is empty; seeds None = 0xAB"""
    torch, sora = env
    for mcs in ([14], [8, 9], [11, 13, 10]):
        mp = [bytes(np.random.default_rng(m).integers(0, 256, 60 + m).astype(np.uint8)) for m in mcs]
        a0, a1, aoff = sora.mod11n_by_stages(mp, mcs)
        b0, b1, boff = sora.tx11n(mp, mcs)
        assert aoff == boff and np.array_equal(a0.cpu().numpy(), b0.cpu().numpy()) and np.array_equal(a1.cpu().numpy(), b1.cpu().numpy()), mcs
