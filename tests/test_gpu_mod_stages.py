"""GPU parity of the 802.11a modulation graph's stage entry points (sora_amd/csrc/k_mod.hip) against the per-brick numpy models of tests/mod11a_model.py
(pinned to the oracle and the reference modulator by tests/test_mod11a_model.py), bit for bit; and of their composition against the fused transmitter."""
import numpy as np
import pytest

import mod11a_model as M
from oracle.pyoracle import RATES
from tx11a44_model import has_rail, up40to44

pytestmark = pytest.mark.gpu

NSYMS = (1, 2, 31, 32, 33, 63, 64, 65, 257)                                      # one symbol, a part of a tile, the edges of one tile of 32 and of two either side, several workgroups


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


def test_scramble(env):
    torch, sora = env
    rng = np.random.default_rng(1)
    lens = [1, 2, 15, 16, 17, 127, 128, 300, 2000] * 4 + [255, 256, 257, 1016]   # 40 frames
    tails = []
    for f, ln in enumerate(lens):                                               # absent (no frame's byte), 0, last, >= len
        tails.append([0xFFFFFFFF - 7, 0, ln - 1, ln, ln + 5][f % 5])
    seeds = [0x00, 0x01, 0xFF, 0x5B, 0x80, 0x7E] * 7
    gaps = rng.integers(0, 7, len(lens))                                         # ragged offsets: nothing is aligned
    off = np.cumsum([g + ln for g, ln in zip(gaps, [0] + lens[:-1])]) + 3
    total = int(off[-1] + lens[-1] + 9)
    x = rng.integers(0, 256, total).astype(np.uint8)
    want = x.copy()
    for f, ln in enumerate(lens):
        want[off[f]:off[f] + ln] = M.scramble(x[off[f]:off[f] + ln], seeds[f], tails[f] if tails[f] < ln else None)
    d_tail = dev(torch, np.asarray(tails, np.uint32).view(np.int32))
    d_seed = dev(torch, np.asarray(seeds[:len(lens)], np.uint8))
    got = sora.scramble11a(dev(torch, x), i32(torch, off), i32(torch, lens), d_seed, tail=d_tail, max_len=2000).cpu().numpy()
    assert np.array_equal(got, want)                                             # (the bytes between the frames are the wrapper's copy: untouched)
    # no tail array at all: every byte DO_SCRAMBLE
    want2 = x.copy()
    for f, ln in enumerate(lens):
        want2[off[f]:off[f] + ln] = M.scramble(x[off[f]:off[f] + ln], seeds[f])
    got2 = sora.scramble11a(dev(torch, x), i32(torch, off), i32(torch, lens), d_seed).cpu().numpy()
    assert np.array_equal(got2, want2) and not np.array_equal(want, want2)


@pytest.mark.parametrize("cr", [M.CR_12, M.CR_23, M.CR_34])
def test_conv_encode(env, cr):
    torch, sora = env
    rng = np.random.default_rng(10 + cr)
    lens = [1, 2, 3, 4, 5, 6, 7, 63, 64, 65, 300, 2001]
    bin_ = cr + 1
    in_off = np.cumsum([0] + [ln + 5 for ln in lens[:-1]]) + 1
    x = rng.integers(0, 256, int(in_off[-1] + lens[-1] + 4)).astype(np.uint8)
    outs = [M.conv_encode(x[o:o + ln], cr) for o, ln in zip(in_off, lens)]
    assert [len(o) for o in outs] == [ln // bin_ * (bin_ + 1) for ln in lens]
    out_off = np.cumsum([0] + [len(o) + 3 for o in outs[:-1]]) + 2
    fill = rng.integers(0, 256, int(out_off[-1] + len(outs[-1]) + 8)).astype(np.uint8)
    want = fill.copy()
    for o, y in zip(out_off, outs):
        want[o:o + len(y)] = y                                                   # the bytes behind a frame's output stay as they were
    d_out = dev(torch, fill)
    sora.conv_encode11a(dev(torch, x), i32(torch, in_off), i32(torch, lens), cr, d_out, i32(torch, out_off), max_len=2001)
    torch.cuda.synchronize()
    assert np.array_equal(d_out.cpu().numpy(), want)


@pytest.fixture(scope="module")
def coded_symbols():
    rng = np.random.default_rng(20)
    return {nb: rng.integers(0, 256, (max(NSYMS), 6 * nb)).astype(np.uint8) for nb in (1, 2, 4, 6)}


@pytest.mark.parametrize("nb", [1, 2, 4, 6])
def test_interleave(env, coded_symbols, nb):
    torch, sora = env
    x = coded_symbols[nb]
    want = M.interleave(x, nb)
    for n in NSYMS:
        got = sora.interleave11a(dev(torch, x[:n]), nb).cpu().numpy()
        assert np.array_equal(got, want[:n]), n


@pytest.mark.parametrize("nb", [1, 2, 4, 6])
def test_map(env, coded_symbols, nb):
    torch, sora = env
    x = coded_symbols[nb]
    for mod in (0, 30339):                                                       # the 802.11a default; the 802.11n graph's BPSK amplitude (QAM levels wrap like the brick's short)
        want = M.map11a(x, nb, mod)
        for n in NSYMS:
            got = sora.map11a(dev(torch, x[:n]), nb, mod).cpu().numpy()
            assert np.array_equal(got, want[:n]), (mod, n)


def test_add_pilot(env):
    torch, sora = env
    rng = np.random.default_rng(30)
    nsym = [1, 2, 127, 128, 129, 300] + [1, 17, 16, 15, 33, 5, 2]                # the index wrap; a batch whose frames do not tile a workgroup's 16 symbols
    first = np.cumsum([0] + [n + (i % 3) for i, n in enumerate(nsym[:-1])]) + 2  # symbols no frame owns lie between
    total = int(first[-1] + nsym[-1] + 3)
    car = rng.integers(-32768, 32768, (total, 48, 2)).astype(np.int16)
    for mod in (0, 30339):
        want = np.zeros((total, 64, 2), np.int16)
        for f, n in zip(first, nsym):
            want[f:f + n] = M.add_pilot(car[f:f + n], mod or M.BPSK_MOD)
        got = sora.add_pilot11a(dev(torch, car), i32(torch, first), i32(torch, nsym), bpsk_mod=mod).cpu().numpy()
        assert np.array_equal(got, want), mod
    for n in NSYMS:                                                              # one frame of n symbols
        got = sora.add_pilot11a(dev(torch, car[:n]), i32(torch, [0]), i32(torch, [n])).cpu().numpy()
        assert np.array_equal(got, M.add_pilot(car[:n])), n
    # a frame continued from position 200 (what a brick adapter asks for burst by burst)
    whole = M.add_pilot(car[:300])
    got = sora.add_pilot11a(dev(torch, car[200:300]), i32(torch, [0]), i32(torch, [100]), pos0=i32(torch, [200])).cpu().numpy()
    assert np.array_equal(got, whole[200:300])


@pytest.fixture(scope="module")
def ifftx_cases():
    rng = np.random.default_rng(40)
    n = max(NSYMS)
    x = np.zeros((n, 64, 2), np.int16)
    x[:64] = rng.integers(-300, 301, (64, 64, 2)); x[64:128] = rng.integers(-11000, 11001, (64, 64, 2)); x[128:n - 65] = rng.integers(-32768, 32768, (n - 193, 64, 2))
    x[n - 65] = np.where(rng.integers(0, 2, (64, 2)) == 1, 32767, -32767)        # every bin at a rail: the saturating butterflies
    for b in range(64):                                                          # a single tone per bin
        x[n - 64 + b, b] = (32767, -32767) if b & 1 else (-32767, 32767)
    extra = np.stack([np.full((64, 2), 32767), np.full((64, 2), -32767), np.where(rng.integers(0, 2, (64, 2)) == 1, 32767, -32767)]).astype(np.int16)
    x = np.concatenate([x, extra])
    return x, M.ifftx(x)


def test_ifftx(env, ifftx_cases):
    torch, sora = env
    x, want = ifftx_cases
    got = sora.ifftx11a(dev(torch, x)).cpu().numpy()
    bad = np.flatnonzero((got != want).any(axis=(1, 2)))
    assert len(bad) == 0, bad[:10]
    for n in NSYMS:
        got = sora.ifftx11a(dev(torch, x[len(x) - n:])).cpu().numpy()            # (the tail holds the full-scale and single-tone symbols)
        assert np.array_equal(got, want[len(x) - n:]), n


def test_pack16to8(env):
    torch, sora = env
    rng = np.random.default_rng(50)
    edge = np.array([-32768, -32767, -130, -129, -128, -127, -1, 0, 1, 126, 127, 128, 129, 32766, 32767], np.int16)
    for n in NSYMS:
        x = rng.integers(-300, 301, (160 * n, 2)).astype(np.int16)
        x[:len(edge) * 2] = rng.choice(edge, (len(edge) * 2, 2))
        x[-15:, 0] = edge; x[-15:, 1] = edge[::-1]
        got = sora.pack16to8(dev(torch, x)).cpu().numpy()
        assert np.array_equal(got, M.pack16to8(x)), n
    x = np.stack([np.repeat(edge, 15), np.tile(edge, 15)], 1)[:224]              # every pair of edge values, 28 bursts
    assert np.array_equal(sora.pack16to8(dev(torch, x)).cpu().numpy(), M.pack16to8(x))
    with pytest.raises(sora.SoraError):
        sora.pack16to8(dev(torch, x[:12]))


def test_upsample40to44(env):
    torch, sora = env
    rng = np.random.default_rng(60)
    for n in NSYMS:
        x = rng.integers(-32768, 32768, (n, 160, 2)).astype(np.int16)
        x[0, :8] = 32767; x[-1, -8:] = -32768; x[n // 2, ::2] = 32767; x[n // 2, 1::2] = -32768      # rails
        sees = rng.integers(0, 2, n).astype(np.uint8)
        got = sora.upsample40to44(dev(torch, x), dev(torch, sees)).cpu().numpy()
        assert np.array_equal(got.reshape(-1, 2), up40to44(x.reshape(-1, 2), sees)), n
        got = sora.upsample40to44(dev(torch, x)).cpu().numpy()                   # no array: x[160] = 0 everywhere
        assert np.array_equal(got.reshape(-1, 2), up40to44(x.reshape(-1, 2), np.zeros(n, np.uint8))), n
    x = rng.integers(-32768, 32768, (5, 160, 2)).astype(np.int16)
    x[:, 0] = (32767, -32768)                                                    # the sample a block may see
    for pat in range(32):                                                        # every sees_next pattern over five blocks (the last block never sees one)
        sees = np.array([(pat >> b) & 1 for b in range(5)], np.uint8)
        got = sora.upsample40to44(dev(torch, x), dev(torch, sees)).cpu().numpy()
        assert np.array_equal(got.reshape(-1, 2), up40to44(x.reshape(-1, 2), sees)), pat


def test_preamble(env, oracle):
    torch, sora = env
    want = M.preamble()
    for n in (1, 3, 2049):
        got = sora.preamble11a(n).cpu().numpy()
        assert got.shape == (n, 640, 2) and (got == want[None]).all(), n
    assert np.array_equal(M.pack16to8(want), oracle.tx(b"x", 6000)[:640])


@pytest.fixture(scope="module")
def frames(oracle):
    """all eight rates x lengths 1, 37, 260, 1496; seeds so that frames with samples at the int8 rail (seeds 0 and 1: the all-zero scrambler) are among them"""
    out = []
    for i, rate in enumerate(RATES):
        for j, ln in enumerate((1, 37, 260, 1496)):
            seed = (0x00, 0xFF, 0x01, 0x5B)[(i + j) % 4]
            out.append((bytes(np.random.default_rng([rate, ln]).integers(0, 256, ln).astype(np.uint8)), rate, seed))
    want40 = [oracle.tx(*f) for f in out]
    assert sum(has_rail(w) for w in want40) >= 8 and sum(not has_rail(w) for w in want40) >= 8
    return out, want40


@pytest.mark.parametrize("mhz", [40, 44])
def test_chain_of_stages_equals_the_fused_transmitter(env, frames, mhz):
    torch, sora = env
    fr, want40 = frames
    mp, rates, seeds = [f[0] for f in fr], [f[1] for f in fr], [f[2] for f in fr]
    a, aoff = sora.mod11a_by_stages(mp, rates, seeds, sample_rate_mhz=mhz)
    b, boff = sora.tx11a(mp, rates, seeds, sample_rate_mhz=mhz)
    assert aoff == boff
    a, b = a.cpu().numpy(), b.cpu().numpy()
    assert a.shape == b.shape
    for f in range(len(fr)):
        assert np.array_equal(a[aoff[f]:aoff[f + 1]], b[boff[f]:boff[f + 1]]), (fr[f][1], len(fr[f][0]), fr[f][2])
    if mhz == 40:                                                                # ... and the oracle's transmitter
        for f, w in enumerate(want40):
            assert np.array_equal(a[aoff[f]:aoff[f + 1]], w), f


def test_chain_of_one_frame_and_of_one_modulation(env, oracle):
    """batches in which some modulation's run of symbols is empty"""
    torch, sora = env
    for rates in ([54000], [6000, 9000], [12000, 48000, 18000]):
        mp = [bytes(np.random.default_rng(r).integers(0, 256, 100 + r // 1000).astype(np.uint8)) for r in rates]
        a, off = sora.mod11a_by_stages(mp, rates)
        a = a.cpu().numpy()
        for f, r in enumerate(rates):
            assert np.array_equal(a[off[f]:off[f + 1]], oracle.tx(mp[f], r, 0xFF)), rates
