"""GPU parity of the oldest stage entry points -- sora_hip_lts11a, _symfront11a, _pilot_track11a, _pilot11a (behind _phase_comp11a), _demap11a, _deinterleave11a:
k_lts_batch, k_symfront_batch, k_ptrack_batch<true|false>, k_demap_batch<NB>, k_deint_batch<NB> of k_stage.hip -- and of the thin 802.11n rows (demap11n,
sig_demap11n, siso_est11n, mimo_est11n) on the families of tests/stage_edge_cases.py: rails, zeros, nulled bins, the carrier-offset sum past 2^31, symbol_count
past 126, the demap clamp edges, per-carrier singular channels, and row counts around every kernel's tile.  Every row and every state word against the oracle, which
tests/test_stage_edges_cpu.py pins to the reference's own bricks on the same families.  0 LSB everywhere; one test per entry point."""
import numpy as np
import pytest

import stage_edge_cases as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import torch
    import sora_amd
    sora_amd.load()
    assert torch.cuda.is_available() and sora_amd.device_count() > 0
    return torch, sora_amd


@pytest.fixture(scope="module")
def lts(oracle):
    names, x = sc.lts_cases(oracle)
    return names, x, sc.run_lts(sc.Engine(oracle), x)[0]


@pytest.fixture(scope="module")
def track(oracle):
    fr = sc.track_frames(oracle)
    return fr, sc.run_track(sc.Engine(oracle), fr)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _rows(a, b):
    return np.argwhere((a != b).reshape(len(a), -1).any(1)).ravel()[:8].tolist()


def test_lts11a(env, lts):
    """all 258 words of every record (cfo_est, the reserved word, FreqCoeffs, ChannelCoeffs with bins 28..35 zero), at 1, 2, 63, 64, 65 and all frames, taken
    from both ends of the family"""
    _, sora = env
    names, x, want = lts
    assert len(x) > max(sc.LTS_ROWS)
    for k in sc.LTS_ROWS + (len(x),):
        for sl in (slice(0, k), slice(len(x) - k, len(x))):
            got = sora.lts11a(_dev(x[sl])).cpu().numpy()
            assert got.shape == (k, 258)
            assert np.array_equal(got, want[sl]), (k, [names[sl][i] for i in _rows(got, want[sl])])
            assert not got[:, 130 + 2 * 28:130 + 2 * 36].any() and not got[:, 1].any()


def test_symfront11a(env, oracle, lts):
    """every symbol kind under every context: the LTS family's own records and full-range coefficient sets; ctx_index given (unsorted, repeats) at every row count
    around the 16-symbol tile and the 64-symbol block, and NULL with one context"""
    _, sora = env
    x = sc.symfront_symbols(); cr = np.concatenate([lts[2], sc.random_ctx_records()]); idx = sc.symfront_index(len(x), len(cr))
    assert len(x) == max(sc.SYMFRONT_ROWS) and set(idx.tolist()) == set(range(len(cr))) and (np.diff(idx) < 0).any()
    want = sc.run_symfront(sc.Engine(oracle), x, cr, idx)
    ctx = _dev(cr)
    for k in sc.SYMFRONT_ROWS:
        got = sora.symfront11a(_dev(x[:k]), ctx, _dev(idx[:k])).cpu().numpy()
        assert np.array_equal(got, want[:k]), (k, _rows(got, want[:k]))
    zero = np.zeros(17, np.int32)
    for c in (0, 2, lts[0].index("tx_level65534"), lts[0].index("tx_echo0"), len(lts[2]), len(lts[2]) + 1, len(cr) - 1):
        got = sora.symfront11a(_dev(x[:17]), _dev(cr[c:c + 1])).cpu().numpy()
        w = sc.run_symfront(sc.Engine(oracle), x[:17], cr[c:c + 1], zero)
        assert np.array_equal(got, w), (c, _rows(got, w))


def test_pilot_track11a(env, track):
    """TPhaseCompensate + TPilotTrack fused: frames of 0 .. 300 symbols laid out unsorted with gaps, from the reset state and from arbitrary records; every row
    (the gaps stay zero) and all 134 words of every state record"""
    _, sora = env
    fr, (want, _, end) = track
    st = _dev(fr["state0"])
    got = sora.pilot_track11a(_dev(fr["eq"]), _dev(fr["first"]), _dev(fr["nsym"]), st).cpu().numpy()
    assert np.array_equal(got, want), _rows(got, want)
    assert np.array_equal(st.cpu().numpy(), end), _rows(st.cpu().numpy(), end)
    inside = np.zeros(len(want), bool)
    for a, n in zip(fr["first"], fr["nsym"]):
        inside[a:a + n] = True
    assert not got[~inside].any() and (~inside).sum() > 10 and got[inside].any()


def test_pilot11a_whole_frames(env, track):
    """TPhaseCompensate and TPilotTrack as two entry points on whole frames: phase_comp11a with one state record per symbol (the record the tracker had before
    that symbol), then pilot11a over every frame in ONE call -- the outputs and the state pilot_track11a leaves"""
    torch, sora = env
    fr, (want, states, end) = track
    before = np.tile(sc.reset_state(), (len(want), 1))
    for f in range(len(fr["first"])):
        a, n = int(fr["first"][f]), int(fr["nsym"][f])
        if n:
            before[a] = fr["state0"][f]; before[a + 1:a + n] = states[a:a + n - 1]
    pcs = sora.phase_comp11a(_dev(fr["eq"]), _dev(before), torch.arange(len(want), dtype=torch.int32).cuda())
    st = _dev(fr["state0"])
    got = sora.pilot11a(pcs, _dev(fr["first"]), _dev(fr["nsym"]), st).cpu().numpy()
    assert np.array_equal(got, want), _rows(got, want)
    assert np.array_equal(st.cpu().numpy(), end), _rows(st.cpu().numpy(), end)


def test_pilot11a_symbol_by_symbol(env, track):
    """the same two entry points symbol by symbol, as the reference's graph runs them, for every frame of at most 128 symbols (all of them in step): after each
    symbol the state record on the device is the next symbol's phase compensation"""
    torch, sora = env
    fr, (want, _, end) = track
    nf = len(fr["first"])
    short = fr["nsym"] <= 128
    assert short.sum() >= 25 and fr["nsym"][short].max() == 128
    eq = _dev(fr["eq"]); st = _dev(fr["state0"])
    got = np.zeros_like(want)
    for s in range(128):
        act = np.flatnonzero(short & (fr["nsym"] > s)).astype(np.int32)
        rows = fr["first"][act] + s
        pcs = sora.phase_comp11a(eq[torch.from_numpy(rows.astype(np.int64)).cuda()].contiguous(), st, _dev(act))
        first = np.zeros(nf, np.int32); n1 = np.zeros(nf, np.int32)
        first[act] = np.arange(len(act)); n1[act] = 1
        got[rows] = sora.pilot11a(pcs, _dev(first), _dev(n1), st).cpu().numpy()
    sth = st.cpu().numpy()
    for f in np.flatnonzero(short):
        a, n = int(fr["first"][f]), int(fr["nsym"][f])
        assert np.array_equal(got[a:a + n], want[a:a + n]), (f, _rows(got[a:a + n], want[a:a + n]))
        assert np.array_equal(sth[f], end[f]), f
    assert np.array_equal(sth[~short], fr["state0"][~short])


@pytest.mark.parametrize("nb", [1, 2, 4, 6])
def test_demap11a(env, oracle, nb):
    """uniform full range, every multiple of 16 with -1, 0, +1 across +-2100 (both clamp edges of re >> 4 from both sides) and the rails, around the 32-symbol tile"""
    _, sora = env
    x = sc.demap_symbols()
    want = np.stack([oracle.demap(nb, s) for s in x])
    for k in sc.DEMAP_ROWS:
        got = sora.demap11a(_dev(x[:k]), nb).cpu().numpy()
        assert np.array_equal(got, want[:k]), (k, _rows(got, want[:k]))
    got = sora.demap11a(_dev(x[-33:]), nb).cpu().numpy()
    assert np.array_equal(got, want[-33:])


@pytest.mark.parametrize("nb", [1, 2, 4, 6])
def test_deinterleave11a(env, oracle, nb):
    """the permutation itself through two byte planes, and random bytes of all 256 values, around the 32-symbol tile"""
    _, sora = env
    s = sc.deint_bytes(nb)
    want = np.stack([oracle.deinterleave(nb, r) for r in s])
    for k in sc.DEMAP_ROWS:
        got = sora.deinterleave11a(_dev(s[:k]), nb).cpu().numpy()
        assert np.array_equal(got, want[:k]), (k, _rows(got, want[:k]))
    g = sora.deinterleave11a(_dev(s[:2]), nb).cpu().numpy().astype(int)
    assert sorted((g[0] | (g[1] << 8)).tolist()) == list(range(48 * nb))


def test_demap11n_and_sig_demap11n(env, oracle):
    _, sora = env
    x = sc.demap11n_symbols()
    for nb in (1, 2, 4, 6):
        got = sora.demap11n(_dev(x), nb).cpu().numpy()
        want = np.stack([oracle.demap11n(nb, s) for s in x])
        assert np.array_equal(got, want), (nb, _rows(got, want))
    sig = sc.sig_demap11n_symbols()
    got = sora.sig_demap11n(_dev(sig)).cpu().numpy()
    want = np.stack([oracle.sig_demap11n(s) for s in sig])
    assert np.array_equal(got, want), _rows(got, want)


def test_siso_est11n(env, oracle):
    """both chains at full scale, on the rails, at zero, and with one chain zero"""
    _, sora = env
    l0, l1 = sc.siso_est11n_lltfs()
    got = sora.siso_est11n(_dev(l0), _dev(l1)).cpu().numpy()
    want = np.stack([oracle.siso_est11n(a, b) for a, b in zip(l0, l1)])
    assert np.array_equal(got, want), _rows(got, want)


def test_mimo_est11n(env, oracle):
    """zero LTFs, rails, one chain zero, channels singular on 1 .. 55 carriers only, amplitudes 1 .. 3"""
    _, sora = env
    l0, l1 = sc.mimo_est11n_ltfs()
    h, hinv = (t.cpu().numpy() for t in sora.mimo_est11n(_dev(l0), _dev(l1)))
    for i in range(len(l0)):
        wh, whi = oracle.mimo_est11n(l0[i], l1[i])
        assert np.array_equal(h[i], wh) and np.array_equal(hinv[i], whi), i
