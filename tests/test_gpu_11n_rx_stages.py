"""GPU parity of the stages that complete the 802.11n receive graph (sora_amd/csrc/k_11n.hip: sora_hip_cca11n, _data_symbol11n, _stream_join11n, _desc11a, _frame_sink11a)
against the per-brick model of tests/rx11n_stage_model.py (pinned to the oracle by tests/test_11n_stage_model_cpu.py): output, record and d_used bit for bit, over ragged,
unaligned stream tables with guards around every output; and their composition, sora_amd.rx11n_by_stages, against the model's composition in every intermediate and against
the sora_rx11n_* handle's first row per capture.  The carrier-sense streams are those whose branches the CPU test counts."""
import os
import zlib

import numpy as np
import pytest

import rx11n_stage_cases as cases
import rx11n_stage_model as model
from sora_amd import capi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD16, GUARD8, GUARD32 = 0x5A5A, 0xA5, 0x5A5AA5A5
TILE_BURSTS = 64                                                                 # k_cca11n's tile: 256 samples
E_FRAME_OK, E_PLCP, E_CRC32_FAIL, E_CS_TIMEOUT = 0x1, 0x80000005, 0x80000006, 0x80000007


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
    return dev(torch, (np.asarray(a, np.int64) & 0xFFFFFFFF).astype(np.uint32).view(np.int32))


def ragged(rng, sizes, lead=3):
    """-> (first element of each stream, total): gaps of 1 .. 6 elements between the streams: nothing is aligned"""
    first, at = [], lead
    for s in sizes:
        first.append(at); at += int(s) + int(rng.integers(1, 7))
    return np.asarray(first, np.int64), at + 5


# ------------------------------------------------------------------ TCCA11n
@pytest.fixture(scope="module")
def cca_streams():
    rng = np.random.default_rng(2026)
    return [(a, b) for _, a, b in cases.built_streams()] + cases.lengths_streams(rng, TILE_BURSTS)


def gpu_cca(env, rng, streams, states, flags, n=None):
    """one call over the batch, the streams laid out ragged in one buffer per chain, guard records and counts around the tables -> (states after, used)"""
    torch, sora = env
    n = np.array([len(a) // 4 for a, _ in streams], np.int64) if n is None else np.asarray(n, np.int64)
    first, total = ragged(rng, [len(a) for a, _ in streams])
    x0 = rng.integers(-32768, 32768, (total, 2)).astype(np.int16); x1 = rng.integers(-32768, 32768, (total, 2)).astype(np.int16)
    for f, (a, b) in zip(first, streams):
        x0[f:f + len(a)] = a; x1[f:f + len(b)] = b
    ns = len(streams)
    st = np.full((ns + 2, capi.CCA11N_WORDS), GUARD32, np.int32); st[1:-1] = states
    d_st = dev(torch, st); d_used = dev(torch, np.full(ns + 2, GUARD32, np.int32))
    load = sora.load()
    d_x0, d_x1, d_first, d_n = dev(torch, x0), dev(torch, x1), i32(torch, first), i32(torch, n)      # (held until the call has run)
    rc = load.sora_hip_cca11n(d_x0.data_ptr(), d_x1.data_ptr(), d_first.data_ptr(), d_n.data_ptr(), d_st[1:].data_ptr(), d_used[1:].data_ptr(), ns,
                              int(n.max()) if ns else 0, int(flags), None)
    assert rc == 0, load.sora_hip_last_error()
    torch.cuda.synchronize()
    st = d_st.cpu().numpy(); used = d_used.cpu().numpy()
    assert (st[0] == GUARD32).all() and (st[-1] == GUARD32).all() and used[0] == GUARD32 and used[-1] == GUARD32
    return st[1:-1], used[1:-1]


def model_cca(streams, states, flags, n=None):
    st = np.array(states, np.int32); used = np.zeros(len(streams), np.int32)
    for f, (a, b) in enumerate(streams):
        k = len(a) // 4 if n is None else int(n[f])
        st[f], used[f] = model.cca(a[:4 * k], b[:4 * k], states[f], flags)
    return st, used


def same_cca(got, want, what):
    (gs, gu), (ws, wu) = got, want
    assert np.array_equal(gu, wu), (what, np.flatnonzero(gu != wu)[:8], gu[gu != wu][:8], wu[gu != wu][:8])
    bad = np.flatnonzero((gs != ws).any(axis=1))
    assert len(bad) == 0, (what, bad[:8], [np.flatnonzero(gs[b] != ws[b])[:6].tolist() for b in bad[:4]])


@pytest.mark.parametrize("flags", [0, capi.CCA11N_REARM])
def test_cca_equals_the_model_in_one_call_and_in_two(env, cca_streams, flags):
    rng = np.random.default_rng(31 + flags)
    ns = len(cca_streams)
    fresh = capi.cca11n_states(ns)
    want = model_cca(cca_streams, fresh, flags)
    same_cca(gpu_cca(env, rng, cca_streams, fresh, flags), want, "one call")
    assert (want[0][:, 0] == 1).sum() >= 1 and (want[1] == 0).sum() >= 1        # detections; the stream of 0 bursts
    if flags:
        assert (want[0][:, 0] == 1).sum() >= 20 and (want[0][:, 7] >= 2).sum() >= 20 and (want[0][:, 1] == 0).all()
    else:
        assert ((want[0][:, 1].astype(np.int64) & 0xFFFFFFFF) == E_CS_TIMEOUT).sum() >= 20
    nb = np.array([len(a) // 4 for a, _ in cca_streams], np.int64); used = want[1].astype(np.int64)
    for what, cut in (("at 1", np.minimum(1, nb)), ("before the deciding burst", np.maximum(used - 1, 0)), ("at the deciding burst", used),
                      ("behind the deciding burst", np.minimum(used + 1, nb)), ("at n - 1", np.maximum(nb - 1, 0))):
        mid, u1 = gpu_cca(env, rng, cca_streams, fresh, flags, n=cut)
        same_cca((mid, u1), model_cca(cca_streams, fresh, flags, n=cut), "first part, cut " + what)
        rest = [(a[4 * int(k):], b[4 * int(k):]) for (a, b), k in zip(cca_streams, u1)]
        end, u2 = gpu_cca(env, rng, rest, mid, flags)
        same_cca((end, u1 + u2), want, "second part, cut " + what)


@pytest.mark.parametrize("nstreams", [1, 3, 64, 257])
def test_cca_batches(env, cca_streams, nstreams):
    rng = np.random.default_rng(nstreams)
    pick = [cca_streams[int(i)] for i in rng.permutation(len(cca_streams))[:nstreams]] if nstreams <= len(cca_streams) else \
           [cca_streams[i % len(cca_streams)] for i in range(nstreams)]
    pick = [(a[4 * (i % 3):], b[4 * (i % 3):]) for i, (a, b) in enumerate(pick)]  # (and not the same stream twice over)
    fresh = capi.cca11n_states(len(pick))
    same_cca(gpu_cca(env, rng, pick, fresh, capi.CCA11N_REARM), model_cca(pick, fresh, capi.CCA11N_REARM), nstreams)


def test_cca_second_frames_and_streams_that_enter_decided(env):
    """a detection, the frame's bursts withheld, the brick Reset, the same record again: the slipped ring; and records that enter with power detected or an error standing"""
    rng = np.random.default_rng(9)
    two = [(a, b) for name, a, b in cases.built_streams() if name.startswith("two")]
    fresh = capi.cca11n_states(len(two))
    st, used = gpu_cca(env, rng, two, fresh, capi.CCA11N_REARM)
    same_cca((st, used), model_cca(two, fresh, capi.CCA11N_REARM), "first frame")
    assert (st[:, 0] == 1).all() and (st[:, 6] % 4 != 0).any()
    decided = st.copy(); decided[1, 1] = np.int32(E_CS_TIMEOUT - (1 << 32)); decided[1, 0] = 0
    same_cca(gpu_cca(env, rng, two, decided, capi.CCA11N_REARM), (decided, np.zeros(len(two), np.int32)), "enters decided")
    again = st.copy(); again[:, 0] = 0; again[:, 3:6] = 0
    rest = [(a[4 * (int(k) + 330):], b[4 * (int(k) + 330):]) for (a, b), k in zip(two, used)]
    want = model_cca(rest, again, capi.CCA11N_REARM)
    same_cca(gpu_cca(env, rng, rest, again, capi.CCA11N_REARM), want, "second frame")
    assert (want[0][:, 0] == 1).all()


# ------------------------------------------------------------------ T11nDataSymbol
@pytest.mark.parametrize("shift", [0, 1])
def test_data_symbol(env, shift):
    """0, 1, 2, 7 and 300 symbols per frame at every d_first mod 4; shift 1: the output buffers start one sample off 16-byte alignment"""
    torch, sora = env
    rng = np.random.default_rng(5 + shift)
    nsym = np.array([k for k in (0, 1, 2, 7, 300) for _ in range(4)], np.int64)
    first, at = [], 0
    for i, k in enumerate(nsym):
        at += int(rng.integers(1, 5)) * 4; first.append(at + i % 4); at += 80 * int(k) + 4
    first = np.array(first, np.int64); total = at + 8
    assert sorted(set((first % 4).tolist())) == [0, 1, 2, 3]
    x = [rng.integers(-32768, 32768, (total, 2)).astype(np.int16) for _ in range(2)]
    out_first = np.concatenate([[1], 1 + np.cumsum(nsym + 1)])[:-1]
    out_total = int(out_first[-1] + nsym[-1] + 2) * 64
    blank = np.full((out_total + shift, 2), GUARD16, np.uint16).view(np.int16)
    want = [blank.copy(), blank.copy()]
    for f, k, o in zip(first, nsym, out_first):
        for c in range(2):
            want[c][shift + 64 * o:shift + 64 * (o + k)] = model.data_symbol(x[c][f:f + 80 * k], int(k))
    d_out = [dev(torch, blank), dev(torch, blank)]
    sora.data_symbol11n(dev(torch, x[0]), dev(torch, x[1]), i32(torch, first), i32(torch, nsym), i32(torch, out_first), d_out[0][shift:], d_out[1][shift:])
    for c in range(2):
        got = d_out[c].cpu().numpy()
        assert np.array_equal(got, want[c]), (c, np.flatnonzero((got != want[c]).any(axis=1))[:8])
    assert not np.array_equal(want[0], blank)


# ------------------------------------------------------------------ TStreamJoin + TStreamConcat
@pytest.mark.parametrize("nb", [1, 2, 4, 6])
def test_stream_join(env, nb):
    torch, sora = env
    rng = np.random.default_rng(nb)
    for n in (0, 1, 3, 64, 1025):
        for shift in (0, 1) if n in (3, 64) else (0,):                           # shift 1: no buffer is 16-byte aligned
            s0 = rng.integers(0, 256, (n, 52 * nb)).astype(np.uint8); s1 = rng.integers(0, 256, (n, 52 * nb)).astype(np.uint8)
            pad = np.zeros(16, np.uint8)                                         # (n = 0: a buffer all the same; a null pointer is refused first)
            d0 = dev(torch, np.concatenate([pad[:shift], s0.reshape(-1), pad])); d1 = dev(torch, np.concatenate([pad[:shift], s1.reshape(-1), pad]))
            d_out = dev(torch, np.full(shift + n * 104 * nb + 64, GUARD8, np.uint8))
            rc = sora.load().sora_hip_stream_join11n(d0[shift:].data_ptr(), d1[shift:].data_ptr(), d_out[shift:].data_ptr(), nb, n, None)
            assert rc == 0, sora.load().sora_hip_last_error()
            got = d_out.cpu().numpy()
            assert np.array_equal(got[shift:shift + n * 104 * nb], model.stream_join(s0, s1, nb).reshape(-1)), (nb, n, shift)
            assert (got[:shift] == GUARD8).all() and (got[shift + n * 104 * nb:] == GUARD8).all(), (nb, n, shift)


def test_stream_join_refuses_three_bits(env):
    torch, sora = env
    z = dev(torch, np.zeros(4096, np.uint8))
    with pytest.raises(sora.SoraError):
        sora.stream_join11n(z[:156].reshape(1, 156), z[256:412].reshape(1, 156), 3)


# ------------------------------------------------------------------ T11aDesc, TBB11aFrameSink
@pytest.mark.parametrize("nframes", [1, 5, 257])
def test_desc_and_frame_sink(env, nframes):
    """lengths 4, 5, 14, 1500 and 4095 with a good FCS and a corrupted one (and, for the sink, lengths below 4 and behind its LDS buffer), at odd offsets"""
    torch, sora = env
    from oracle.pyoracle import Oracle
    from test_11n_stage_model_cpu import tail_cases
    rng = np.random.default_rng(100 + nframes)
    pool = tail_cases(Oracle(), rng)
    fr = [pool[(3 * i + 7) % len(pool)] if nframes > 1 else pool[6] for i in range(nframes)]
    if nframes >= 5:
        for i, L in enumerate((0, 1, 2, 3)):
            fr[i + 1] = (rng.integers(0, 256, L + 2, dtype=np.uint8), L, False)
    if nframes > 5:
        body = rng.integers(0, 256, 4996, dtype=np.uint8).tobytes()
        dec = np.zeros(5002, np.uint8); dec[2:] = np.frombuffer(body + (zlib.crc32(body) & 0xFFFFFFFF).to_bytes(4, "little"), np.uint8)   # seed 0: the register stays 0
        fr[7] = (dec, 5000, True)
    lens = np.array([L for _, L, _ in fr], np.int64)
    off, total = ragged(rng, lens + 2); off |= 1
    out_off, out_total = ragged(rng, lens, lead=1); out_off |= 1
    buf = rng.integers(0, 256, total + 2).astype(np.uint8)
    for (dec, L, _), a in zip(fr, off):
        buf[a:a + L + 2] = dec
    blank = np.full(out_total + 2, GUARD8, np.uint8); want = blank.copy(); wrec = np.zeros((nframes, 2), np.uint32)
    for i, ((dec, L, good), o) in enumerate(zip(fr, out_off)):
        want[o:o + L] = model.desc(dec, L)
        wrec[i] = model.frame_sink(want[o:o + L], L)
        if L >= 4:
            assert wrec[i, 0] == (E_FRAME_OK if good else E_CRC32_FAIL)
    d_out = dev(torch, blank)
    sora.desc11a(dev(torch, buf), i32(torch, off), i32(torch, lens), d_out, i32(torch, out_off))
    got = d_out.cpu().numpy()
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]
    d_rec = dev(torch, np.full((nframes + 2, 2), GUARD32, np.int32))
    d_off, d_len = i32(torch, out_off), i32(torch, lens)
    rc = sora.load().sora_hip_frame_sink11a(d_out.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), d_rec[1:].data_ptr(), nframes, None)
    assert rc == 0, sora.load().sora_hip_last_error()
    rec = d_rec.cpu().numpy()
    assert np.array_equal(rec[1:-1].view(np.uint32), wrec), np.flatnonzero((rec[1:-1].view(np.uint32) != wrec).any(axis=1))[:8]
    assert (rec[0] == GUARD32).all() and (rec[-1] == GUARD32).all()


# ------------------------------------------------------------------ the composition
def composition_captures(sora):
    """24 two-chain captures of one whole frame each: MCS 8..14 x PSDU lengths 14, 100, 257 behind leads of 200 .. 2000 samples through identity and cross-talk channels
    with a CFO, one with a payload symbol blanked (CRC), one with HT-SIG 1 negated (header), one of noise only -> (captures, the gate each needs)"""
    import rx11n_ext_model as ext
    rng = np.random.default_rng(20261020)
    plan = [(8 + k % 7, (14, 100, 257)[(k // 7 + k) % 3]) for k in range(21)] + [(10, 257), (9, 100)]
    o0, o1, off = sora.tx11n([rng.integers(0, 256, L - 4).astype(np.uint8).tobytes() for _, L in plan], [m for m, _ in plan])
    a, b = o0.cpu().numpy(), o1.cpu().numpy()
    caps = []
    for i, (mcs, L) in enumerate(plan):
        s0 = a[off[i]:off[i + 1]].copy(); s1 = b[off[i]:off[i + 1]].copy()
        if i == 21:
            s0[1600 + 3 * 160:1600 + 4 * 160] = 0; s1[1600 + 3 * 160:1600 + 4 * 160] = 0      # the fourth data symbol (40 MHz: 1600 samples of preamble, 160 per symbol)
        if i == 22:
            s0[800:960] = -s0[800:960]; s1[800:960] = -s1[800:960]                             # HT-SIG 1
        caps.append(ext.clean_channel(rng, s0, s1, sigma=float(rng.uniform(10, 20)), lead=int(rng.integers(200, 2001))))
    n = 28 * 150
    caps.append(tuple(np.rint(rng.normal(0, 30, (n, 2))).astype(np.int16) for _ in range(2)))
    return caps, [m for m, _ in plan] + [10]


def test_rx11n_by_stages_equals_the_model_composition_and_the_handle(env):
    torch, sora = env
    caps, mcs = composition_captures(sora)
    key = lambda r: None if r is None else (r["error_code"], r["rate_kbps"], r["length"], r["crc32"], r["mpdu"])
    seen = []
    for gate, idx in ((10, [i for i, m in enumerate(mcs) if m <= 10]), (14, [i for i, m in enumerate(mcs) if m > 10])):
        sub = [caps[i] for i in idx]
        iq0 = np.ascontiguousarray(np.concatenate([a for a, _ in sub])); iq1 = np.ascontiguousarray(np.concatenate([b for _, b in sub]))
        lens = np.array([len(a) for a, _ in sub]); offs = np.concatenate([[0], np.cumsum(lens)])[:-1]
        descs = [(int(o), int(n)) for o, n in zip(offs, lens)]
        tg, tm = [], []
        got = sora.rx11n_by_stages(dev(torch, iq0), dev(torch, iq1), descs, mcs_max=gate, trace=tg)
        want = model.first_events(iq0, iq1, descs, mcs_max=gate, trace=tm)
        for (name, g), (wname, w) in zip(tg, tm):                                # every intermediate the walk hands on, in its order
            assert name == wname and g.shape == w.shape, (gate, name, wname, g.shape, w.shape)
            assert np.array_equal(g.view(np.uint8), w.view(np.uint8)), (gate, name, np.flatnonzero((g != w).reshape(len(g), -1).any(axis=1))[:8])
        assert [n for n, _ in tg] == [n for n, _ in tm] and len(tg) > 15
        assert [key(r) for r in got] == [key(r) for r in want], gate
        rx = sora.Rx11n(len(sub), len(iq0))
        if gate != 10:
            assert rx.set_mcs_max(gate) == 10
        rx.process_dev(dev(torch, iq0), dev(torch, iq1), [(o, n, i) for i, (o, n) in enumerate(descs)])
        rows = rx.results(); rx.close()
        first = [None] * len(sub)
        for r in sorted(rows, key=lambda r: r["end_sample"]):
            if first[r["capture_id"]] is None:
                first[r["capture_id"]] = r
        hkey = lambda r: None if r is None else (r["error_code"], r["rate_kbps"], r["length"], r["crc32"], r["mpdu"]) if r["error_code"] != E_PLCP else (E_PLCP, 0, 0, 0, b"")
        assert [key(r) for r in got] == [hkey(r) for r in first], gate
        seen += [(mcs[i], r["error_code"] if r else None) for i, r in zip(idx, got)]
    assert len(seen) == 24
    assert {m for m, e in seen if e == E_FRAME_OK} == set(range(8, 15)) and [e for _, e in seen].count(E_CRC32_FAIL) == 1
    assert [e for _, e in seen].count(E_PLCP) == 1 and [e for _, e in seen].count(None) == 1


# ------------------------------------------------------------------ the C++ host
def test_rx11n_tail_chain_host(env):
    """tests/cxx/rx11n_tail_chain.cpp: de-interleaved soft bytes -> THip11nStreamJoin -> the trellis stage -> THip11aDesc -> the frame sink, against this process's stages"""
    from test_gpu_hosts import build, run
    out = run([build("g++", "-std=c++17", os.path.join(ROOT, "tests", "cxx", "rx11n_tail_chain.cpp"), "rx11n_tail_chain")])
    lines = dict(l.split("=", 1) for l in out.split() if "=" in l)
    payload = bytes((37 * i + 11) & 0xFF for i in range(96))
    assert lines["decided"] == "1" and lines["error_code"] == "0x1" and int(lines["crc32"], 16) == zlib.crc32(payload) & 0xFFFFFFFF and int(lines["length"]) == 100
