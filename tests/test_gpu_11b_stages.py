"""GPU parity of the 802.11b receive graph's stage entry points (sora_amd/csrc/k_11b.hip) against the per-brick C model of tests/rx11b_stage_model.py (pinned to the
whole-capture model and the oracle by tests/test_11b_stage_model_cpu.py): every stage equals its model, output and state, bit for bit; and their composition,
sora_amd.rx11b_by_stages, equals the model's composition and the sora_rx11b_* handle's first row per capture."""
import zlib

import numpy as np
import pytest

import rx11b_stage_model as sm
import stage11b_captures as sc
from test_11b_stage_model_cpu import fields, tied_chips

pytestmark = pytest.mark.gpu

DN = (0, 1, 2, 63, 64, 65, 255, 256, 257, 1000, 3001, 1)                       # units per stream: none, a part of a workgroup's tile, its edges, several workgroups
GUARD16, GUARD8 = 0x5A5A, 0xA5


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


def word(v):
    return (int(v[0]) & 0xFFFF) | ((int(v[1]) & 0xFFFF) << 16)


def ragged(rng, sizes, lead=3):
    """-> (first element of each stream, total): streams of `sizes` elements with gaps of 1 .. 6 elements between them: nothing is aligned"""
    first, at = [], lead
    for s in sizes:
        first.append(at); at += s + int(rng.integers(1, 7))
    return np.asarray(first, np.int64), at + 5


def random_states(rng, n):
    st = np.zeros((n, 4), np.int32)
    st[:, 0] = rng.integers(-2 ** 31, 2 ** 31, n); st[:, 1] = rng.integers(0, 256, n); st[:, 2] = rng.integers(0, 2, n); st[-1, 2] = 1; st[:, 3] = 0x1234
    return st


# ------------------------------------------------------------------ the position-parallel stages
# kind -> (input elements per unit, output elements per unit, input is bytes, output is bytes)
SHAPES = {"dc_remove": (4, 4, False, False), "despread": (11, 1, False, False), "dbpsk": (8, 1, False, True), "dqpsk": (4, 1, False, True),
          "cck5p5": (16, 1, False, True), "cck11": (8, 1, False, True), "desc741": (1, 1, True, True)}


def model_stage(kind, x, state, dc):
    """-> (output of one stream, state after)"""
    if kind == "dc_remove":
        return sm.dc_remove(x, dc), state
    if kind == "despread":
        return sm.despread(x), state
    return sm.stream_stage(kind, x, state)


def gpu_stage(env, kind, d_x, first, n, out_first, state, dc, d_out):
    """one call over the batch -> state after (numpy)"""
    torch, sora = env
    t = lambda a: i32(torch, a)
    if kind == "dc_remove":
        sora.dc_remove11b(d_x, t(first), t(n), t(out_first), dev(torch, dc.astype(np.uint32).view(np.int16).reshape(-1, 2)), d_out, max_n=max(DN))
        return state
    if kind == "despread":
        sora.despread11b(d_x, t(first), t(n), t(out_first), d_out, max_n=max(DN))
        return state
    d_st = dev(torch, state)
    fn = {"dbpsk": sora.dbpsk_demap11b, "dqpsk": sora.dqpsk_demap11b, "cck5p5": sora.cck5p5_decode11b, "cck11": sora.cck11_decode11b, "desc741": sora.desc741_11b}[kind]
    fn(d_x, t(first), t(n), t(out_first), d_st, d_out, max_n=max(DN))
    return d_st.cpu().numpy()


def check_stream_stage(env, kind, rng, tied=False):
    torch, sora = env
    per_in, per_out, in_bytes, out_bytes = SHAPES[kind]
    n = np.asarray(DN, np.int64)
    first, total = ragged(rng, n * per_in); out_first, out_total = ragged(rng, n * per_out, lead=5)
    if in_bytes:
        x = rng.integers(0, 256, total).astype(np.uint8)
    else:
        x = rng.integers(-32768, 32768, (total, 2)).astype(np.int16)              # full range: every wrap is hit
        if tied:
            for f, k in zip(first, n):
                x[f:f + 8 * k * (per_in // 8)] = tied_chips(rng, int(k) * (per_in // 8))
    state0 = random_states(rng, len(n))
    dc = rng.integers(0, 2 ** 32, len(n)).astype(np.uint32)
    blank = np.full(out_total, GUARD8, np.uint8) if out_bytes else np.full((out_total, 2), GUARD16, np.uint16).view(np.int16)
    want = blank.copy(); want_state = state0.copy()
    for f in range(len(n)):
        o, want_state[f] = model_stage(kind, x[first[f]:first[f] + n[f] * per_in], state0[f], dc[f])
        want[out_first[f]:out_first[f] + n[f] * per_out] = o
    d_x = dev(torch, x)
    d_out = dev(torch, blank)
    got_state = gpu_stage(env, kind, d_x, first, n, out_first, state0, dc, d_out)
    got = d_out.cpu().numpy()
    assert np.array_equal(got, want), (kind, np.flatnonzero((got != want).reshape(len(got), -1).any(axis=1))[:8])    # (guards included: nothing between the streams is written)
    assert np.array_equal(got_state, want_state), kind
    assert not np.array_equal(want, blank)
    # the same streams cut into two calls at an odd unit, the state handed over
    n1 = np.where(n > 1, (n // 2) | 1, 0); n1 = np.minimum(n1, n)
    d_out2 = dev(torch, blank)
    mid = gpu_stage(env, kind, d_x, first, n1, out_first, state0, dc, d_out2)
    end = gpu_stage(env, kind, d_x, first + n1 * per_in, n - n1, out_first + n1 * per_out, mid, dc, d_out2)
    assert np.array_equal(d_out2.cpu().numpy(), want) and np.array_equal(end, want_state), kind


@pytest.mark.parametrize("kind", ["dc_remove", "despread", "dbpsk", "dqpsk", "cck5p5", "cck11", "desc741"])
def test_stream_stage_equals_the_model(env, kind):
    check_stream_stage(env, kind, np.random.default_rng([1914, len(kind), SHAPES[kind][0]]))


@pytest.mark.parametrize("kind", ["cck5p5", "cck11"])
def test_cck_decoders_where_metrics_tie(env, kind):
    check_stream_stage(env, kind, np.random.default_rng([1915, SHAPES[kind][0]]), tied=True)


# ------------------------------------------------------------------ TSymTiming
@pytest.fixture(scope="module")
def symtiming_case():
    """8 streams of 1 .. 19 000 blocks: the samples behind the switch of seven model captures, and one whose sampling phase drifts both ways"""
    nblocks = (1, 2, 7, 64, 65, 300, 1000, 19000)
    names = [c.name for c in sc.all_captures()]
    src = ["long-1000-1", "long-2000-5", "short-2000-14", "long-5500-33", "short-11000-120", "long-2000-120", "long-1000-120"]
    rng = np.random.default_rng(1916)
    xs = []
    for nb, name in zip(nblocks, src):
        s = sc.streams(names.index(name))["behind"]
        assert len(s) >= 28 * nb, (name, len(s))
        xs.append(s[:28 * nb])
    xs.append(sc.drifting_stream(rng, 19000))
    first, total = ragged(rng, [len(x) for x in xs])
    x = rng.integers(-32768, 32768, (total, 2)).astype(np.int16)
    for f, s in zip(first, xs):
        x[f:f + len(s)] = s
    state0 = np.array([[2, 0]] * 7 + [[3, -2]], np.int32); state0[3] = (0, 3); state0[5] = (1, -3)
    want = [sm.symtiming(s, st, trace=True) for s, st in zip(xs, state0)]
    trace = want[-1][2]
    assert -1 in trace and 4 in trace                                            # m_index leaves [0, 3] in both directions
    assert {len(w[0]) - 7 * nb for w, nb in zip(want, nblocks)} != {0}            # (and blocks of 6 and of 8 chips do not cancel everywhere)
    return np.asarray(nblocks, np.int64), first, x, state0, want


def run_symtiming(env, case, pieces):
    """the streams in `pieces` calls, cut at odd blocks -> (chips per stream, nchips, state after)"""
    torch, sora = env
    n, first, x, state0, want = case
    out_first, out_total = ragged(np.random.default_rng(3), 8 * n, lead=2)
    d_x = dev(torch, x); d_out = dev(torch, np.full((out_total, 2), GUARD16, np.uint16).view(np.int16))
    d_st = dev(torch, state0)
    done = np.zeros(len(n), np.int64); nch = np.zeros(len(n), np.int64)
    for p in range(pieces):
        k = n - done if p == pieces - 1 else np.minimum(n - done, (n // pieces) | 1)
        got = sora.symtiming11b(d_x, i32(torch, first + 28 * done), i32(torch, k), i32(torch, out_first + nch), d_st, d_out, max_n=int(k.max()))
        done += k; nch += got.cpu().numpy().astype(np.int64)
    out = d_out.cpu().numpy()
    chips = [out[o:o + c] for o, c in zip(out_first, nch)]
    guards = np.ones(len(out), bool)
    for o, c in zip(out_first, nch):
        guards[o:o + c] = False
    assert (out[guards].view(np.uint16) == GUARD16).all()                         # nothing behind a stream's chips is written
    return chips, nch, d_st.cpu().numpy()


@pytest.mark.parametrize("pieces", [1, 2])
def test_symtiming_equals_the_model(env, symtiming_case, pieces):
    chips, nch, st = run_symtiming(env, symtiming_case, pieces)
    for f, (wc, ws, _) in enumerate(symtiming_case[4]):
        assert nch[f] == len(wc) and np.array_equal(chips[f], wc), (f, nch[f], len(wc))
        assert list(st[f]) == list(ws), f


# ------------------------------------------------------------------ the three searches: 64 streams per call, some too short to decide, continued in a second call
def search_streams(rng, key, per, short_len, random_len, noise):
    """-> 64 streams: the 44 captures' own stream `key` where the graph got that far, random streams for the rest"""
    xs = []
    for i in range(len(sc.all_captures())):
        s = sc.streams(i).get(key)
        if s is not None and len(s) >= per:
            xs.append(s[:len(s) // per * per])
    assert len(xs) >= 30, (key, len(xs))
    while len(xs) < 64:
        a = noise[len(xs) % len(noise)]
        xs.append(np.clip(np.rint(rng.normal(0, a, (random_len * per, 2))), -32768, 32767).astype(np.int16))
    xs = xs[:64]
    n = np.array([len(s) // per for s in xs], np.int64)
    n[::4] = np.minimum(n[::4], short_len)                                       # every fourth stream: shorter than any decision
    n[1] = 0
    return xs, n


def check_search(env, kind, xs, n, per, state0, model, gpu):
    torch, sora = env
    first, total = ragged(np.random.default_rng(7), [len(s) for s in xs])
    x = np.zeros((total, 2), np.int16)
    for f, s in zip(first, xs):
        x[f:f + len(s)] = s
    d_x = dev(torch, x)
    full = np.array([len(s) // per for s in xs], np.int64)
    want1 = [model(s[:per * k], st) for s, k, st in zip(xs, n, state0)]
    d_st = dev(torch, state0)
    used1 = gpu(d_x, i32(torch, first), i32(torch, n), d_st).cpu().numpy().astype(np.int64)
    st1 = d_st.cpu().numpy()
    for f, (ws, wu) in enumerate(want1):
        assert used1[f] == wu and np.array_equal(st1[f], ws), (kind, f, used1[f], wu)
    undecided = [f for f in range(len(xs)) if used1[f] == n[f] and n[f] < full[f]]
    assert len(undecided) >= 8, (kind, len(undecided))                           # streams that ended before the brick decided: state carried, d_used == d_n
    # the continuation: every stream from where it stopped to its end
    n2 = full - used1
    want2 = [model(s[per * u:], st) for s, u, st in zip(xs, used1, st1)]
    used2 = gpu(d_x, i32(torch, first + per * used1), i32(torch, n2), d_st).cpu().numpy().astype(np.int64)
    st2 = d_st.cpu().numpy()
    whole = [model(s, st) for s, st in zip(xs, state0)]
    for f in range(len(xs)):
        assert used2[f] == want2[f][1] and np.array_equal(st2[f], want2[f][0]), (kind, f)
        if f in undecided:
            assert used1[f] + used2[f] == whole[f][1] and np.array_equal(st2[f], whole[f][0]), (kind, f)   # cut in two = uncut
    return st2


def test_energy_detect_equals_the_model(env):
    torch, sora = env
    rng = np.random.default_rng(1917)
    xs, n = search_streams(rng, "front", 4, 9, 130, noise=(3.0, 400.0, 1200.0, 9000.0))
    st = sora.state11b_reset("energy", 64)
    for f in range(44, 64):                                                      # the random streams start mid-way: a running window, a DC sum under way
        st[f, 1:9] = rng.integers(0, 50000, 8); st[f, 0] = st[f, 1:9].sum(); st[f, 9] = rng.integers(0, 8); st[f, 10] = rng.integers(0, 40)
        st[f, 14] = rng.integers(0, 9); st[f, 15] = rng.integers(-2 ** 31, 2 ** 31); st[f, 16] = rng.integers(-2 ** 31, 2 ** 31)
    end = check_search(env, "energy", xs, n, 4, st, sm.energy_detect, lambda x, a, k, s: sora.energy_detect11b(x, a, k, s, max_n=4096))
    assert (end[:, 11] == 1).sum() >= 30 and (end[:, 12] == 0x80000007 - 2 ** 32).sum() >= 4     # power detected, and carrier-sense time-outs


def test_barker_sync_equals_the_model(env):
    torch, sora = env
    rng = np.random.default_rng(1918)
    xs, n = search_streams(rng, "chips", 1, 7, 60, noise=(500.0, 3000.0))
    xs = [s[:200] for s in xs]; n = np.minimum(n, 200)
    end = check_search(env, "barker", xs, n, 1, sora.state11b_reset("barker", 64), sm.barker_sync, lambda x, a, k, s: sora.barker_sync11b(x, a, k, s, max_n=200))
    assert (end[:, 0] == 4).sum() >= 30 and (end[:, 14] == 0x80000009 - 2 ** 32).sum() >= 3        # synced, and time-outs


@pytest.mark.parametrize("mode", [0, 1])
def test_sfd_sync_equals_the_model(env, mode):
    torch, sora = env
    rng = np.random.default_rng(1919)
    xs = []
    for i in range(len(sc.all_captures())):
        s = sc.streams(i, mode).get("sfd_symbols")
        if s is not None and len(s):
            xs.append(s)
    assert len(xs) >= 30
    while len(xs) < 64:
        xs.append(np.clip(np.rint(rng.normal(0, 2000.0, (170, 2))), -32768, 32767).astype(np.int16))
    xs = xs[:64]
    n = np.array([len(s) for s in xs], np.int64); n[::4] = np.minimum(n[::4], 21); n[1] = 0
    st = sora.state11b_reset("sfd", 64)
    st[40:, 0] = rng.integers(-2 ** 31, 2 ** 31, 24); st[40:, 1] = rng.integers(0, 256, 24)       # the context the brick finds: any last_symbol, any byte_reg
    end = check_search(env, "sfd", xs, n, 1, st, lambda s, state: sm.sfd_sync(s, state, mode), lambda x, a, k, s: sora.sfd_sync11b(x, a, k, s, mode=mode, max_n=256))
    rates = set(end[:, 7].tolist()); errs = set((end[:, 8].astype(np.int64) & 0xFFFFFFFF).tolist())
    assert 1 in rates and (2 in rates) == (mode == 1) and errs & {0x80000004, 0x80000008}, (rates, errs)


# ------------------------------------------------------------------ the parser and the sink
def crc16(b):
    c = 0xFFFF
    for v in b:
        c ^= v
        for _ in range(8):
            c = (c >> 1) ^ 0x8408 if c & 1 else c >> 1
    return ~c & 0xFFFF


def test_plcp_parse_equals_the_model(env):
    torch, sora = env
    rng = np.random.default_rng(1920)
    hdrs = []
    for signal in (0x0A, 0x14, 0x37, 0x6E, 0x55):                                # the four SIGNAL values and an unknown one
        for service in (0x00, 0x80, 0x08, 0x88, 0x04):                           # both SERVICE length bits
            for ln in (0, 8, 1000, 11999, 65535):
                h = [signal, service, ln & 255, ln >> 8]; c = crc16(h)
                hdrs.append(h + [c & 255, c >> 8])
    hdrs.append(hdrs[3][:4] + [hdrs[3][4] ^ 1, hdrs[3][5]])                      # a wrong CRC
    hdrs.append(hdrs[40][:5] + [hdrs[40][5] ^ 0x80])
    hdrs += rng.integers(0, 256, (64, 6)).tolist()                               # 64 random headers
    h = np.asarray(hdrs, np.uint8)
    want = np.stack([sm.plcp_parse(r) for r in h])
    got = sora.plcp_parse11b(dev(torch, h)).cpu().numpy()
    assert np.array_equal(got, want)
    assert set(want[:, 1].tolist()) == {0, 1000, 2000, 5500, 11000} and (want[:, 0] != 0).sum() >= 60 and (want[:125, 0] == 0).all()


def test_frame_sink_equals_the_model(env):
    torch, sora = env
    rng = np.random.default_rng(1921)
    lens, frames = [], []
    for ln in (0, 3, 4, 5, 6, 64, 1504, 4095):
        for good in (True, False):
            body = rng.integers(0, 256, max(ln - 4, 0)).astype(np.uint8).tobytes()
            fr = bytearray(body + zlib.crc32(body).to_bytes(4, "little"))[:max(ln, 4)]
            if not good:
                fr[int(rng.integers(0, max(ln - 1, 1)))] ^= 0x10
            lens.append(ln); frames.append(bytes(fr[:max(ln - 1, 0)]))           # the sink never reads byte frame_length - 1: it is not even there
    first, total = ragged(rng, [len(f) for f in frames])
    x = rng.integers(0, 256, total).astype(np.uint8)
    for a, f in zip(first, frames):
        x[a:a + len(f)] = np.frombuffer(f, np.uint8)
    want = np.stack([sm.frame_sink(x[a:a + max(ln - 1, 0)], ln) for a, ln in zip(first, lens)])
    got = sora.frame_sink11b(dev(torch, x), i32(torch, first), i32(torch, lens)).cpu().numpy()
    assert np.array_equal(got, want)
    codes = (want[:, 0].astype(np.int64) & 0xFFFFFFFF).tolist()
    assert codes[:4] == [0, 0, 0, 0] and codes[4::2] == [1] * 6 and codes[5::2] == [0x80000006] * 6
    assert (want[:, 1].astype(np.int64) >> 24 == 0).all()


# ------------------------------------------------------------------ the composition
@pytest.fixture(scope="module")
def batch():
    iq, descs = sc.batch()
    return iq, descs


@pytest.mark.parametrize("mode", [0, 1])
def test_by_stages_equals_the_model_and_the_handle(env, batch, mode):
    torch, sora = env
    iq, descs = batch
    d_iq = dev(torch, iq)
    got = sora.rx11b_by_stages(d_iq, descs, mode)
    want = sm.first_events(iq, descs, mode)
    assert [fields(e) for e in got] == [fields(e) for e in want]
    assert sum(e is not None and e["error_code"] == 1 for e in got) == (35 if mode else 20)
    # the handle's first row per capture
    rx = sora.Rx11b(len(descs), len(iq), max_frames_per_capture=8)
    rx.set_preamble(mode)
    rx.process_dev(d_iq, [(o, n, i) for i, (o, n) in enumerate(descs)])
    rows = rx.results(); rx.close()
    firsts = {}
    for r in rows:
        firsts.setdefault(r["capture_id"], r)
    for i, e in enumerate(got):
        r = firsts.get(i)
        assert (e is None) == (r is None), i
        if e is None:
            continue
        assert (e["error_code"], e["rate_kbps"], e["length"], e["flags"], e["crc32"] & 0xFFFFFF) == \
               (r["error_code"], r["rate_kbps"], r["length"], r["flags"], r["crc32"] & 0xFFFFFF), i
        if e["error_code"] in (0x1, 0x80000006):
            assert e["mpdu"][:e["length"] - 1] == r["mpdu"][:r["length"] - 1], i
