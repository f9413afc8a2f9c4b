"""GPU parity of the 802.11a receive graph's front-end stages (sora_amd/csrc/k_11a.hip: sora_hip_dc_remove11a, _dc_estimate11a, _cca11a, _carrier_sense11a,
_data_symbol11a, _viterbi_sig11a, _plcp_parse11a) against the per-brick model of tests/rx11a_stage_model.py (pinned to the oracle by
tests/test_11a_stage_model_cpu.py): output, record, d_used and d_npass bit for bit, over ragged, unaligned stream tables with guards around every output; the same
stream cut into two calls; and the carrier-sense record, mapped, against the receive handle's own continuation record at every prefix of the composite stream."""
import numpy as np
import pytest

import rx11a_stage_cases as cases
import rx11a_stage_model as model
import scan_captures as sc
from gpu_util import batch
from sora_amd import capi

pytestmark = pytest.mark.gpu

GUARD16, GUARD32 = 0x5A5A, 0x5A5AA5A5
STOP = capi.CCA11A_STOP_ON_TIMEOUT


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


def ragged(rng, sizes, lead=3, unit=1):
    """-> (first element of each stream, total): gaps of 1 .. 6 units between the streams: nothing is aligned, odd offsets included"""
    first, at = [], lead
    for s in sizes:
        first.append(at); at += int(s) + unit * int(rng.integers(1, 7))
    return np.asarray(first, np.int64), at + 5


def lay_out(rng, xs):
    first, total = ragged(rng, [len(x) for x in xs])
    buf = rng.integers(-32768, 32768, (total, 2)).astype(np.int16)
    for f, x in zip(first, xs):
        buf[f:f + len(x)] = x
    assert (first % 2 == 1).any()
    return buf, first


# ------------------------------------------------------------------ TCCA11a, and the loop TDCRemoveEx -> TCCA11a -> TDCEstimator
def gpu_sense(env, rng, xs, states, flags, fused, n=None, max_n=None):
    """one call over the batch -> (states after, used[, npass, the gated bursts per stream])"""
    torch, sora = env
    ns = len(xs); words = capi.CS11A_WORDS if fused else capi.CCA11A_WORDS
    n = np.array([len(x) // 4 for x in xs], np.int64) if n is None else np.asarray(n, np.int64)
    max_n = int(n.max()) if max_n is None else int(max_n)
    buf, first = lay_out(rng, xs)
    st = np.full((ns + 2, words), GUARD32, np.int32); st[1:-1] = np.asarray(states)[:, :words]
    d_st = dev(torch, st); d_used = dev(torch, np.full(ns + 2, GUARD32, np.int32))
    d_x, d_first, d_n = dev(torch, buf), i32(torch, first), i32(torch, n)
    L = sora.load()
    if fused:
        rc = L.sora_hip_carrier_sense11a(d_x.data_ptr(), d_first.data_ptr(), d_n.data_ptr(), d_st[1:].data_ptr(), d_used[1:].data_ptr(), ns, max_n, int(flags), None)
    else:
        ofirst, ototal = ragged(rng, np.minimum(n, max_n), lead=1)
        d_out = dev(torch, np.full((4 * ototal, 2), GUARD16, np.int16)); d_np = dev(torch, np.full(ns + 2, GUARD32, np.int32)); d_of = i32(torch, ofirst)
        rc = L.sora_hip_cca11a(d_x.data_ptr(), d_first.data_ptr(), d_n.data_ptr(), d_of.data_ptr(), d_st[1:].data_ptr(), d_out.data_ptr(), d_used[1:].data_ptr(),
                               d_np[1:].data_ptr(), ns, max_n, int(flags), None)
    assert rc == 0, L.sora_hip_last_error()
    torch.cuda.synchronize()
    st = d_st.cpu().numpy(); used = d_used.cpu().numpy()
    assert (st[0] == GUARD32).all() and (st[-1] == GUARD32).all() and used[0] == GUARD32 and used[-1] == GUARD32
    if fused:
        return st[1:-1], used[1:-1]
    npass = d_np.cpu().numpy(); out = d_out.cpu().numpy()
    assert npass[0] == GUARD32 and npass[-1] == GUARD32
    gated = []; touched = np.zeros(len(out), bool)
    for f in range(ns):
        a = 4 * int(ofirst[f]); b = a + 4 * int(npass[1 + f])
        gated.append(out[a:b].copy()); touched[a:b] = True
    assert (out[~touched].view(np.uint16) == GUARD16).all()                       # nothing written outside what d_npass announces
    return st[1:-1], used[1:-1], npass[1:-1], gated


def model_sense(xs, states, flags, fused, n=None, max_n=None):
    out = []
    for f, x in enumerate(xs):
        k = len(x) // 4 if n is None else int(n[f])
        k = k if max_n is None else min(k, int(max_n))
        out.append(model.carrier_sense(x[:4 * k], states[f], flags) if fused else model.cca(x[:4 * k], states[f][:capi.CCA11A_WORDS], flags))
    return out


def same_sense(got, want, fused, what):
    ws = np.stack([w[0] for w in want]); wu = np.array([w[1] for w in want], np.int32)
    gs, gu = got[0], got[1]
    assert np.array_equal(gu, wu), (what, np.flatnonzero(gu != wu)[:8], gu[gu != wu][:8], wu[gu != wu][:8])
    bad = np.flatnonzero((gs != ws).any(axis=1))
    assert len(bad) == 0, (what, bad[:8], [np.flatnonzero(gs[b] != ws[b])[:6].tolist() for b in bad[:4]])
    if not fused:
        assert np.array_equal(got[2], np.array([len(w[2]) // 4 for w in want], np.int32)), what
        for f, w in enumerate(want):
            assert np.array_equal(got[3][f], w[2]), (what, f)


@pytest.fixture(scope="module")
def streams(oracle):
    s = cases.sense_streams(oracle, model)
    assert 256 <= len(s) + 1 <= 512 and max(len(x) for x, _ in s) <= 4 * 2048
    return s


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("flags", [0, STOP])
def test_sense_equals_the_model(env, streams, flags, fused):
    """every stream under this flag, plus a stream of 0 bursts; then max_n below most streams' d_n"""
    rng = np.random.default_rng(41 + flags + 2 * fused)
    xs = [x for x, _ in streams] + [np.zeros((0, 2), np.int16)]
    states = [s for _, s in streams] + [capi.cs11a_states(1)[0]]
    want = model_sense(xs, states, flags, fused)
    same_sense(gpu_sense(env, rng, xs, states, flags, fused), want, fused, "one call")
    ws = np.stack([w[0] for w in want]); wu = np.array([w[1] for w in want])
    assert (ws[:, 0] == 1).sum() >= 20 and wu[-1] == 0 and (ws[:, 5] == 1).sum() >= 1           # detections, the empty stream, a lock held at the end
    assert (ws[:, 1].view(np.uint32) == capi.E_CS_TIMEOUT).sum() >= 20
    if flags:
        assert ((wu < np.array([len(x) // 4 for x in xs])) & (ws[:, 0] == 0)).sum() >= 20          # streams the flag ended
    for max_n in (1, 63, 64, 65, 200):
        want = model_sense(xs, states, flags, fused, max_n=max_n)
        same_sense(gpu_sense(env, rng, xs, states, flags, fused, max_n=max_n), want, fused, "max_n %d" % max_n)


@pytest.mark.parametrize("fused", [True, False])
def test_the_composite_stream_cut_into_two_calls_gives_what_one_call_gives(env, oracle, fused):
    """spans of the composite stream that begin in quiet, on the DC step, in front of each fragment and frame and in the loud noise, each cut at 24 positions spread
    over what the walk consumes: the lead, the plateau, the lock, the burst before the decision"""
    rng = np.random.default_rng(43)
    x = cases.x20(sc.composite_stream(oracle))
    spans = [x[a:a + 4 * 2048] for a in (0, 700, 2100, 3100, 3400, 3650, 3900, 4350, 5900, 6300, 7000)]
    spans = [s[:len(s) // 4 * 4] for s in spans]
    fresh = capi.cs11a_states(len(spans))
    for flags in (0, STOP):
        whole = model_sense(spans, fresh, flags, fused)
        xs, owner, cuts = [], [], []
        for j, (s, w) in enumerate(zip(spans, whole)):
            for c in sorted(set(np.linspace(0, w[1], 24).astype(int).tolist() + [max(w[1] - 1, 0)])):
                xs.append(s); owner.append(j); cuts.append(c)
        assert len(xs) >= 64
        st0 = capi.cs11a_states(len(xs))
        a = gpu_sense(env, rng, xs, st0, flags, fused, n=cuts)
        same_sense(a, model_sense(xs, st0, flags, fused, n=cuts), fused, "first part")
        rest = [s[4 * int(u):] for s, u in zip(xs, a[1])]
        full = np.zeros((len(xs), capi.CS11A_WORDS), np.int32); full[:, :a[0].shape[1]] = a[0]
        b = gpu_sense(env, rng, rest, full, flags, fused)
        continued = 0
        for k, j in enumerate(owner):
            w = whole[j]
            if a[1][k] == w[1] and np.array_equal(a[0][k], w[0]):                 # the first call already ended where one call ends (the decision, or the flag's stop)
                continue
            assert a[1][k] == cuts[k], (flags, k)
            assert a[1][k] + b[1][k] == w[1] and np.array_equal(b[0][k], w[0]), (flags, k, cuts[k], np.flatnonzero(b[0][k] != w[0]))
            continued += 1
        assert continued >= 64


def test_the_mapped_record_equals_the_receive_handles_at_every_prefix_of_the_composite_stream(env, oracle):
    """the GPU's carrier-sense entry walked over the composite stream by the harness's rules, one call per source call; at each prefix's last resume point the record,
    mapped by cs11a_record_words, is words 0-39 of what the stream-mode handle stores for that prefix (sora_rx_stream_record_of)"""
    torch, sora = env
    x = sc.composite_stream(oracle); x2 = cases.x20(x); n20 = len(x2)
    rows = oracle.rx_capture(x, 40, max_frames=8)
    d_x = dev(torch, x2)
    d_first = torch.zeros(1, dtype=torch.int32, device="cuda"); d_n = torch.zeros(1, dtype=torch.int32, device="cuda")

    def step(p, m, st, flags):
        d_first.fill_(p); d_n.fill_(m)
        d_st = dev(torch, st.reshape(1, -1))
        used = capi.carrier_sense11a(d_x, d_first, d_n, d_st, flags, max_n=m)
        return d_st.cpu().numpy()[0], int(used.cpu().numpy()[0])

    det, pts = model.sense_walk_by(step, n20, rows)
    assert det == [r["start_sample"] for r in rows] and len(det) >= 4
    pos = np.array([p for p, _ in pts])
    K = len(x) // 56
    iq, descs = batch([x[:56 * k] for k in range(1, K + 1)])
    rx = sora.Rx(K, len(iq), sample_rate_mhz=40, max_frames_per_capture=8)
    assert rx.set_stream_mode(1) == 0
    t = rx.process_dev(torch.from_numpy(iq).cuda(), descs)
    used = rx.stream_consumed(t, K)
    seen = set()
    for k in range(1, K + 1):
        i = int(np.searchsorted(pos, 28 * k, side="right")) - 1
        assert i >= 0 and int(used[k - 1]) == 2 * pos[i], k
        got = rx.stream_record_of(t, k - 1)
        mine = capi.cs11a_record_words(pts[i][1])
        assert np.array_equal(got[:40], mine), (k, pos[i], np.flatnonzero(got[:40] != mine))
        seen.add(i)
    rx.close()
    assert len(seen) >= 200


# ------------------------------------------------------------------ the composition
@pytest.mark.parametrize("rate_mhz", [40, 20])
def test_rx11a_by_stages_equals_the_handle_in_every_row_and_mpdu_byte(env, oracle, rate_mhz):
    """the CPU composition test's captures through sora_amd.rx11a_by_stages and through Rx (default kernels): every event of every capture"""
    torch, sora = env
    caps = cases.composition_captures(oracle, rate_mhz)
    iq, descs = batch(caps)
    iq = np.concatenate([iq, np.zeros(((-len(iq)) % 8, 2), np.int16)])
    d_iq = torch.from_numpy(iq).cuda()
    rx = sora.Rx(len(caps), len(iq), sample_rate_mhz=rate_mhz, max_frames_per_capture=16)
    rows = rx.results(ticket=rx.process_dev(d_iq, descs))
    rx.close()
    got = sora.rx11a_by_stages(d_iq, [(o, n) for o, n, _ in descs], rate_mhz)
    assert len(got) == len(caps)
    total = 0
    for k in range(len(caps)):
        want = [r for r in rows if r["capture_id"] == k]
        why = cases.same_events(got[k], want)
        assert why is None, (rate_mhz, k, why)
        total += len(want)
    assert total >= 60 and {0x1, 0x80000005} <= {r["error_code"] for r in rows}


# ------------------------------------------------------------------ the stateless and the small bricks
@pytest.mark.parametrize("what", ["dc_remove", "data_symbol"])
def test_dc_remove_and_data_symbol_at_1_63_64_65_units_per_stream(env, what):
    torch, sora = env
    rng = np.random.default_rng(47)
    unit_in, unit_out = (4, 4) if what == "dc_remove" else (80, 64)
    n = np.array([1, 63, 64, 65, 0, 130, 64], np.int64); max_n = 65; ne = np.minimum(n, max_n)
    xs = [rng.integers(-32768, 32768, (unit_in * int(k), 2)).astype(np.int16) for k in n]
    buf, first = lay_out(rng, xs)
    L = sora.load()
    d_x, d_first, d_n = dev(torch, buf), i32(torch, first), i32(torch, n)
    if what == "dc_remove":
        dc = rng.integers(-32768, 32768, (len(n), 2)).astype(np.int16); dc[0] = (-32768, 32767)
        ofirst, ototal = ragged(rng, 4 * ne)
        d_out = dev(torch, np.full((ototal, 2), GUARD16, np.int16)); d_of = i32(torch, ofirst); d_dc = dev(torch, dc)
        rc = L.sora_hip_dc_remove11a(d_x.data_ptr(), d_first.data_ptr(), d_n.data_ptr(), d_of.data_ptr(), d_dc.data_ptr(), d_out.data_ptr(), len(n), max_n, None)
        want = [model.dc_remove(x[:4 * int(k)], d) for x, k, d in zip(xs, ne, dc)]
        at = ofirst
    else:
        ofirst, ototal = ragged(rng, ne, lead=1)
        d_out = dev(torch, np.full((64 * ototal, 2), GUARD16, np.int16)); d_of = i32(torch, ofirst)
        rc = L.sora_hip_data_symbol11a(d_x.data_ptr(), d_first.data_ptr(), d_n.data_ptr(), d_of.data_ptr(), d_out.data_ptr(), len(n), max_n, None)
        want = [model.data_symbol(x, int(k)) for x, k in zip(xs, ne)]
        at = 64 * ofirst
    assert rc == 0, L.sora_hip_last_error()
    torch.cuda.synchronize()
    out = d_out.cpu().numpy(); touched = np.zeros(len(out), bool)
    for a, w in zip(at, want):
        assert np.array_equal(out[a:a + len(w)], w)
        touched[a:a + len(w)] = True
    assert (out[~touched].view(np.uint16) == GUARD16).all()


def test_dc_estimate_cut_at_every_phase_of_its_count_of_eight(env):
    torch, sora = env
    rng = np.random.default_rng(53)
    base = rng.integers(-32768, 32768, (4 * 200, 2)).astype(np.int16)
    base[:400] = rng.integers(-600, 600, (400, 2))
    xs, states = [], []
    for cnt in range(9):
        for n in (0, 1, 7, 8, 9, 63, 64, 65, 200):
            s = capi.dcest11a_states(1)[0]; s[0] = cnt; u = s.view(np.uint32); u[1] = model.pack((int(rng.integers(-32768, 32768)), 100)); u[2] = model.pack((-5, 32767))
            xs.append(base[:4 * n]); states.append(s)
    want = np.stack([model.dc_estimate(x, s) for x, s in zip(xs, states)])
    for max_n in (200, 64, 5):
        n = np.array([len(x) // 4 for x in xs], np.int64)
        buf, first = lay_out(rng, xs)
        st = np.full((len(xs) + 2, 4), GUARD32, np.int32); st[1:-1] = np.stack(states)
        d_st = dev(torch, st); d_x, d_first, d_n = dev(torch, buf), i32(torch, first), i32(torch, n)
        L = sora.load()
        assert L.sora_hip_dc_estimate11a(d_x.data_ptr(), d_first.data_ptr(), d_n.data_ptr(), d_st[1:].data_ptr(), len(xs), max_n, None) == 0, L.sora_hip_last_error()
        torch.cuda.synchronize()
        got = d_st.cpu().numpy()
        assert (got[0] == GUARD32).all() and (got[-1] == GUARD32).all()
        w = want if max_n == 200 else np.stack([model.dc_estimate(x[:4 * max_n], s) for x, s in zip(xs, states)])
        assert np.array_equal(got[1:-1, :3], w[:, :3]), (max_n, np.flatnonzero((got[1:-1, :3] != w[:, :3]).any(axis=1))[:8])
        # every cut of the 200-burst stream: the second call continues from the first one's record
    for cut in range(0, 20):
        a = model.dc_estimate(base[:4 * cut], capi.dcest11a_states(1)[0])
        d_st = dev(torch, a.reshape(1, -1)); d_x = dev(torch, base[4 * cut:]); d_first = i32(torch, [0]); d_n = i32(torch, [200 - cut])
        capi.dc_estimate11a(d_x, d_first, d_n, d_st)
        assert np.array_equal(d_st.cpu().numpy()[0, :3], model.dc_estimate(base, capi.dcest11a_states(1)[0])[:3]), cut


def test_viterbi_sig_and_plcp_parse_on_the_cpu_tests_inputs(env, oracle):
    torch, sora = env
    softs = cases.signal_softs(oracle)
    got = capi.viterbi_sig11a(dev(torch, softs)).cpu().numpy().view(np.uint32)
    assert np.array_equal(got, np.array([model.viterbi_sig(s) for s in softs], np.uint32))
    words = cases.signal_words()
    rec = capi.plcp_parse11a(dev(torch, words.view(np.int32))).cpu().numpy().view(np.uint32)
    want = np.stack([model.plcp_parse(w) for w in words])
    assert np.array_equal(rec, want), np.flatnonzero((rec != want).any(axis=1))[:8]
    # the chain: the real SIGNAL symbols' soft values -> word -> record
    rec = capi.plcp_parse11a(capi.viterbi_sig11a(dev(torch, softs[:8]))).cpu().numpy()
    assert list(rec[:, 1]) == list(cases.RATES) and not rec[:, 0].any()
