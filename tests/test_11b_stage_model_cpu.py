"""The 802.11b stage model (tests/cxx/rx11b_stage_model.c: every brick of the receive graph alone) is pinned here: composed again by rx11b_stage_model.first_event --
the walk sora_amd.rx11b_by_stages runs over the GPU's stages -- it reports what tests/rx11b_ext_model.py's whole-capture walk reports first, at mode 0 and mode 1, and at
mode 0 what the oracle reports, over 35 captures that decode and 9 that do not; and two bricks on the corners their captures do not reach.  No GPU."""
import numpy as np
import pytest

import rx11b_ext_model as rxm
import rx11b_stage_model as sm
import stage11b_captures as sc
from oracle.pyoracle import Oracle

E_OK, E_SFD_FAIL, E_PLCP, E_CRC32, E_SFD_TIMEOUT, E_SYNC_TIMEOUT = 0x1, 0x80000004, 0x80000005, 0x80000006, 0x80000008, 0x80000009
FIELDS = ("error_code", "rate_kbps", "length", "crc32", "flags", "mpdu")


def fields(r):
    return None if r is None else tuple(r.get(f, 0) for f in FIELDS)


def first(rows):
    return fields(rows[0]) if rows else None


def test_all_35_decode_in_the_existing_model():
    good, bad = sc.captures()
    assert len(good) == 35 and len(bad) == 9
    for c in good:
        rows = rxm.rx11b(c.iq, 1)
        assert rows and rows[0]["error_code"] == E_OK and rows[0]["mpdu"][:len(c.mpdu)] == c.mpdu and rows[0]["rate_kbps"] == c.rate, c.name
        assert rows[0]["flags"] == (rxm.ROW_SHORT_PREAMBLE if c.preamble else 0), c.name


@pytest.mark.parametrize("mode", [0, 1])
def test_first_event_equals_the_existing_model(mode):
    for c in sc.all_captures():
        assert fields(sm.first_event(c.iq, mode)) == first(rxm.rx11b(c.iq, mode)), (c.name, mode)


def test_first_event_equals_the_oracle_at_mode_0():
    o = Oracle()
    for c in sc.all_captures():
        rows = o.rx11b_capture(c.iq)
        assert fields(sm.first_event(c.iq, 0)) == (first([{**rows[0], "flags": 0}]) if rows else None), c.name


def test_the_batch_form_equals_the_single_form():
    iq, descs = sc.batch()
    assert [fields(e) for e in sm.first_events(iq, descs, 1)] == [fields(sm.first_event(c.iq, 1)) for c in sc.all_captures()]


def test_captures_that_do_not_decode():
    _, bad = sc.captures()
    by = {c.name: c for c in bad}
    for k in range(3):
        assert sm.first_event(by["noise10-%d" % k].iq, 1) is None
        assert sm.first_event(by["noise1500-%d" % k].iq, 1)["error_code"] == E_SYNC_TIMEOUT
    assert sm.first_event(by["header-symbol-negated"].iq, 1)["error_code"] == E_PLCP
    r = sm.first_event(by["payload-symbol-negated"].iq, 1)
    assert r["error_code"] == E_CRC32 and r["rate_kbps"] == 1000 and r["length"] == 37
    assert sm.first_event(by["sync-cut"].iq, 1)["error_code"] in (E_SFD_FAIL, E_SFD_TIMEOUT)


# ------------------------------------------------------------------ TSymTiming on energies that force every branch
def symtiming_restated(x, m_index, m_frag):
    """TSymTiming::Process (symtiming.hpp:42-170) in plain Python -> (chips, m_index, m_frag, trace, the branches taken)"""
    w32 = lambda v: (v + 2 ** 31) % 2 ** 32 - 2 ** 31
    chips, trace, hit = [], [], set()
    for b in range(len(x) // 28):
        blk = x[28 * b:28 * b + 28].astype(np.int64)
        idx = m_index
        while idx < 28:
            if idx < 0:
                chips.append(blk[0]); m_index += 4; hit.add("negative index")
            else:
                chips.append(blk[idx])
            idx += 4
        if m_index >= 4:
            m_index = 0; hit.add("index 4 folded")
        s = [0, 0, 0, 0]
        for i in range(28):
            re, im = int(blk[i][0]) >> 3, int(blk[i][1]) >> 3
            s[i & 3] = w32(s[i & 3] + w32(re * re + im * im))
        mi = m_index; early = 3 if mi == 0 else mi - 1; late = 0 if mi == 3 else mi + 1
        if s[early] < s[late]:
            if s[mi] < s[early]: m_index += 1; m_frag = 0; hit.add("step late")
            elif s[mi] < s[late]: m_frag += 1
        else:
            if s[mi] < s[late]: m_index -= 1; m_frag = 0; hit.add("step early")
            elif s[mi] < s[early]: m_frag -= 1
        if m_frag >= 4: m_index += 1; m_frag = -3; hit.add("frag +4")
        elif m_frag <= -4: m_index -= 1; m_frag = 3; hit.add("frag -4")
        trace.append(m_index)
    return np.array(chips, np.int16).reshape(-1, 2), m_index, m_frag, trace, hit


def phase_blocks(rng, nblocks):
    """blocks whose four sampling phases carry four distinct random levels (and random signs): every ordering of early / on time / late comes up"""
    x = np.zeros((28 * nblocks, 2), np.int16)
    for b in range(nblocks):
        lv = rng.permutation([400, 900, 1700, 3100]) if b % 5 else rng.permutation([900, 900, 1700, 400])
        for i in range(28):
            x[28 * b + i] = (lv[i & 3] * rng.choice([-1, 1]) + rng.integers(-7, 8), rng.integers(-40, 41))
    return x


def test_symtiming_brick_on_every_branch():
    rng = np.random.default_rng(1912)
    x = phase_blocks(rng, 600)
    chips, mi, fr, trace, hit = symtiming_restated(x, 2, 0)
    assert hit == {"negative index", "index 4 folded", "step late", "step early", "frag +4", "frag -4"}
    assert -1 in trace and 4 in trace
    got, st, tr = sm.symtiming(x, [2, 0], trace=True)
    assert np.array_equal(got, chips) and list(st) == [mi, fr] and list(tr) == trace
    # cut at an odd block, the state handed over
    a, sa = sm.symtiming(x[:28 * 301], [2, 0]); b, sb = sm.symtiming(x[28 * 301:], sa)
    assert np.array_equal(np.concatenate([a, b]), chips) and list(sb) == [mi, fr]


# ------------------------------------------------------------------ TCCK11Decoder where metrics tie
def cck11_restated(P, last, even):
    """TCCK11Decoder::CCK11_DECODER (cck.hpp:255-763) on 8 chips in plain Python (complex components as ints, int32 wrap)"""
    w32 = lambda v: (v + 2 ** 31) % 2 ** 32 - 2 ** 31
    rot = lambda a, k: [(a[0], a[1]), (-a[1], a[0]), (-a[0], -a[1]), (a[1], -a[0])][k & 3]
    add = lambda a, b: (w32(a[0] + b[0]), w32(a[1] + b[1]))

    def module(m):
        k = (4 - m) & 3
        A = [add(P[1], rot(P[0], k)), add(rot(P[2], k), rot(P[3], 2)), add(P[5], rot(P[4], k)), add(P[7], rot(P[6], k + 2))]
        M, V = [], []
        for s, base in enumerate((0x00, 0x30, 0x10, 0x20)):
            bx = add(A[1], rot(A[0], s)); by = add(A[3], rot(A[2], s))
            bx = (bx[0] >> 2, bx[1] >> 2); by = (by[0] >> 2, by[1] >> 2)
            lre = w32(w32(bx[0] * by[0]) + w32(bx[1] * by[1])); lim = w32(w32(bx[0] * by[1]) - w32(bx[1] * by[0]))
            a1 = w32(-lre) if lre < 0 else lre; a2 = w32(-lim) if lim < 0 else lim
            if a1 > a2:
                M.append(lre if lre > 0 else w32(-lre)); V.append(base | (0x00 if lre > 0 else 0x40))
            else:
                M.append(lim if lim > 0 else w32(-lim)); V.append(base | (0xC0 if lim > 0 else 0x80))
        mm, vv = (M[0], V[0]) if M[0] > M[1] else (M[1], V[1])
        if M[2] > M[3]:
            if M[2] > mm: mm, vv = M[2], V[2]
        elif M[3] > mm: mm, vv = M[3], V[3]
        return mm, vv

    m1, v1 = module(0); m2, v2 = module(1); v2 |= 0x08
    if m1 > m2:
        m34, v34 = module(3); out = v1 if m1 > m34 else v34 | 0x0C
    else:
        m34, v34 = module(2); out = v2 if m2 > m34 else v34 | 0x04
    re = w32(last[0] * P[7][0] + last[1] * P[7][1]) >> 1; im = w32(last[0] * P[7][1] - last[1] * P[7][0]) >> 1
    out |= (w32(re + im) < 0) | ((w32(re - im) < 0) << 1)
    return out ^ (3 if even else 0)


def tied_chips(rng, n):
    """8 n chips whose phi2 / phi3 metrics tie: all-zero symbols, one chip repeated, (a, a) and (a, -a) chips, sign patterns of one amplitude"""
    x = np.zeros((n, 8, 2), np.int16)
    for k in range(n):
        a = int(rng.integers(1, 32768)) * int(rng.choice([-1, 1]))
        kind = k % 5
        if kind == 1: x[k, :] = (a, 0)
        elif kind == 2: x[k, :] = (a, a)
        elif kind == 3: x[k, :, 0] = a * rng.choice([-1, 1], 8); x[k, :, 1] = a * rng.choice([-1, 1], 8)
        elif kind == 4: x[k, ::2] = (a, -a); x[k, 1::2] = (-a, a)
    return x.reshape(-1, 2)


def test_cck11_brick_where_metrics_tie():
    got, st = sm.stream_stage("cck11", np.zeros((16, 2), np.int16), [0, 0, 0, 0])
    assert list(got) == [0xB4, 0xB7] and list(st) == [0, 0, 0, 0]               # all ties: every strict comparison falls through to the last hypothesis tried
    rng = np.random.default_rng(1913)
    x = tied_chips(rng, 200)
    last, even = (12345, -321), 1
    got, st = sm.stream_stage("cck11", x, [(last[0] & 0xFFFF) | ((last[1] & 0xFFFF) << 16), 0x55, even, 0])
    want = []
    for k in range(200):
        P = [(int(v[0]), int(v[1])) for v in x[8 * k:8 * k + 8]]
        want.append(cck11_restated(P, last, even)); last = P[7]; even ^= 1
    assert list(got) == want
    assert len(set(want)) > 8
