"""The integer model of the 40 MHz HT front end (tests/cxx/ht40_front_model.c, tests/ht40_front_model.py) held to what it must not be an echo of: with its three
own definitions switched off it is the reference-pinned 802.11n receiver (Oracle.rx11n_capture), its SIG field extraction is so_sig_decode11n's wherever that
accepts, and on py_ht40's frames it finds what the generator sent -- position, MCS, LENGTH, symbol count, carrier offset, and the noise scale DESIGN.md states.
Then a census: the capture set of tests/test_gpu_ht40_front.py reaches every branch the front end has, counted on the model alone.  No GPU."""
import functools

import numpy as np
import pytest

from oracle import py_ht40 as m
import ht40_front_captures as fc
import ht40_front_model as fm
import level_captures as lc

E_PLCP = 0x80000005
TOTAL = {}                                              # counters over every SIG field any test here walked


def front(iq0, iq1, flags=fm.OWN):
    cn = {}
    ev = fm.front(iq0, iq1, flags=flags, counters=cn)
    for k, v in cn.items():
        TOTAL[k] = TOTAL.get(k, 0) + v
    return ev, cn


def ref_key(rows):
    return [(r["end_sample"], r["error_code"]) + ((r["rate_kbps"], r["length"]) if r["error_code"] != E_PLCP else (0, 0)) for r in rows]


def own_key(ev):
    return [(e["end_sample"], e["error_code"], e["mcs"], e["ht_len"]) for e in ev]


def ht40_capture(rng, mcs, length, sigma, cfo_step=0.0, lead=400, H=fc.H_MIX):
    x, nsym, ps = fc.frame(rng, mcs, length)
    pair = fc.each(lc.whole, fc.gauss(fc.cat(fc.quiet(lead), fc.through(x, H, cfo_step), fc.quiet(600)), rng, sigma))
    return pair, nsym


# ------------------------------------------------------------------ against the reference-pinned receiver
def test_with_its_own_definitions_off_the_model_is_the_reference_pinned_receiver(oracle):
    """end_sample, error code, MCS and length of every event, on the 802.11n set of tests/level_captures.py (overdriven, DC, near-silent, rails, the stream) and on
    py_ht40 frames as the 20 MHz front end sees them (front_end_view)"""
    caps = [(c.name, c.iq) for c in lc.chain_11n()]
    rng = np.random.default_rng(40)
    for mcs in range(8, 15):
        for sigma in (0.0, 8.0):
            pair, _ = ht40_capture(rng, mcs, 40 + 11 * mcs, sigma, cfo_step=(-21.0, 30.5)[mcs % 2])
            caps.append(("front_end_view mcs%d sigma %g" % (mcs, sigma), fc.each(m.front_end_view, pair)))
            # ... and the sign flip is front_end_view's: the model with that one definition on, on the raw capture
            assert own_key(front(*pair, flags=fm.OWN_SIGN)[0]) == own_key(front(*caps[-1][1], flags=0)[0]), caps[-1][0]
    events = 0
    for name, iq in caps:
        got = own_key(front(iq[0], iq[1], flags=0)[0])
        assert got == ref_key(oracle.rx11n_capture(iq[0], iq[1], max_frames=lc.MAX_EVENTS["11n"])), name
        events += len(got)
    assert len(caps) > 270 and events > 400


def test_the_sig_fields_are_the_reference_parsers_wherever_it_accepts(oracle):
    """L-SIG rate, parity and length, HT-SIG MCS, LENGTH and CRC-8 of every SIG field met -- the 802.11n level set under the reference's gate and the whole GPU
    case set under the library's -- against so_sig_decode11n: no disagreement.  And the reference accepts headers that say CBW 40: T11nSigParser never looks at
    that bit (DESIGN.md section 7 g1 said it answers "unsupported"; the difference in the gate is MCS 8..14 and LENGTH <= 4000, and CBW 40 is REQUIRED here)."""
    n = {"sig_fields": 0, "disagreements": 0, "ref_accepts_cbw40": 0}
    for cn in [front(c.iq[0], c.iq[1], flags=0)[1] for c in lc.chain_11n()] + census_set()[2]:
        for k in n:
            n[k] += cn[k]
    assert n["sig_fields"] > 400 and n["disagreements"] == 0 and n["ref_accepts_cbw40"] >= 10, n


# ------------------------------------------------------------------ against the generator
@pytest.mark.parametrize("sigma", [0.0, 20.0])
def test_on_py_ht40_frames_the_model_finds_what_was_sent(sigma):
    """Every MCS 8..14 through a unit channel, clean and at sigma = 20.
    a20: the receiver's symbol timing must fall inside the cyclic prefix in front of where tx_frame put the HT-STF (16 samples at 20 MHz), or its FFT windows
    would reach into the next symbol: htstf / 2 - 16 <= a20 <= htstf / 2.
    cfo: -2 cfo_step (cfo_step is per 40 MHz sample and the channel's sign is the opposite of the correction's).  Tolerance: one step for the estimator's own
    quantisation (the arctangent table, the >> 6), plus at sigma > 0 five standard deviations of the phase of a sum of 128 products under white noise,
    sqrt(2 sigma^2 / (128 P)) / 64 radians per sample, P the L-LTF's mean power per sample.
    noise: S / 416 within +-35 % of 2 sigma^2 / 128 (416 real degrees of freedom: five standard deviations of sqrt(2 / 416))."""
    rng = np.random.default_rng(2020)
    for mcs in range(8, 15):
        cfo_step = (-21.0, 30.5, 0.0)[mcs % 3]; length = 30 + 17 * (mcs - 8)
        pair, nsym = ht40_capture(rng, mcs, length, sigma, cfo_step, lead=400 + 4 * mcs, H=fc.H_UNIT)
        ev, _ = front(*pair)
        tag = (mcs, sigma, ev)
        assert len(ev) == 1 and ev[0]["error_code"] == 0, tag
        e = ev[0]
        true20 = (400 + 4 * mcs + fc.PRE - 160) // 2
        assert (e["mcs"], e["ht_len"], e["nsym"]) == (mcs, length, nsym) and nsym == m.nsym_for([length, length], *m.MCS2[mcs]), tag
        assert true20 - 16 <= e["a20"] <= true20, tag
        assert e["end_sample"] == -(-2 * (e["a20"] + 240 + 80 * nsym) // 28) * 28, tag         # the source call that holds the frame's last sample
        ltf = pair[0][400 + 4 * mcs + 320 + 64:400 + 4 * mcs + 640:2].astype(float)
        P = float(np.mean(ltf[:, 0] ** 2 + ltf[:, 1] ** 2))
        tol = 1.0 + 5.0 * np.sqrt(2 * sigma * sigma / (128.0 * P)) / 64.0 * 65536.0 / (2 * np.pi)
        assert abs(e["cfo"] + 2 * cfo_step) <= tol, (tag, tol)
        if sigma:
            implied = 2 * sigma * sigma / 128.0
            assert 0.65 * implied <= fm.noise_var_of(e["S"]) <= 1.35 * implied, (tag, fm.noise_var_of(e["S"]), implied)
        else:
            # no noise: what is left is the fixed-point FFT's rounding and the CFO estimate's quantisation (one step off turns the second L-LTF symbol by
            # 64 * 2 pi / 65536 against the first: about 1.3 at this amplitude).  It must stay inside the band the sigma = 20 check allows around its value
            assert fm.noise_var_of(e["S"]) < 0.35 * (2 * 20.0 * 20.0 / 128.0), tag


def test_the_case_sets_frames_are_tx_frames_waveform():
    """tests/ht40_front_captures.py restates tx_frame's preamble so that the SIG fields can lie; with honest fields it is tx_frame's, sample for sample"""
    for mcs, length in ((8, 33), (13, 200)):
        ps = [m.add_fcs(bytes(length - 4))] * 2
        x, nsym, pre = m.tx_frame(ps, mcs)
        assert pre == fc.PRE and np.array_equal(x[0, :pre], fc.preamble(mcs, length, nsym)) and np.array_equal(x[1, :pre], x[0, :pre])


def test_the_plans_translation_of_a_record():
    """k_ht40_plan, stated: offset = capture offset + 2 a20 + 160, cfo halved toward zero, noise_var unchanged, n_bpsc / code_rate from the MCS, lengths (len, len)
    or, in joint coding, (len, 0)"""
    assert [fm.trunc_half(c) for c in (-5, -4, -3, -2, -1, 0, 1, 2, 3)] == [-2, -2, -1, -1, 0, 0, 0, 1, 1]
    assert [fm.trunc_half(c) for c in (-3, -1)] != [c >> 1 for c in (-3, -1)]
    rec = {"a20": 748, "mcs": 13, "ht_len": 77, "nsym": 2, "cfo": -41, "end_sample": 2296, "error_code": 0}
    assert fm.descriptor(1004, rec, 6.5, False, 9) == (1004 + 1496 + 160, 6, 1, 77, 77, -20, 6.5, 9)
    assert fm.descriptor(1004, dict(rec, mcs=10, cfo=41), 0.0, True, 9) == (2660, 2, 2, 77, 0, 20, 0.0, 9)
    assert {k: fm.MCS2[k] for k in fm.MCS2} == m.MCS2


# ------------------------------------------------------------------ the census of the GPU case set
@functools.lru_cache(maxsize=None)
def census_set():
    caps = fc.build(False)
    out = [front(c.iq[0], c.iq[1]) for c in caps]
    return caps, [o[0] for o in out], [o[1] for o in out]


def test_census_the_gpu_case_set_reaches_every_branch():
    caps, events, counters = census_set()
    tagged = lambda t: [(c, ev, cn) for c, ev, cn in zip(caps, events, counters) if t in c.tags]
    count = {}
    # a recorded frame of every MCS
    for mcs in range(8, 15):
        count["mcs%d" % mcs] = sum(any(e["error_code"] == 0 and e["mcs"] == mcs for e in ev) for c, ev, cn in tagged("mcs%d" % mcs))
    # a header failure from each cause: L-SIG parity, HT-SIG CRC-8, MCS 7, MCS 15, CBW 20, LENGTH 3, LENGTH 4001
    for cause in ("lsig_parity", "ht_crc", "mcs_low", "mcs_high", "cbw20", "len_short", "len_long"):
        count[cause] = sum(cn[cause] == 1 and [e["error_code"] for e in ev] == [E_PLCP] for c, ev, cn in tagged(cause))
    # ... and T11nSigParser's own L-SIG bound, which the gate leaves standing: 2 x the L-SIG LENGTH field <= 1500, so 750 passes and 751 does not
    count["lsig_length"] = sum(cn["lsig_length"] == 1 and [e["error_code"] for e in ev] == [E_PLCP] for c, ev, cn in tagged("lsig_length"))
    count["lsig_750"] = sum([e["error_code"] for e in ev] == [0] for c, ev, cn in tagged("lsig_750"))
    # a capture that ends behind 0, 1 and 2 SIG symbols: the flush cases
    for k in range(3):
        count["flush%d" % k] = sum(cn["flush%d" % k] == 1 for c, ev, cn in tagged("flush%d" % k))
    # ... the last case behind a whole frame with the same header: zero-filled, the second header fails; read from what the first left, it would pass
    count["flush2_behind_a_frame"] = sum(cn["flush2"] == 1 and [e["error_code"] for e in ev] == [0, E_PLCP] for c, ev, cn in tagged("flush2_behind_a_frame"))
    # a frame whose last data sample is the capture's last (recorded), and the same capture 28 samples shorter (no event)
    (ce, eve, _), = tagged("exact"); (cs, evs, cns), = tagged("short28")
    count["exact"] = int(len(eve) == 1 and eve[0]["error_code"] == 0 and 2 * (eve[0]["a20"] + 240 + 80 * eve[0]["nsym"]) == len(ce.iq[0]) == eve[0]["end_sample"])
    count["short28"] = int(evs == [] and cns["cut_frames"] == 1 and len(cs.iq[0]) == len(ce.iq[0]) - 28 and np.array_equal(cs.iq[0], ce.iq[0][:-28]))
    count["cut"] = sum(ev == [] and cn["cut_frames"] == 1 for c, ev, cn in tagged("cut"))
    # a carrier-sense time-out
    count["timeout"] = sum(cn["timeouts"] > 0 for cn in counters)
    # a detection that fires early at a 4 - 6 LSB floor: the frame's own first samples are taken for the end of a plateau, and the frame is lost
    count["early"] = sum(bool(ev) and ev[0]["a20"] < c.sent[0]["htstf"] // 2 - 16 for c, ev, cn in tagged("floor46"))
    count["on_time"] = sum(bool(ev) and ev[0]["error_code"] == 0 and ev[0]["a20"] >= c.sent[0]["htstf"] // 2 - 16 for c, ev, cn in tagged("floor46"))
    # a negative odd CFO estimate of a recorded frame (cfo / 2 and cfo >> 1 differ)
    count["negative_odd_cfo"] = sum(any(e["error_code"] == 0 and e["cfo"] < 0 and e["cfo"] % 2 for e in ev) for ev in events)
    # a sample of -32768 under the derotation's negate (kept sample m odd), inside the L-LTF an event's CFO and S are computed from
    def negated_rail(c, ev):
        for e in ev:
            mm = np.arange(e["a20"] - 368, e["a20"] - 240); mm = mm[mm % 2 == 1]
            if any(np.any(x[2 * mm] == -32768) for x in c.iq):
                return True
        return False
    count["negated_rail"] = sum(negated_rail(c, ev) for c, ev, cn in tagged("neg_rail"))
    # a capture with more events than row slots
    count["slots"] = sum(len(ev) > fc.MAX_EVENTS for c, ev, cn in tagged("slots"))
    count["several"] = sum(len(ev) == 3 for c, ev, cn in tagged("several"))
    assert all(v >= 1 for v in count.values()), count
    # every family is there, frames carry 4 - 200 bytes but the one at LENGTH 4000 and MCS 14, and the offsets are multiples of 4 but not of 8 or 28
    assert {c.family for c in caps} == {"plain", "overdriven", "rails", "dc", "silent", "floor", "cfo", "gate", "cut", "several"}
    lengths = sorted(s["length"] for c in caps for s in c.sent if s["sound"])
    assert lengths[0] == 4 and lengths[-1] == 4000 and lengths[-2] <= 200
    assert any(e["mcs"] == 14 and e["ht_len"] == 4000 and e["error_code"] == 0 for ev in events for e in ev)
    _, descs = fc.layout(caps)
    assert all(d[0] % 4 == 0 and d[0] % 8 and d[0] % 28 for d in descs)
    # the levels: a clipped capture, events found at a peak below 32 LSB and captures that peak at a few LSB, S beyond single precision's 24 bits and S = 0
    peak = lambda c: int(np.abs(c.iq[0].astype(int)).max())
    assert any(peak(c) >= 32767 and ev for c, ev in zip(caps, events) if c.family == "overdriven")
    assert any(peak(c) < 32 and ev for c, ev in zip(caps, events) if c.family == "silent") and any(peak(c) <= 8 for c in caps if c.family == "silent")
    assert any(e["S"] > 1 << 24 for ev in events for e in ev) and any(e["S"] == 0 for ev in events for e in ev)


def test_the_joint_case_set_reaches_its_cut_offs_too():
    """the cuts of the joint set follow the joint symbol count"""
    caps = fc.build(True)
    for tag, want in (("exact", 1), ("short28", 0), ("slots", fc.MAX_EVENTS + 2)):
        (c,) = [c for c in caps if tag in c.tags]
        ev, _ = front(c.iq[0], c.iq[1], flags=fm.OWN | fm.JOINT)
        assert len(ev) == want, (tag, ev)
        assert all(e["nsym"] == -(-(22 + 8 * e["ht_len"]) // (2 * m.ndbps(*m.MCS2[e["mcs"]]))) for e in ev if e["error_code"] == 0)
