"""The per-brick model of the 802.11a receive graph's front end (tests/rx11a_stage_model.py) pinned to the oracle, without a GPU: the carrier-sense loop against
the restatement's state at every resume point, its detections and its branch counters over the capture families of tests/scan_captures.py at 40 and 20 MHz; the three
split bricks against the loop; T11aViterbiSig and T11aPLCPParser against the oracle's; T11aDataSymbol by definition.  What the GPU stages are then held to is this
model (tests/test_gpu_11a_rx_stages.py)."""
import ctypes

import numpy as np
import pytest

import rx11a_stage_cases as cases
import rx11a_stage_model as model
import scan_captures as sc
from oracle.pyoracle import CS_COUNTERS
from sora_amd import capi

FLOOR = 8
RATE_OF_CODE = {0x8: 48000, 0x9: 24000, 0xA: 12000, 0xB: 6000, 0xC: 54000, 0xD: 36000, 0xE: 18000, 0xF: 9000}      # ieee80211a_cmn.h:97-107
CODE_RATE_OF = {6000: 0, 12000: 0, 24000: 0, 48000: 1, 9000: 2, 18000: 2, 36000: 2, 54000: 2}                       # SORA_CR_12 / _23 / _34


def _captures(oracle, rate_mhz):
    for name, caps in sc.families(oracle).items():
        for c in caps:
            yield name, (c if rate_mhz == 40 else np.ascontiguousarray(c[::2]))


@pytest.mark.parametrize("rate_mhz", [40, 20])
def test_carrier_sense_equals_the_restatement_at_every_resume_point_and_in_every_branch(oracle, rate_mhz):
    """the whole families (3.4 M bursts per rate run in a few seconds); a 20 MHz capture is the even samples of the 40 MHz one, cut to whole 14-sample source calls"""
    got = model.new_counters(); points = 0; detections = 0
    oracle.cs_counters(True)
    try:
        rows_of = []
        for name, c in _captures(oracle, rate_mhz):
            c = c[:len(c) // (28 if rate_mhz == 40 else 14) * (28 if rate_mhz == 40 else 14)]
            rows_of.append((name, c, oracle.rx_capture(c, rate_mhz, max_frames=80)))
        want = oracle.cs_counters_read()
    finally:
        oracle.cs_counters(False)
    for name, c, rows in rows_of:
        det, pos, rec = model.sense_walk(cases.x20(c, rate_mhz), rows, counters=got)
        assert list(det) == [r["start_sample"] for r in rows] or (len(det) == len(rows) + 1 and list(det[:-1]) == [r["start_sample"] for r in rows]), name
        opos, orec = oracle.cs_trace(c, rate_mhz)
        assert np.array_equal(pos, opos), (name, len(pos), len(opos))
        mapped = np.stack([capi.cs11a_record_words(r) for r in rec]) if len(rec) else np.zeros((0, 40), np.uint32)
        assert np.array_equal(mapped, orec[:, :40]), (name, np.argwhere(mapped != orec[:, :40])[:4])
        points += len(pos); detections += len(det)
    got = {k: int(v) for k, v in zip(CS_COUNTERS, got)}
    print("802.11a carrier-sense model at %d MHz: %d resume points, %d detections, branches %s" % (rate_mhz, points, detections, got))
    assert got == want
    assert min(got.values()) >= FLOOR, got
    assert points > 10000 and detections > 3000


def test_the_three_split_bricks_cut_at_each_dc_update_equal_the_loop(oracle):
    x = cases.x20(sc.composite_stream(oracle))
    s1 = capi.cs11a_states(1)[0]; s2 = s1.copy(); b = 0; nb = len(x) // 4; events = 0
    while b < nb:
        s1, u1 = model.carrier_sense(x[4 * b:], s1, capi.CCA11A_STOP_ON_TIMEOUT)
        s2, u2 = model.carrier_sense_split(x[4 * b:], s2, capi.CCA11A_STOP_ON_TIMEOUT)
        assert u1 == u2 and np.array_equal(s1, s2), b
        b += u1; events += 1
        if s1[0] == 1:
            b += 200                                                             # a frame's worth of bursts go elsewhere
        capi.cca11a_reset(s1.reshape(1, -1)); capi.cca11a_reset(s2.reshape(1, -1))
    assert events > 20


def test_cut_into_two_calls_gives_what_one_call_gives(oracle):
    x = cases.x20(sc.composite_stream(oracle))[:4 * 1200]
    whole, used = model.carrier_sense(x, capi.cs11a_states(1)[0])
    for cut in range(0, used, 13):
        a, ua = model.carrier_sense(x[:4 * cut], capi.cs11a_states(1)[0])
        b, ub = model.carrier_sense(x[4 * ua:], a) if a[0] != 1 else (a, 0)
        assert ua + ub == used and np.array_equal(b, whole), cut


def test_viterbi_sig_equals_the_oracle(oracle):
    softs = cases.signal_softs(oracle)
    assert len(softs) >= 8 + 64 + 8 + 4
    for s in softs:
        assert model.viterbi_sig(s) == oracle.viterbi_sig(s)
    # the real SIGNAL symbols decode to words the parser accepts, at their rates
    for s, rate in zip(softs, cases.RATES):
        rec = model.plcp_parse(model.viterbi_sig(s))
        assert rec[0] == 0 and rec[1] == rate


def test_plcp_parse_equals_the_oracle_on_every_word_without_reserved_bits_and_on_words_with_one(oracle):
    words = cases.signal_words()
    assert len(words) == 131072 + 4096
    L = oracle.L
    kbps = ctypes.c_uint32(); ln = ctypes.c_uint16(); cr = ctypes.c_uint16(); ns = ctypes.c_uint16()
    rejects = {"reserved": 0, "parity": 0, "rate": 0, "length": 0}; ok = 0
    for w in words:
        w = int(w); rec = model.plcp_parse(w)
        good = L.so_parse_plcp(w, ctypes.byref(kbps), ctypes.byref(ln), ctypes.byref(cr), ctypes.byref(ns))
        if good:
            ok += 1
            assert list(rec) == [0, kbps.value, ln.value, cr.value, ns.value + 1], hex(w)
        else:
            assert rec[0] == 0x80000005 and rec[4] == 0, hex(w)
            kind = "reserved" if w & 0xFC0010 else "parity" if bin(w).count("1") & 1 else "rate" if (w & 0xF) < 8 else "length"
            rejects[kind] += 1
            # what each reject leaves behind, as include/sora_hip.h states it (PHY_11a.hpp:548-580: the fields are written in the order rate, code rate, length)
            if kind == "length":
                rate = RATE_OF_CODE[w & 0xF]
                assert list(rec) == [0x80000005, rate, (w >> 5) & 0xFFF, CODE_RATE_OF[rate], 0] and rec[2] > 2500, hex(w)
            else:
                assert list(rec) == [0x80000005, 0, 0, 0, 0], hex(w)
    assert ok > 10000 and min(rejects.values()) >= 1000, (ok, rejects)


def test_data_symbol_by_definition():
    rng = np.random.default_rng(5)
    x = rng.integers(-32768, 32768, (3 * 80 + 5, 2)).astype(np.int16)
    y = model.data_symbol(x[5:], 3)
    for k in range(3):
        assert np.array_equal(y[64 * k:64 * k + 64], x[5 + 80 * k + 8:5 + 80 * k + 72])


@pytest.mark.parametrize("rate_mhz", [40, 20])
def test_the_composition_over_the_models_bricks_equals_the_restatement_in_every_row(oracle, rate_mhz):
    """sora_amd.capi.rx11a_stages -- the walk rx11a_by_stages runs over the GPU's stages -- with the model's bricks: every event of every capture, no capture left out"""
    from gpu_util import batch
    caps = cases.composition_captures(oracle, rate_mhz)
    assert len(caps) == 1 + 25 + 16 + 48
    iq, descs = batch(caps)
    got = model.events(iq, [(o, n) for o, n, _ in descs], rate_mhz)
    kinds = set(); total = 0
    for k, c in enumerate(caps):
        want = oracle.rx_capture(c, rate_mhz, max_frames=16)
        why = cases.same_events(got[k], want)
        assert why is None, (rate_mhz, k, why)
        kinds |= {r["error_code"] for r in want}; total += len(want)
    assert total >= 60 and {0x1, 0x80000005} <= kinds, (total, kinds)


def test_the_record_helpers():
    s = capi.cs11a_states(2, 12345)
    assert s.shape == (2, 48) and s[0, 2] == 12345 and s[0, 44] == 8 and np.count_nonzero(s[0]) == 2
    s[:, 5:48] = 7; s[:, 0:2] = 9
    capi.cca11a_reset(s, context=False)
    assert (s[:, 5:44] == 0).all() and (s[:, 44] == 8).all() and (s[:, 45] == 0).all() and (s[:, 46] == 7).all() and (s[:, 0:5] == [9, 9, 12345, 0, 0]).all()
    capi.cca11a_reset(s)
    assert (s[:, 0:2] == 0).all()
    r = capi.cs11a_states(1)[0]; u = r.view(np.uint32); u[45] = model.pack((-3, 5)); u[46] = model.pack((7, -9))
    w = capi.cs11a_record_words(r)
    assert list(w[35:40].view(np.int32)) == [8, -3, 5, 7, -9]
