"""The traffic result delivery is held to its contract on (tests/deliver_model.py, tests/test_gpu_deliver.py): per handle eight distinct base captures, made with the
project's own GPU transmitters and the loop-back recipes of the handles' parity tests, and calls that are sequences of kind indices tiled into one buffer.  The
named cases and their coverage assertions are computed from the kinds alone (tests/test_deliver_model_cpu.py runs them without a GPU), so a case cannot silently
lose what it is for.  TEST INFRASTRUCTURE.

The truth per distinct capture comes once, on the CPU, from the model the handle's parity tests use (oracle.rx_capture, rx11b_ext_model at the short-preamble
mode -- the oracle's rows plus the flag --, oracle.rx11n_capture, ht40_front_model plus the transmitted PSDUs).  The table assembly is under test here, not the
decoders: test_gpu_deliver.py also asserts that truth against the transmitted bytes and against SPEC below.

The delivery kernels scan UNITS in tiles of 1024: captures for the 802.11a / b / n handles, frames for the 40 MHz HT descriptor form, EVENTS for its raw-capture
form (an empty capture is no unit there, a capture with three events is three).  units() says where the tile edges of a call fall."""
import numpy as np

import deliver_model as dm

SILENCE, NOISE, HEADER, ONE, CRC, TWO, FOUR, LARGEST = range(8)
NAMES = ("silence", "noise", "header fails", "one byte", "FCS fails", "two frames", "four frames", "largest")
HANDLES = ("11a", "11b", "11n", "ht40")
TILE = 1024
COUNTS = (1, 1023, 1024, 1025, 2049, 3073)
# payload bytes (without FCS) of the frames of each kind; LARGEST: what the handle's header gate admits -- k_scan.hip's SIGNAL parser refuses LENGTH > 2500, the
# 802.11b PLCP parser has no bound (dev_11b.h: any LENGTH behind a good CRC-16), so the transmitter's 4092 bytes, which fill the row's 4096-byte slot; dev_11n.h /
# k_rx11n.hip refuse an HT LENGTH > 1500; the 40 MHz front end's gate is 4 <= LENGTH <= 4000 (sora_hip.h)
PAYLOAD = {ONE: (1,), CRC: (40,), TWO: (33, 61), FOUR: (7, 20, 9, 15), HEADER: (1,)}
LARGEST_PAYLOAD = {"11a": 2496, "11b": 4092, "11n": 1496, "ht40": 3996}
ROWS_PER_FRAME = {"11a": 1, "11b": 1, "11n": 1, "ht40": 2}


def spec(handle):
    """-> {kind: [(error_code, length with FCS)]}: the frames each base capture is built to yield, in time order"""
    ok = lambda k: [(dm.E_FRAME_OK, n + 4) for n in PAYLOAD[k]]
    return {SILENCE: [], NOISE: [], HEADER: [(dm.E_PLCP_HEADER_FAIL, 0)], ONE: ok(ONE), CRC: [(dm.E_CRC32_FAIL, PAYLOAD[CRC][0] + 4)], TWO: ok(TWO), FOUR: ok(FOUR),
            LARGEST: [(dm.E_FRAME_OK, LARGEST_PAYLOAD[handle] + 4)]}


def capture_id(i):
    """out of order and non-contiguous, distinct below 100003 captures"""
    return (7919 * i + 13) % 100003


# ---- the named cases ------------------------------------------------------------------------------------------------------------------------------------------------
ONE_ROW = (ONE, HEADER, CRC)                                # kinds of exactly one frame: with them a capture index is also an event index
MIXED = (ONE, HEADER, CRC, HEADER, TWO, NOISE)


class Case:
    def __init__(self, name, kinds, mf, purpose):
        self.name, self.kinds, self.mf, self.purpose = name, np.asarray(kinds, np.uint8), mf, purpose
        assert len(self.kinds) in COUNTS, (name, len(self.kinds))

    def __repr__(self):
        return self.name


def _cycle(kinds, n, start=0):
    return [kinds[(start + i) % len(kinds)] for i in range(n)]


def _edges(n, at, first, second):
    """one-frame captures everywhere, `first` at captures at[...] and `second` right behind"""
    k = _cycle(ONE_ROW, n)
    for a in at:
        k[a] = first; k[a + 1] = second
    return k


def cases():
    trunc = {3: FOUR, 1: TWO}
    out = [Case("single", [TWO], 3, "single")]
    for mf in (3, 1):
        out.append(Case("truncated_then_empty_mf%d" % mf, _edges(2049, (1023, 2047), trunc[mf], SILENCE), mf, "truncated_last_lane"))
        out.append(Case("empty_then_truncated_mf%d" % mf, _edges(2049, (1023, 2047), SILENCE, trunc[mf]), mf, "truncated_first_lane"))
    out.append(Case("empty_tile", _cycle(MIXED, 1024) + _cycle((SILENCE, NOISE), 1024) + _cycle(MIXED, 1025, 2), 3, "empty_tile"))
    out.append(Case("all_truncated_mf1", [TWO] * 1025, 1, "all_truncated"))
    out.append(Case("all_truncated_mf2", [FOUR] * 1023, 2, "all_truncated"))
    mixed = _cycle(MIXED, 1025)
    mixed[1021] = LARGEST; mixed[1024] = LARGEST
    out.append(Case("mixed_1025", mixed, 3, "mixed"))
    out.append(Case("mixed_1024", _cycle(MIXED, 1024, 1), 3, "mixed"))
    return out


def by_name(name):
    return next(c for c in cases() if c.name == name)


def found(handle, kind):
    return len(spec(handle)[kind])


def units(handle, case):
    """per capture, the units of the delivery's scan it makes: 1 for the capture-scanning handles, its events (rows / 2) for the 40 MHz raw-capture form"""
    if handle != "ht40":
        return np.ones(len(case.kinds), np.int64)
    return np.array([min(found(handle, k), case.mf) for k in case.kinds], np.int64)


def frames_of(handle, case):
    """per capture: [(error_code, length, truncated)] of its rows' frames (one entry per frame; the 40 MHz handle makes two rows of a recorded one)"""
    s = spec(handle)
    out = []
    for k in case.kinds:
        fr = s[k]
        out.append([(e, n, i == case.mf - 1 and len(fr) > case.mf) for i, (e, n) in enumerate(fr[:case.mf])])
    return out


def totals(handle, case):
    """closed form, from the kinds: (rows, MPDU bytes) of the call"""
    s = spec(handle)
    rows = nbytes = 0
    for k, cnt in zip(*np.unique(case.kinds, return_counts=True)):
        fr = s[int(k)][:case.mf]
        per = lambda e: ROWS_PER_FRAME[handle] if e != dm.E_PLCP_HEADER_FAIL else 1
        rows += int(cnt) * sum(per(e) for e, _ in fr)
        nbytes += int(cnt) * sum(per(e) * min(n, 4096) for e, n in fr if e != dm.E_PLCP_HEADER_FAIL)
    return rows, nbytes


def check_coverage(handle, case):
    """what the case is for, asserted from the kinds and SPEC alone"""
    fr = frames_of(handle, case)
    nfound = np.array([found(handle, k) for k in case.kinds])
    u = units(handle, case)
    first_unit = np.concatenate([[0], np.cumsum(u)[:-1]])
    n = len(case.kinds)
    if case.purpose == "single":
        assert n == 1 and nfound[0] >= 1
    elif case.purpose in ("truncated_last_lane", "truncated_first_lane"):
        t, e = (1023, 1024) if case.purpose == "truncated_last_lane" else (1024, 1023)
        for base in (0, 1024):
            assert nfound[base + t] > case.mf and nfound[base + e] == 0, (case, base)
            assert fr[base + t][-1][2] and not fr[base + e]
        assert all(nfound[i] == 1 for i in range(1023)), "capture 1023 is unit 1023 for every handle"
        if handle == "ht40":                                 # the scan's lanes are events there: the flagged event lies on the tile's edge, an empty capture is no lane
            flagged = first_unit[t] + case.mf - 1
            assert flagged in ((1023, 1025) if t == 1023 else (1023 + case.mf - 1,)), (case, flagged)
            assert u.sum() > TILE
    elif case.purpose == "empty_tile":
        assert n == 3073 and not nfound[1024:2048].any() and nfound[:1024].sum() > 1000 and nfound[2048:].sum() > 1000
        assert len(set(case.kinds[1024:2048])) == 2
        if handle == "ht40":
            assert u.sum() > TILE                            # (no unit is empty there; the tile edge is crossed all the same)
    elif case.purpose == "all_truncated":
        assert (nfound > case.mf).all() and all(f[-1][2] for f in fr)
        assert n > TILE or case.mf == 2
        if case.mf == 1:
            assert u.sum() > TILE
    elif case.purpose == "mixed":
        # in every tile of units: a row without bytes between two rows with bytes
        owns = [(int(first_unit[c]) + i, e != dm.E_PLCP_HEADER_FAIL) for c, f in enumerate(fr) for i, (e, _, _) in enumerate(f)]
        for tile in range(int(-(-u.sum() // TILE))):
            seq = [o for at, o in owns if at // TILE == tile]
            if len(seq) >= 3:
                assert any(seq[i - 1] and not seq[i] and seq[i + 1] for i in range(1, len(seq) - 1)), (case, tile)
        assert u.sum() >= TILE and (n != 1025 or (case.kinds == LARGEST).sum() == 2)
    else:
        raise AssertionError(case.purpose)


HT40_DESC_FRAMES = (1025, 2049)                              # the descriptor form: frames of the shortest data field, per-stream and joint coding


# ---- base captures (GPU transmitters; the receivers' own loop-back recipes) -------------------------------------------------------------------------------------------
def _payloads(rng, handle):
    p = {k: [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in v] for k, v in PAYLOAD.items()}
    p[LARGEST] = [rng.integers(0, 256, LARGEST_PAYLOAD[handle], dtype=np.uint8).tobytes()]
    p[SILENCE] = p[NOISE] = []
    return p


def _whole(x):
    n = (len(x) + 27) // 28 * 28
    return np.ascontiguousarray(np.concatenate([x, np.zeros((n - len(x),) + x.shape[1:], x.dtype)]))


def _noise(rng, n, sigma):
    return np.rint(rng.normal(0, sigma, (n, 2))).astype(np.int16)


class Base:
    """caps[kind]: int16 [n, 2] (a pair of them for the two-chain handles); sent[kind]: the payloads transmitted, in time order"""
    def __init__(self, handle, caps, sent):
        self.handle, self.caps, self.sent, self.chains = handle, caps, sent, 2 if handle in ("11n", "ht40") else 1

    def length(self, kind):
        return len(self.caps[kind][0] if self.chains == 2 else self.caps[kind])


def base_11a(sora, seed=4101):
    """test_gpu_tx.py's loop back: COMPLEX8 << 8 at 40 MHz, 400 samples of silence behind every frame (240 in front of the first); the SIGNAL symbol of `header
    fails` is blanked (it decodes to rate code 0, which the parser refuses), one data symbol of `FCS fails` is blanked"""
    rng = np.random.default_rng(seed); sent = _payloads(rng, "11a"); caps = {}
    for k in range(8):
        if k == SILENCE:
            caps[k] = np.zeros((28, 2), np.int16); continue
        if k == NOISE:
            caps[k] = _noise(rng, 28 * 20, 20.0); continue
        out, off = sora.tx11a(sent[k], [54000 if k == LARGEST else 24000] * len(sent[k]), [1 + 5 * i for i in range(len(sent[k]))])
        w = out.cpu().numpy().astype(np.int16) << 8
        parts = [np.zeros((240, 2), np.int16)]
        for f in range(len(sent[k])):
            x = w[off[f]:off[f + 1]].copy()
            if k == HEADER:
                x[640:800] = 0
            if k == CRC:
                x[800 + 160:800 + 320] = 0
            parts += [x, np.zeros((400, 2), np.int16)]
        caps[k] = _whole(np.concatenate(parts))
    return Base("11a", caps, sent)


def base_11b(sora, seed=4102):
    """test_gpu_11b_short.py's loop back (rx11b_ext_model.capture): short preamble, 11 Mbps, COMPLEX8 x 96, a floor of sigma 5; one header symbol of `header fails`
    is negated (the CRC-16 fails) and the frame ends with its header, one code word of `FCS fails` is negated"""
    import rx11b_ext_model as rxm
    rng = np.random.default_rng(seed); sent = _payloads(rng, "11b"); caps = {}
    for k in range(8):
        if k == SILENCE:
            caps[k] = np.zeros((28, 2), np.int16); continue
        if k == NOISE:
            caps[k] = _noise(rng, 28 * 40, 10.0); continue
        out, off = sora.tx11b(sent[k], 11000, preamble=1)
        w = out.cpu().numpy()
        waves = []
        for f in range(len(sent[k])):
            x = w[off[f]:off[f + 1]].copy()
            if k == HEADER:                                  # (and nothing behind the header: a data field without one raises a time-out of its own)
                x = x[:96 * 44 + 22]
                x[72 * 44 + 5 * 44:72 * 44 + 6 * 44] = -x[72 * 44 + 5 * 44:72 * 44 + 6 * 44]
            if k == CRC:
                x[96 * 44 + 10 * 32:96 * 44 + 11 * 32] = -x[96 * 44 + 10 * 32:96 * 44 + 11 * 32]
            waves.append(x)
        caps[k] = rxm.capture(rng, waves, [1500] + [600] * (len(waves) - 1), 5.0)
    return Base("11b", caps, sent)


def base_11n(sora, seed=4103):
    """test_gpu_tx11n.py's loop back: 400 samples of silence, 10 % cross-talk, sigma 20, frame after frame; `header fails` is an MCS 12 frame, which the SIG
    parser's gate refuses (mcs_max 10, the reference's); one data symbol of `FCS fails` is blanked"""
    from test_gpu_tx11n import loopback_capture
    rng = np.random.default_rng(seed); sent = _payloads(rng, "11n"); caps = {}
    for k in range(8):
        if k == SILENCE:
            caps[k] = (np.zeros((28, 2), np.int16), np.zeros((28, 2), np.int16)); continue
        if k == NOISE:
            caps[k] = (_noise(rng, 28 * 20, 20.0), _noise(rng, 28 * 20, 20.0)); continue
        o0, o1, off = sora.tx11n(sent[k], [12 if k == HEADER else 10 if k == LARGEST else 8] * len(sent[k]))
        o0, o1 = o0.cpu().numpy(), o1.cpu().numpy()
        a, b = [], []
        for f in range(len(sent[k])):
            s0, s1 = o0[off[f]:off[f + 1]].astype(np.float64), o1[off[f]:off[f + 1]].astype(np.float64)
            if k == CRC:
                s0[1600 + 160:1600 + 320] = 0; s1[1600 + 160:1600 + 320] = 0
            x, y = loopback_capture(rng, s0, s1)
            a.append(x); b.append(y)
        caps[k] = (np.ascontiguousarray(np.concatenate(a)), np.ascontiguousarray(np.concatenate(b)))
    return Base("11n", caps, sent)


HT40_MCS = {HEADER: 9, ONE: 14, CRC: 9, TWO: 11, FOUR: 13, LARGEST: 14}


def base_ht40(sora, seed=4104):
    """test_gpu_tx_ht40.py's loop back: the transmitter's chains through H_MIX at the level the receiver's tests decode at, 400 samples of silence in front of every
    frame and 800 behind the last, sigma 8; both HT-SIG symbols of `header fails` are blanked (ht40_front_captures' spoiled CRC-8, on a sent waveform), one data
    symbol of `FCS fails`.  sent[kind]: per frame the two streams' payloads"""
    import tx_ht40_model as T
    gain = 250.0 * 128.0 / T.A
    H = np.array([[1.0, 0.3j], [-0.25, 0.9j]]) * gain
    rng = np.random.default_rng(seed); sent = {}; caps = {}
    p0, p1 = _payloads(rng, "ht40"), _payloads(rng, "ht40")
    for k in range(8):
        sent[k] = list(zip(p0[k], p1[k]))
        if k == SILENCE:
            caps[k] = (np.zeros((28, 2), np.int16), np.zeros((28, 2), np.int16)); continue
        if k == NOISE:
            caps[k] = (_noise(rng, 28 * 20, 8.0), _noise(rng, 28 * 20, 8.0)); continue
        o0, o1, off = sora.tx_ht40(p0[k], p1[k], [HT40_MCS[k]] * len(p0[k]), [(3 + 2 * i, 90 - i) for i in range(len(p0[k]))])
        o0, o1 = o0.cpu().numpy().astype(np.float64), o1.cpu().numpy().astype(np.float64)
        segs = []
        for f in range(len(p0[k])):
            x = np.stack([o[off[f]:off[f + 1], 0] + 1j * o[off[f]:off[f + 1], 1] for o in (o0, o1)])
            if k == HEADER:
                x[:, 800:1120] = 0
            if k == CRC:
                x[:, 1600 + 160:1600 + 320] = 0
            segs += [np.zeros((2, 400), complex), H @ x]
        y = np.concatenate(segs + [np.zeros((2, 800), complex)], axis=1)
        y = np.stack([y.real, y.imag], -1) + rng.normal(0, 8.0, y.shape + (2,))
        y = np.clip(np.rint(y), -32768, 32767).astype(np.int16)
        caps[k] = (_whole(y[0]), _whole(y[1]))
    return Base("ht40", caps, sent)


BUILD = {"11a": base_11a, "11b": base_11b, "11n": base_11n, "ht40": base_ht40}


# ---- the truth per distinct capture (CPU) -----------------------------------------------------------------------------------------------------------------------------
def _fcs(payload):
    import zlib
    return bytes(payload) + zlib.crc32(bytes(payload)).to_bytes(4, "little")


def truth(base, oracle, max_frames=16):
    """-> {kind: frames found, in time order, as deliver_model takes them}"""
    out = {}
    for k in range(8):
        c = base.caps[k]
        if base.handle == "11a":
            fr = oracle.rx_capture(c, 40, max_frames=max_frames)
        elif base.handle == "11b":
            import rx11b_ext_model as rxm
            fr = rxm.rx11b(c, 1, max_frames=max_frames)
        elif base.handle == "11n":
            fr = oracle.rx11n_capture(c[0], c[1], max_frames=max_frames)
        else:
            fr = _truth_ht40(base, k)
        out[k] = [{f: v for f, v in r.items() if f in dm.FIELDS + ("mpdu", "streams")} for r in fr]
        for r in out[k]:
            r.pop("mpdu_offset", None); r.pop("capture_id", None)
    return out


def _truth_ht40(base, k):
    """events of the front-end model; a recorded frame's two rows from the transmitted PSDUs (FRAME_OK, or CRC32_FAIL with the bytes as decoded -- those are not
    known here: "mpdu" None, test_gpu_deliver.py fills them in from the lone call and says so)"""
    import ht40_front_model as fm
    ev = fm.front(base.caps[k][0], base.caps[k][1], flags=fm.OWN)
    out, f = [], 0
    for e in ev:
        if e["error_code"]:
            out.append({"end_sample": e["end_sample"], "error_code": e["error_code"], "streams": None})
            continue
        ps = [_fcs(p) for p in base.sent[k][f]]; f += 1
        bad = k == CRC
        out.append({"end_sample": e["end_sample"], "error_code": 0, "rate_kbps": e["mcs"], "nsym": e["nsym"],
                    "streams": [{"error_code": dm.E_CRC32_FAIL if bad else dm.E_FRAME_OK, "length": len(p), "crc32": None if bad else int.from_bytes(p[-4:], "little"),
                                 "mpdu": None if bad else p} for p in ps]})
    return out


# ---- calls ------------------------------------------------------------------------------------------------------------------------------------------------------------
def tile(base, kinds):
    """-> (iq int16 [N, 2], or the pair of chains; descs [(offset, nsamples, capture_id)] as a packed array of Rx.CAPTURE_DTYPE's fields)"""
    kinds = np.asarray(kinds)
    lens = np.array([base.length(k) for k in range(8)], np.int64)[kinds]
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]])
    assert not (offs % 4).any()
    descs = np.zeros(len(kinds), np.dtype([("offset", "<u8"), ("nsamples", "<u4"), ("capture_id", "<u4")]))
    descs["offset"] = offs; descs["nsamples"] = lens; descs["capture_id"] = [capture_id(i) for i in range(len(kinds))]
    if base.chains == 2:
        iq = tuple(np.concatenate([base.caps[k][c] for k in kinds]) for c in range(2))
    else:
        iq = np.concatenate([base.caps[k] for k in kinds])
    return iq, descs


def model_captures(handle, tr, kinds, mf):
    """the call as deliver_model takes it"""
    caps = [(capture_id(i), tr[int(k)], mf) for i, k in enumerate(kinds)]
    return dm.ht40_capture_call(caps) if handle == "ht40" else caps
