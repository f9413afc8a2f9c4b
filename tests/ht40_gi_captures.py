"""Raw captures that hold SHORT-GI frames, for the 40 MHz HT front end in SORA_HT40_GUARD_SIGNALLED (tests/test_gpu_ht40_gi_front.py, tests/test_gpu_stream_ht40_gi.py;
DESIGN.md section 7 g4).  The frames are tests/tx_ht40_gi_model.py's integer frames (HT-SIG bit 31 set, data symbols of 144 samples) in py_ht40.tx_frame's unit, through
tests/ht40_front_captures.py's float channel; where a case depends on the receiver's own timing -- a frame whose short extent ends on the capture's last sample -- the cut
is placed with the model's a20 (tests/ht40_front_gi_model.py), as that set does it.  TEST INFRASTRUCTURE."""
import numpy as np

from oracle import py_ht40 as m
import ht40_front_captures as fc
import ht40_front_gi_model as fg
import tx_ht40_gi_model as TG
from level_captures import whole

MAX_EVENTS = 4                                         # max_frames_per_capture of the GPU runs: only `slots` raises more


def frame(rng, mcs, length, gi, joint=False, ht_mcs=None, oracle=None):
    """a frame whose PSDUs have `length` bytes (FCS included) -> (complex128 [2, n] in tx_frame's unit, nsym, psdus).  ht_mcs: what HT-SIG says instead of mcs"""
    ps = [m.add_fcs(rng.integers(0, 256, length - 4, dtype=np.uint8).tobytes()) for _ in range(1 if joint else 2)]
    fr, nsym, _ = TG.frame_int(ps[0] if joint else ps, mcs, gi, joint=joint, oracle=oracle)
    if ht_mcs is not None:
        fr = fr.copy(); fr[:, 640:1120] = TG.sig_symbols(ht_mcs, length, nsym, gi, oracle=oracle)
    return (fr[..., 0].astype(float) + 1j * fr[..., 1].astype(float)) * (128.0 / TG.T.A), nsym, ps


def _first(pair, joint, guard=True):
    ev = fg.front(pair[0], pair[1], guard=guard, joint=joint)
    return ev[0] if ev else None


def build(joint=False, oracle=None):
    """-> [Cap]: tags name what the capture is there for"""
    out = []
    rng = lambda: np.random.default_rng([20261021, int(joint), len(out)])

    def add(name, pair, sent=(), tags=()):
        out.append(fc.Cap(name, "short_gi", fc.each(whole, pair), sent, tags))

    def one(name, mcs, length, gi, lead=400, tail=600, sigma=8.0, cfo_step=0.0, tags=(), **kw):
        r = rng()
        x, nsym, ps = frame(r, mcs, length, gi, joint, oracle=oracle, **kw)
        pair = fc.gauss(fc.cat(fc.quiet(lead), fc.through(x, cfo_step=cfo_step), fc.quiet(tail)), r, sigma)
        add(name, pair, [{"mcs": mcs, "length": length, "nsym": nsym, "gi": gi, "psdus": ps, "sound": "ht_mcs" not in kw}], tags)

    # ---- every MCS behind the short guard interval, lengths on both sides of a symbol-count step, and long frames between them
    for mcs in range(8, 15):
        for k, L in enumerate(fc.step_lengths(mcs, joint=joint)):
            one("short mcs%d len%d" % (mcs, L), mcs, L, 1, lead=300 + 4 * mcs, cfo_step=(0.0, 21.0, -37.25)[(mcs + k) % 3], tags={"short"})
    one("long mcs11 len90", 11, 90, 0, tags={"long"})
    one("short mcs14 len4000", 14, 4000, 1, tags={"short"})
    # ---- the short extent against the capture's end, placed by the model's timing
    for lead in range(400, 400 + 8 * 14, 8):           # a20 moves in steps of 4 with the lead: one of seven leads puts the short extent's end on a source-call boundary
        x, nsym, ps = frame(np.random.default_rng([79, int(joint)]), 11, 150, 1, joint, oracle=oracle)
        pair = fc.each(whole, fc.cat(fc.quiet(lead), fc.through(x), fc.quiet(600)))
        e = _first(pair, joint)
        if e is None or e["error_code"] or not e["short_gi"]:
            continue
        end20 = e["a20"] + 240 + 72 * e["nsym"]
        if end20 % 14 == 0:
            sent = [{"mcs": 11, "length": 150, "nsym": nsym, "gi": 1, "psdus": ps, "sound": True}]
            add("short extent ends on the last sample", fc.each(lambda a: a[:2 * end20], pair), sent, {"exact"})
            add("short extent ends 28 samples early", fc.each(lambda a: a[:2 * end20 - 28], pair), (), {"short28"})
            # the long extent (8 nsym kept samples more) passes the end, the short one does not
            mid = 2 * end20 + 28 * max(1, (8 * e["nsym"]) // 28)
            assert 2 * end20 < mid < 2 * (e["a20"] + 240 + 80 * e["nsym"])
            add("fits only because it is short", fc.each(lambda a: a[:mid], pair), sent, {"only_short"})
            break
    # ---- a short frame, then a second frame a few hundred samples behind it: its detection depends on the origin behind the first
    for g, (gi0, gi1) in enumerate(((1, 0), (1, 1), (0, 1))):
        r = rng()
        xa, na, pa = frame(r, 10, 60, gi0, joint, oracle=oracle); xb, nb_, pb = frame(r, 12, 90, gi1, joint, oracle=oracle)
        pair = fc.gauss(fc.cat(fc.quiet(400), fc.through(xa), fc.quiet(300 + 60 * g), fc.through(xb), fc.quiet(28 * 30)), r, 8.0)
        add("two frames, kinds %d %d" % (gi0, gi1), pair, [{"mcs": 10, "length": 60, "nsym": na, "gi": gi0, "psdus": pa, "sound": True},
                                                              {"mcs": 12, "length": 90, "nsym": nb_, "gi": gi1, "psdus": pb, "sound": True}], {"two"})
    # ---- a header that fails with bit 31 set: MCS 15 behind a sound CRC-8
    one("gate mcs15, short", 9, 60, 1, ht_mcs=15, tags={"gate"})
    # ---- more events than row slots, short and long alternating: the last slot's rows carry both flags
    r = rng(); parts, sent = [fc.quiet(280)], []
    for i in range(MAX_EVENTS + 2):
        gi = 0 if i == 1 else 1
        x, nsym, ps = frame(r, 9 + i % 5, 24 + i, gi, joint, oracle=oracle)
        sent.append({"mcs": 9 + i % 5, "length": 24 + i, "nsym": nsym, "gi": gi, "psdus": ps, "sound": True})
        parts += [fc.through(x), fc.quiet(420)]
    add("%d events" % (MAX_EVENTS + 2), fc.gauss(fc.cat(*parts), r, 8.0), sent, {"slots"})
    return out


def want_records(caps, joint, guard):
    """the model's events per capture in the shape tests/test_gpu_ht40_front.check_records reads: the library's record fields (mcs with SORA_HT40_SHORT_GI on it) and S"""
    return [[dict(fg.found(e), S=e["S"], short_gi=e["short_gi"]) for e in fg.front(c.iq[0], c.iq[1], guard=guard, joint=joint)] for c in caps]
