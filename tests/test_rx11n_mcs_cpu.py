"""sora_rx11n_set_mcs_max, checked without a GPU: the export is declared, bound, typed and refuses a null handle; the test-side model of the graph with
the gate moved (tests/rx11n_ext_model.py) is the oracle -- and, where oracle/_ref is built, the compiled reference graph -- event for event at the
reference's gate, decodes every reference-modulated MCS 11..14 frame through a clean channel with the gate at 14, and places those events where the
compiled graph places a frame of as many symbols; k_frame11n, which now holds ten de-interleaver entries per lane, keeps them in registers."""
import ctypes
import os

import numpy as np
import pytest

import rx11n_ext_model as model
from gpu_util import capture_11n, same_events_11n
from oracle.pyoracle import Oracle, ReferenceGraph
from test_capi_cpu import declared_functions
from test_stream11n_cpu import kernel_metadata

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SORA_ERR_INVALID_PARAM = -1
E_OK, E_PLCP, E_CRC = 0x1, 0x80000005, 0x80000006
NDBPS = {8: 52, 9: 104, 10: 156, 11: 208, 12: 312, 13: 416, 14: 468}


def recorded_frames():
    """{mcs: [(s0, s1, mpdu without FCS)]}: the reference modulator's recorded waveforms, MCS 8, 9, 10, 12 (refgraph_11n.npz) and, last in their lists, MCS 9 and
    11..14 of two data symbols each (refmod_11n_mcs11_14.npz)"""
    z = np.load(os.path.join(GOLD, "refgraph_11n.npz")); y = np.load(os.path.join(GOLD, "refmod_11n_mcs11_14.npz"))
    out = {}
    for i, mcs in enumerate((8, 9, 10, 12)):                                 # the MCS of tx0..tx3
        out.setdefault(mcs, []).append((z["tx%d_0" % i], z["tx%d_1" % i], z["mpdu%d" % i].tobytes()))
    for mcs in (9, 11, 12, 13, 14):
        out.setdefault(mcs, []).append((y["tx%d_0" % mcs], y["tx%d_1" % mcs], y["mpdu%d" % mcs].tobytes()))
    return out


def nsym_of(mcs, length_nofcs):
    return -(-(8 * (length_nofcs + 4) + 22) // NDBPS[mcs])


# ---- the entry point
def test_export_is_declared_bound_typed_and_refuses_a_null_handle():
    import sora_amd
    from sora_amd import capi
    lib = sora_amd.load(build_if_missing=False)
    n = "sora_rx11n_set_mcs_max"
    assert hasattr(lib, n) and n in declared_functions() and n in capi.EXPORTS
    assert lib.sora_rx11n_set_mcs_max.argtypes == [ctypes.c_void_p, ctypes.c_int]
    assert hasattr(capi.Rx11n, "set_mcs_max")
    for v in (14, 10, -1, 0, 99):
        lib.sora_hip_table_digest(None, None)                               # leaves a message that names no receive handle
        assert lib.sora_rx11n_set_mcs_max(None, v) == SORA_ERR_INVALID_PARAM
        assert n.encode() in lib.sora_hip_last_error()


# ---- the model at the reference's gate
def test_model_at_gate_10_is_the_oracle_and_the_reference_graph():
    """320 two-chain captures, 1-3 frames of MCS 8..14 each (the recorded waveforms), gains, phases, cross-talk, CFO, noise of sigma 3..1500, every third
    capture cut inside its last frame: position, code, MCS, length, FCS and MPDU bytes (CRC-failed ones included) of every event."""
    o = Oracle(); g = ReferenceGraph()
    fr = [(s0, s1) for v in recorded_frames().values() for s0, s1, _ in v]
    rng = np.random.default_rng(20261017)
    kinds = {}; nev = 0
    for t in range(320):
        pick = [fr[int(i)] for i in rng.integers(0, len(fr), size=int(rng.integers(1, 4)))]
        a, b = capture_11n(rng, pick, sigma=float(rng.choice([3, 20, 60, 200, 600, 1500])), cut=float(rng.uniform(0.05, 1.0)) if t % 3 == 2 else None)
        want = o.rx11n_capture(a, b); got = model.rx11n(a, b, mcs_max=10)
        assert got == want, (t, got, want)
        if g.available():
            ok, why = same_events_11n(got, g.rx11n(a, b), position="sample_index")
            assert ok, (t, why)
        nev += len(want)
        for e in want:
            kinds[e["error_code"]] = kinds.get(e["error_code"], 0) + 1
    assert model.parser_disagreements() == 0
    # decoded frames, refusals (the MCS 11..14 frames among them) and CRC failures all occur
    assert nev > 320 and kinds.get(E_OK, 0) > 80 and kinds.get(E_PLCP, 0) > 120 and kinds.get(E_CRC, 0) > 10, kinds


# ---- the model with the gate at 14
CLEAN_SEED = 20261018        # every frame below decodes under this seed (checked on the CPU with the model alone, recorded and live frames)


def clean_cases(rng):
    """(mcs, s0, s1, mpdu without FCS): the recorded frames, and, where the reference modulator is compiled, lengths 1, 2, 40, 1495, 1496 and random"""
    rec = recorded_frames(); g = ReferenceGraph()
    for mcs in (11, 12, 13, 14):
        s0, s1, mp = rec[mcs][-1]
        for _ in range(10):
            yield mcs, s0, s1, mp
        if g.available():
            for ln in (1, 2, 40, 1495, 1496, int(rng.integers(1, 1497)), int(rng.integers(1, 1497))):
                mp = rng.integers(0, 256, ln).astype(np.uint8).tobytes()
                s0, s1 = g.tx11n(mp, mcs)
                yield mcs, s0, s1, mp


def test_model_at_gate_14_decodes_every_reference_modulated_frame():
    """unit gain, random phase per chain, cross-talk 0 or 0.1, CFO up to 2e-4 rad/sample, sigma 10..20: FRAME_OK and exactly the transmitted bytes + FCS,
    no frame left out; the same capture at the reference's gate is one PLCP header failure"""
    rng = np.random.default_rng(CLEAN_SEED)
    n = 0
    for mcs, s0, s1, mp in clean_cases(rng):
        a, b = model.clean_channel(rng, s0, s1, sigma=float(rng.uniform(10, 20)))
        ev = model.rx11n(a, b, mcs_max=14)
        assert [(e["error_code"], e["rate_kbps"], e["length"]) for e in ev] == [(E_OK, mcs, len(mp) + 4)], (n, mcs, len(mp), ev)
        assert ev[0]["mpdu"] == mp + model.fcs(mp) and ev[0]["crc32"] == int.from_bytes(model.fcs(mp), "little"), (n, mcs, len(mp))
        assert [e["error_code"] for e in model.rx11n(a, b, mcs_max=10)] == [E_PLCP]
        assert [e["error_code"] for e in model.rx11n(a, b, mcs_max=mcs - 1)] == [E_PLCP]
        n += 1
    assert n >= 40


def test_an_mcs_11_14_event_falls_where_the_compiled_graph_puts_a_frame_of_as_many_symbols():
    """The same place, noise and channel draw, once with an MCS 11..14 frame and once with an MCS 8..10 frame of as many data symbols: the first one's
    end_sample under the model at gate 14 is the second one's position as the oracle reports it and, where oracle/_ref is built, as the compiled reference
    graph reports it (sample_index).  Recorded frames (two symbols each, against the recorded two-symbol MCS 9 frame); with the reference modulator
    compiled also 3, 5 and 26 symbols."""
    o = Oracle(); g = ReferenceGraph(); rec = recorded_frames()
    pairs = []
    low = [f for f in rec[9] if nsym_of(9, len(f[2])) == 2][0]
    for mcs in (11, 12, 13, 14):
        assert nsym_of(mcs, len(rec[mcs][-1][2])) == 2
        pairs.append((mcs, rec[mcs][-1], 9, low))
    if g.available():
        rng = np.random.default_rng(5)
        for mcs in (11, 12, 13, 14):
            for ns, lo in ((3, 8), (5, 9), (26, 10)):
                la = min((ns * NDBPS[mcs] - 22) // 8 - 4, 1496); lb = (ns * NDBPS[lo] - 22) // 8 - 4
                assert nsym_of(mcs, la) == ns and nsym_of(lo, lb) == ns
                ma = rng.integers(0, 256, la).astype(np.uint8).tobytes(); mb = rng.integers(0, 256, lb).astype(np.uint8).tobytes()
                pairs.append((mcs, g.tx11n(ma, mcs) + (ma,), lo, g.tx11n(mb, lo) + (mb,)))
    for k, (mcs, fa, lo, fb) in enumerate(pairs):
        for lead in (300, 307, 1111):
            a0, a1 = model.clean_channel(np.random.default_rng(100 + k), fa[0], fa[1], sigma=12.0, lead=lead)
            b0, b1 = model.clean_channel(np.random.default_rng(100 + k), fb[0], fb[1], sigma=12.0, lead=lead)
            ea = model.rx11n(a0, a1, mcs_max=14); eb = o.rx11n_capture(b0, b1)
            assert [(e["error_code"], e["rate_kbps"]) for e in ea] == [(E_OK, mcs)] and [(e["error_code"], e["rate_kbps"]) for e in eb] == [(E_OK, lo)], (k, lead)
            assert ea[0]["end_sample"] == eb[0]["end_sample"], (k, lead)
            if g.available():
                er = g.rx11n(b0, b1)
                assert [e["error_code"] for e in er] == [E_OK] and ea[0]["end_sample"] == er[0]["sample_index"], (k, lead)


# ---- the kernels' registers
def test_frame_and_scan_kernels_keep_everything_in_registers(tmp_path):
    md = kernel_metadata(tmp_path)
    seen = set()
    for name, v in md.items():
        for k in ("k_frame11n", "k_finish11n", "k_scan11n", "k_scan11n_stream"):
            if ("%d%sE" % (len(k), k)) in name:
                seen.add(k)
                assert v["private_segment_fixed_size"] == 0 and v.get("vgpr_spill_count", 0) == 0, (k, v)
    assert seen == {"k_frame11n", "k_finish11n", "k_scan11n", "k_scan11n_stream"}, sorted(md)
