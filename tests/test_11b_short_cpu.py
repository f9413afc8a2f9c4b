"""The 802.11b short preamble, the parts that need no GPU: the two models are pinned to the reference where the reference goes (long
preamble), the C ABI's additions, and the loop-back through the models alone -- which is what makes "the GPU equals the model" mean something.

tests/tx11b_model.py at preamble 0 against the compiled reference modulator and the recorded waveforms; tests/rx11b_ext_model.py at mode 0
against oracle/so_rx11b.c, event for event; then short-preamble frames of the TX model through the RX model at mode 1 (decoded, flagged) and at
mode 0 (nothing decoded: the test that fails without the feature), and captures that mix both kinds."""
import ctypes
import os
import re

import numpy as np
import pytest

import rx11b_ext_model as rxm
import tx11b_model as txm
from oracle.pyoracle import Oracle, ReferenceGraph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
E_OK = 0x1
LOOPBACK_SEED = 1107            # the seed of the 300-frame loop-back: the models alone meet the 95 % condition with it (they do with every seed tried: 1100..1109)


@pytest.fixture(scope="module")
def o():
    return Oracle()


@pytest.fixture(scope="module")
def sora():
    import sora_amd
    sora_amd.load()
    return sora_amd


# ------------------------------------------------------------------ the TX model at preamble 0 is the reference's modulator
def test_tx_model_equals_the_recorded_waveforms():
    from test_tx11b_cpu import recorded_frames, start_parity
    frames = recorded_frames()
    assert len(frames) == 12
    for name, k, rate, mp, s in frames:
        got, _ = txm.tx11b(mp, rate, phase_in=start_parity(s), preamble=0)
        assert got.dtype == s.dtype and np.array_equal(got, s), (name, k)


def test_tx_model_equals_the_compiled_reference_modulator():
    """All four rates, lengths 1, 2, 13, 14, 100, 1500, 4092.  The reference keeps last_phase from frame to frame (one process, no reset), so
    the frames form one chain: each starts from the last_phase the model says the one before left, and the run passes through all four values."""
    from test_tx11b_cpu import ref_tx11b, start_parity
    g = ReferenceGraph()
    if not g.available():
        pytest.skip("oracle/_ref/libsora_refgraph.so not built (needs the reference tree)")
    rng = np.random.default_rng(1101)
    phase = None; seen = set()
    for ln in (1, 2, 13, 14, 100, 1500, 4092):
        for rate in (1000, 2000, 5500, 11000):
            mp = rng.integers(0, 256, ln).astype(np.uint8).tobytes()
            want = ref_tx11b(g, mp, rate)
            if phase is None:
                phase = 3 * start_parity(want)                # whatever this process modulated before: only the low bit is visible, and only it matters
            else:
                assert phase & 1 == start_parity(want), (rate, ln)
                seen.add(phase)
            got, phase = txm.tx11b(mp, rate, phase_in=phase, preamble=0)
            assert np.array_equal(got, want), (rate, ln)
    assert seen == {0, 1, 2, 3}, seen


def test_short_frame_geometry():
    """9 x 88 + 6 x 44 = 1056 header chips; the payload is the long frame's, chip for chip, up to the start phase and the scrambler's state"""
    mp = bytes(range(40))
    for rate in (2000, 5500, 11000):
        s, _ = txm.tx11b(mp, rate, preamble=1); l, _ = txm.tx11b(mp, rate, preamble=0)
        assert len(s) == 96 * 44 + 44 * txm.CHIPS_PER_BYTE[rate] * 4 + 24 == len(l) - 96 * 44
    assert txm.samples(40, 1000, 1) == 0 and txm.samples(40, 2000, 7) == 0


# ------------------------------------------------------------------ the RX model at mode 0 is oracle/so_rx11b.c
def same_events(a, b):
    return [rxm.key(r) for r in a] == [rxm.key({**r, "flags": 0}) for r in b]


@pytest.mark.parametrize("fixture", ["refgraph_11b.npz", "refgraph_11b_cck.npz"])
def test_rx_model_mode0_equals_the_oracle_on_the_fixtures(o, fixture):
    from test_oracle_11b import channel_11b
    z = np.load(os.path.join(GOLD, fixture))
    nok = 0
    for f in range(int(z["frames"])):
        for rep in range(3):
            c = channel_11b(z["tx_%d" % f], 100 * f + rep)
            want = o.rx11b_capture(c)
            assert same_events(rxm.rx11b(c, 0), want), (f, rep)
            nok += sum(r["error_code"] == E_OK for r in want)
    assert nok >= 12


def test_rx_model_mode0_equals_the_oracle_at_every_level(o):
    import level_captures as lc
    caps = lc.chain("11b", o)
    n = lc.MAX_EVENTS["11b"]
    assert len(caps) >= 150
    for c in caps:
        assert same_events(rxm.rx11b(c.iq, 0, max_frames=n), o.rx11b_capture(c.iq, max_frames=n)), c.name


def random_long_capture(rng):
    """one to three long-preamble frames of the TX model, any rate, with gaps, gain, DC, noise, sometimes cut short"""
    parts = []
    for _ in range(int(rng.choice([1, 2, 2, 3]))):
        rate = int(rng.choice([1000, 2000, 5500, 11000])); ln = int(rng.choice([1, 5, 14, 20, 60, 150]))
        w, _ = txm.tx11b(rng.integers(0, 256, ln).astype(np.uint8).tobytes(), rate, phase_in=int(rng.integers(0, 4)))
        parts += [np.zeros((int(rng.integers(200, 3000)), 2)), w.astype(np.float64) * float(rng.choice([40, 96, 256]))]
    x = np.concatenate(parts + [np.zeros((int(rng.choice([400, 1600, 2800])), 2))])
    if rng.random() < 0.15:
        x = x[:int(len(x) * rng.uniform(0.3, 0.95))]
    x += rng.uniform(-400, 400, size=(1, 2)) * (rng.random() < 0.3) + rng.normal(0, float(rng.choice([0, 20, 150, 600])), x.shape)
    x = np.clip(np.rint(x), -32768, 32767).astype(np.int16)
    return x[:len(x) // 28 * 28]


def test_rx_model_mode0_equals_the_oracle_on_random_captures(o):
    rng = np.random.default_rng(1102)
    nev = nok = multi = 0
    for i in range(200):
        c = random_long_capture(rng)
        want = o.rx11b_capture(c)
        assert same_events(rxm.rx11b(c, 0), want), i
        nev += len(want); k = sum(r["error_code"] == E_OK for r in want); nok += k; multi += k > 1
    assert nev > 300 and nok > 200 and multi > 50, (nev, nok, multi)


# ------------------------------------------------------------------ the C ABI's additions
def test_abi_surface(sora):
    from sora_amd import capi
    L = sora.load()
    assert L.sora_hip_abi_version() == 4
    txt = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sora_hip.h")).read(), flags=re.S))
    for decl in ("size_t sora_hip_tx11b_pre_samples(uint32_t mpdu_len_nofcs, uint32_t rate_kbps, uint32_t preamble);",
                 "int sora_hip_tx11b_pre(const uint8_t* d_mpdu, const uint32_t* d_off, const uint32_t* d_len, const uint32_t* d_rate_kbps, const uint8_t* d_preamble, "
                 "const uint8_t* d_phase_in, uint8_t* d_phase_out, size_t nframes, int8_t* d_out, const uint64_t* d_out_off, void* stream);",
                 "int sora_rx11b_set_preamble(sora_rx11b_t* rx, int mode);", "#define SORA_ROW_SHORT_PREAMBLE 2u"):
        assert decl in txt, decl
    assert L.sora_hip_tx11b_pre_samples.argtypes == [ctypes.c_uint32] * 3 and L.sora_hip_tx11b_pre_samples.restype is ctypes.c_size_t
    assert L.sora_hip_tx11b_pre.argtypes == [ctypes.c_void_p] * 7 + [ctypes.c_size_t] + [ctypes.c_void_p] * 3
    assert L.sora_rx11b_set_preamble.argtypes == [ctypes.c_void_p, ctypes.c_int]
    assert {"sora_hip_tx11b_pre", "sora_hip_tx11b_pre_samples", "sora_rx11b_set_preamble"} <= set(capi.EXPORTS)
    assert sora.ROW_SHORT_PREAMBLE == 2 == rxm.ROW_SHORT_PREAMBLE
    assert L.sora_rx11b_set_preamble(None, 1) < 0                       # a null handle is refused, not dereferenced


def test_sample_counts(sora):
    L = sora.load()
    per = {2000: 176, 5500: 64, 11000: 32}
    for ln in (1, 2, 3, 13, 14, 64, 257, 1500, 4092):
        for rate, s in per.items():
            assert L.sora_hip_tx11b_pre_samples(ln, rate, 1) == 4224 + (ln + 4) * s + 24 == txm.samples(ln, rate, 1) == sora.tx11b_samples(ln, rate, 1)
        assert L.sora_hip_tx11b_pre_samples(ln, 1000, 1) == 0
        for kind in (2, 7, 255, 0xFFFFFFFF):
            assert L.sora_hip_tx11b_pre_samples(ln, 11000, kind) == 0
        for rate in (1000, 2000, 5500, 11000, 6000):
            assert L.sora_hip_tx11b_pre_samples(ln, rate, 0) == L.sora_hip_tx11b_samples(ln, rate) == sora.tx11b_samples(ln, rate)
    for ln in (0, 4093):
        assert L.sora_hip_tx11b_pre_samples(ln, 11000, 1) == 0


def test_python_wrapper_refuses_before_any_launch(sora):
    for kw in (dict(rates_kbps=[1000], preamble=1), dict(rates_kbps=[2000], preamble=7), dict(rates_kbps=[2000], preamble=[0, 1])):
        with pytest.raises(sora.SoraError):
            sora.tx11b([b"\x01\x02"], **kw)


# ------------------------------------------------------------------ loop-back in the models alone
def loopback_frames(seed, n=300):
    """n short-preamble frames: rates 2000 / 5500 / 11000 in turn, lengths 1..300, as captures (scaled by 96, a lead of 1500..4000 samples, noise of
    sigma <= 20) -> [(mpdu, rate, capture)]"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        rate = (2000, 5500, 11000)[i % 3]; ln = 1 + (i * 7) % 300
        mp = rng.integers(0, 256, ln).astype(np.uint8).tobytes()
        w, _ = txm.tx11b(mp, rate, phase_in=int(rng.integers(0, 4)), preamble=1)
        out.append((mp, rate, rxm.capture(rng, [w], [int(rng.integers(1500, 4001))], float(rng.uniform(0, 20)))))
    return out


@pytest.fixture(scope="module")
def loopback():
    return loopback_frames(LOOPBACK_SEED)


def test_short_frames_decode_at_mode_1(loopback):
    """Condition: at least 95 % of the 300 frames give FRAME_OK with the sent MPDU and the short flag; none gives FRAME_OK with another MPDU."""
    good = wrong = 0
    lengths = set()
    for mp, rate, c in loopback:
        ok = [r for r in rxm.rx11b(c, 1) if r["error_code"] == E_OK]
        for r in ok:
            right = r["mpdu"][:len(mp)] == mp and r["length"] == len(mp) + 4 and r["rate_kbps"] == rate
            wrong += not right
            if right and r["flags"] == rxm.ROW_SHORT_PREAMBLE:
                good += 1; lengths.add(len(mp))
    print("short-preamble loop-back, seed %d: %d of %d frames decoded, %d wrong" % (LOOPBACK_SEED, good, len(loopback), wrong))
    assert wrong == 0 and good >= 0.95 * len(loopback), (good, wrong)
    assert min(lengths) == 1 and max(lengths) >= 295


def test_short_frames_do_not_decode_at_mode_0(o, loopback):
    """the reference's graph knows one SFD: fails without the feature's mode"""
    for k, (mp, rate, c) in enumerate(loopback):
        rows = rxm.rx11b(c, 0)
        assert all(r["error_code"] != E_OK and r["flags"] == 0 for r in rows), k
        if k % 10 == 0:
            assert same_events(rows, o.rx11b_capture(c)), k


# ------------------------------------------------------------------ long and short frames in one capture
def long_key(r, pos="end_sample"):
    """a decoded frame, up to what the stale output buffer leaves in it (PHY_11b.hpp:725-731: the FCS word's top byte and the MPDU's last byte
    are whatever the frame before left there, and that frame differs between the modes); the position apart"""
    return (r["error_code"], r["rate_kbps"], r["length"], r["crc32"] & 0xFFFFFF, r["mpdu"][:-1]), r[pos]


def same_long_rows(got, ref, exact_upto):
    """got: the long frames' rows at mode 1; ref: the decoded rows of the graph that knows the long preamble only (mode 0, the reference) -> the
    number of long frames the latter lost, or -1 if the rows disagree.
    In front of the capture's first short frame (the first exact_upto long frames) the two graphs have seen the same samples in the same state:
    the rows are equal, position included.  Behind a short frame two things differ, and neither is the long frame's decoding.  (i) end_sample is
    the source's position when the harness sees the event, at the end of a 28-sample source call, and the Seek behind every decoded frame
    (fb11b_demod.cpp:47-63) moves the grid of those calls; only mode 1 decodes the short frame, so the grids differ and the positions agree to
    within one call.  (ii) The long-only graph spends the short frame in SFD searches that end 144 symbols after they began, wherever that is: one
    that began late in the short frame runs into the next frame's preamble, and that frame is lost -- to the compiled reference just the same.  So
    there the long-only graph's rows are a subsequence of mode 1's."""
    if got[:exact_upto] != ref[:exact_upto]:
        return -1
    k = exact_upto
    for key, pos in ref[exact_upto:]:
        while k < len(got) and got[k][0] != key:
            k += 1
        if k == len(got) or abs(got[k][1] - pos) >= 28:
            return -1
        k += 1
    return len(got) - len(ref)


def mixed_capture(rng, nframes=4):
    """-> (capture, [(mpdu, rate, kind)]): long and short frames back to back at gaps of 300..3000 samples"""
    waves, leads, sent = [], [], []
    for j in range(nframes):
        kind = int(rng.integers(0, 2))
        rate = int(rng.choice([1000, 2000, 5500, 11000] if kind == 0 else [2000, 5500, 11000])); ln = int(rng.choice([1, 5, 14, 40, 120]))
        mp = rng.integers(0, 256, ln).astype(np.uint8).tobytes()
        w, _ = txm.tx11b(mp, rate, phase_in=int(rng.integers(0, 4)), preamble=kind)
        waves.append(w); leads.append(int(rng.integers(300, 3001)) + (1500 if j == 0 else 0)); sent.append((mp, rate, kind))
    return rxm.capture(rng, waves, leads, float(rng.uniform(0, 20))), sent


def test_mixed_captures(o):
    """Mode 1 reports every frame with its kind's flag.  The long frames' rows are what mode 0 reports for them and -- where it is built -- what the
    compiled reference graph does (same_long_rows says how far "the same" can go behind a short frame): the extension changes nothing for a
    long-preamble frame."""
    g = ReferenceGraph()
    rng = np.random.default_rng(1103)
    nlong = nshort = lost0 = 0
    for i in range(60):
        c, sent = mixed_capture(rng)
        rows1 = rxm.rx11b(c, 1); rows0 = rxm.rx11b(c, 0)
        ok1 = [r for r in rows1 if r["error_code"] == E_OK]
        assert [(r["mpdu"][:-4], r["rate_kbps"], r["flags"]) for r in ok1] == [(mp, rate, 2 * kind) for mp, rate, kind in sent], i
        long1 = [long_key(r) for r in ok1 if r["flags"] == 0]
        first_short = [kind for _, _, kind in sent].index(1) if any(kind for _, _, kind in sent) else len(sent)      # = the long frames in front of it
        lost = same_long_rows(long1, [long_key(r) for r in rows0 if r["error_code"] == E_OK], first_short)
        assert lost >= 0, i
        lost0 += lost
        assert same_events(rows0, o.rx11b_capture(c)), i
        if g.available():
            assert same_long_rows(long1, [long_key(r, "sample_index") for r in g.rx11b(c) if r["error_code"] == E_OK], first_short) == lost, i
        nlong += len(long1); nshort += len(ok1) - len(long1)
    print("mixed captures: %d long and %d short frames decoded at mode 1; the long-only graph lost %d of the long ones behind a short frame" % (nlong, nshort, lost0))
    assert nlong >= 80 and nshort >= 80 and 4 * lost0 < nlong, (nlong, nshort, lost0)
