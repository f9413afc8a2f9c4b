"""802.11b transmitter (sora_hip_tx11b), the parts that need no GPU: the sample count against the recorded frames of the reference
modulator and, where oracle/_ref is built, against the live one; the refusals; the C entry point failing loudly without a device;
the shaper taps the kernel compiles in; and a numpy restatement of the whole transmitter (the kernel's recipe: scrambler, differential
phase in quarter turns, Barker and CCK chip angles, five-chip shaper windows) that reproduces all 12 recordings sample for sample,
the reference's phase carry-over from frame to frame included."""
import ctypes
import os
import re
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
# tests/golden/make_golden.py: the frames of each recording and the seed of their MPDUs (one generator, in this order)
RECORDINGS = [("refgraph_11b.npz", 1102, [(1000, 1), (1000, 14), (1000, 40), (2000, 5), (2000, 60), (2000, 200)]),
              ("refgraph_11b_cck.npz", 1103, [(5500, 1), (5500, 30), (5500, 200), (11000, 2), (11000, 77), (11000, 400)])]
PER_BYTE = {1000: 352, 2000: 176, 5500: 64, 11000: 32}


@pytest.fixture(scope="module")
def sora():
    import sora_amd
    sora_amd.load()
    return sora_amd


def recorded_frames():
    """-> [(name, k, rate, mpdu, samples)] for the 12 recorded frames, MPDUs regenerated from their seeds."""
    out = []
    for name, seed, cases in RECORDINGS:
        z = np.load(os.path.join(GOLD, name))
        rng = np.random.default_rng(seed)
        for k, (rate, ln) in enumerate(cases):
            out.append((name, k, rate, rng.integers(0, 256, ln).astype(np.uint8).tobytes(), z["tx_%d" % k]))
    return out


def start_parity(samples):
    """The low bit of last_phase a recorded frame started from: the preamble comes out as W (sample 6 = +31) or as -W."""
    assert abs(int(samples[6, 0])) == 31 and samples[6, 1] == 0
    return 0 if samples[6, 0] > 0 else 1


def formula(ln, rate):
    return 192 * 44 + (ln + 4) * PER_BYTE[rate] + 24


def ref_tx11b(g, mpdu, rate):
    """The live reference modulator with an output buffer sized from the formula: TModSink does not bound its writes, and
    ReferenceGraph.tx11b's 2^20 samples are too few for 1 Mbps frames longer than 2951 bytes."""
    a = np.frombuffer(bytes(mpdu), np.uint8)
    cap = formula(len(a), rate) + 64
    o = np.zeros((cap, 2), np.int8)
    n = g.L.ref_tx11b(a.ctypes.data_as(ctypes.c_void_p), len(a), rate, o.ctypes.data_as(ctypes.c_void_p), cap)
    assert 0 < n <= cap - 64, n
    return o[:n]


def test_regenerated_mpdus_are_the_recorded_ones():
    """The first frame the reference receiver decoded correctly from each recording carries the regenerated MPDU."""
    frames = iter(recorded_frames())
    for name, _, cases in RECORDINGS:
        z = np.load(os.path.join(GOLD, name))
        cnt, err = z["ev_count"], z["ev_error"]
        ev = 0
        for k in range(len(cases)):
            _, _, _, mp, _ = next(frames)
            n = int(cnt[3 * k:3 * k + 3].sum())
            good = [e for e in range(ev, ev + n) if err[e] == 0x1]
            assert good, (name, k)
            got = z["mpdu_%d" % good[0]].tobytes()
            assert len(got) == len(mp) + 4 and got[:len(mp)] == mp, (name, k)          # (FRAME_OK: the FCS checked out)
            ev += n


def test_sample_count_matches_the_recorded_frames(sora):
    for name, k, rate, mp, s in recorded_frames():
        assert sora.tx11b_samples(len(mp), rate) == len(s) == formula(len(mp), rate), (name, k)


def length_extension(ln):
    size = ln + 4
    us = (size * 8 + 10) // 11
    return us * 11 - size * 8 >= 8


def test_sample_count_equals_the_formula(sora):
    ext = [ln for ln in range(1, 200) if length_extension(ln)]
    assert ext[:4] == [3, 6, 10, 14], ext[:4]                       # 11 Mbps lengths whose SERVICE carries the length-extension bit
    for rate in PER_BYTE:
        for ln in list(range(1, 64)) + ext + [1500, 2951, 2952, 4091, 4092]:
            assert sora.tx11b_samples(ln, rate) == formula(ln, rate), (rate, ln)


def sweep_lengths():
    return [1, 2, 3, 4, 5, 7, 10, 11, 15, 37, 100, 255, 256, 1000, 1500, 2951, 2952, 3000, 4091, 4092]


def test_sample_count_equals_the_reference_modulator(sora):
    from oracle.pyoracle import ReferenceGraph
    g = ReferenceGraph()
    if not g.available():
        pytest.skip("oracle/_ref/libsora_refgraph.so not built (needs the reference tree)")
    for rate in PER_BYTE:
        for ln in sweep_lengths():
            assert sora.tx11b_samples(ln, rate) == len(ref_tx11b(g, bytes(ln), rate)), (rate, ln)


@pytest.mark.parametrize("rate,ln", [(r, 100) for r in (0, 1, 5000, 6000, 5501, 22000, 54000)] +
                         [(r, l) for r in (1000, 2000, 5500, 11000) for l in (0, 4093, 65535)])
def test_unsupported_frames_give_zero_samples(sora, rate, ln):
    assert sora.tx11b_samples(ln, rate) == 0


def test_python_wrapper_refuses_an_unsupported_frame_before_any_launch(sora):
    with pytest.raises(sora.SoraError):
        sora.tx11b([b"\x01\x02\x03"], [6000])
    with pytest.raises(sora.SoraError):
        sora.tx11b([b"\x01", b"\x02"], [1000, 5000])
    with pytest.raises(sora.SoraError):
        sora.tx11b([b""], [11000])
    with pytest.raises(sora.SoraError):
        sora.tx11b([b"\x01"], [1000], phase_in=[4])


def test_entry_point_refuses_without_a_device(sora):
    if sora.device_count() > 0:
        pytest.skip("a HIP device is present")
    L = sora.load()
    p = ctypes.c_void_p(16)
    assert L.sora_hip_tx11b(p, p, p, p, None, None, 1, p, p, None) == -5
    assert b"no HIP device" in L.sora_hip_last_error()


def taps_formula():
    """TQuickPulseShaper's taps for i = 8 .. -11: (short)(x * 80 + .5), x = 4 cos(PI i / 2) / PI / (1 - i^2), 1 at i = +-1, PI = 3.141593;
    the cast truncates toward zero."""
    PI = 3.141593
    i = np.arange(8, -12, -1).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        x = 4 * np.cos(PI * i / 2) / PI / (1 - i * i)
    x[np.abs(i) == 1] = 1.0
    return np.trunc(x * 80 + .5).astype(np.int64)


def test_kernel_taps_equal_the_formula():
    src = open(os.path.join(ROOT, "sora_amd", "csrc", "k_tx11b.hip")).read()
    m = re.search(r"kTx11bTaps\[20\]\s*=\s*\{([^}]*)\}", src)
    assert m, "kTx11bTaps not found"
    got = np.array([int(v) for v in m.group(1).split(",")], np.int64)
    want = taps_formula()
    assert np.array_equal(got, want), (got.tolist(), want.tolist())
    assert want.tolist() == [-1, 0, 3, 0, -6, 0, 34, 80, 102, 80, 34, 0, -6, 0, 3, 0, -1, 0, 1, 0]


# ---- the recipe, in numpy
DQ = [0, 3, 1, 2]                   # quarter turns of a DQPSK dibit d0 + 2 d1 (and of CCK's phi1 increment)
CQ = [0, 2, 1, 3]                   # quarter turns of a CCK 11 phi2..phi4 dibit
BARKER_NEG = [0, 1, 0, 0, 1, 0, 0, 0, 1, 1, 1]
CODE = {1000: 0x0A, 2000: 0x14, 5500: 0x37, 11000: 0x6E}


def crc16(b):
    c = 0xFFFF
    for x in b:
        c ^= x
        for _ in range(8):
            c = (c >> 1) ^ 0x8408 if c & 1 else c >> 1
    return ~c & 0xFFFF


def ppdu(mpdu, rate):
    size = len(mpdu) + 4
    us = {1000: size * 8, 2000: size * 4, 5500: (size * 16 + 10) // 11, 11000: (size * 8 + 10) // 11}[rate]
    ext = int(rate == 11000 and length_extension(len(mpdu)))
    h = bytes([CODE[rate], ext << 7, us & 0xFF, us >> 8])
    c = crc16(h)
    return bytes([0xFF] * 16 + [0xA0, 0xF3]) + h + bytes([c & 0xFF, c >> 8]) + bytes(mpdu) + zlib.crc32(bytes(mpdu)).to_bytes(4, "little")


def scramble(data, reg=0x6C):
    out = []
    for x in data:
        o = 0
        for k in range(8):
            b = ((x >> k) ^ reg ^ (reg >> 3)) & 1
            reg = (reg >> 1) | (b << 6)
            o |= b << k
        out.append(o)
    return out


def recipe(mpdu, rate, phase_in=0):
    """-> (int8 [n, 2] COMPLEX8 @44 MHz, last_phase after the frame)."""
    phi = 2 * (phase_in & 1)
    a = []
    for k, v in enumerate(scramble(ppdu(mpdu, rate))):
        if k < 24 or rate == 1000:
            for i in range(8):
                phi = (phi + 2 * ((v >> i) & 1)) % 4
                a += [(phi + 2 * n) % 4 for n in BARKER_NEG]
        elif rate == 2000:
            for i in range(4):
                phi = (phi + DQ[(v >> 2 * i) & 3]) % 4
                a += [(phi + 2 * n) % 4 for n in BARKER_NEG]
        else:
            d = k - 24
            for w, odd in ([(v & 15, 0), (v >> 4, 1)] if rate == 5500 else [(v, d & 1)]):
                phi = (phi + DQ[w & 3] + 2 * odd) % 4
                if rate == 5500:
                    p2, p3, p4 = 1 + 2 * ((w >> 2) & 1), 0, 2 * ((w >> 3) & 1)
                else:
                    p2, p3, p4 = CQ[(w >> 2) & 3], CQ[(w >> 4) & 3], CQ[(w >> 6) & 3]
                a += [(phi + o) % 4 for o in (p2 + p3 + p4, p3 + p4, p2 + p4, p4 + 2, p2 + p3, p3, p2 + 2, 0)]
    a = np.array(a)
    x = np.array([1, 1j, -1, -1j])[a]
    n = len(x)
    xp = np.concatenate([np.zeros(4), x, np.zeros(6)])
    taps = taps_formula()
    y = np.zeros((n + 6, 4), complex)
    for s in range(4):
        for j in range(5):
            y[:, s] += xp[4 - j:4 - j + n + 6] * taps[4 * j + s]
    y = y.ravel()
    out = np.clip(np.stack([np.rint(y.real), np.rint(y.imag)], 1), -128, 127).astype(np.int8)
    return out, [0, 2, 3, 1][phi]


def test_recipe_reproduces_the_recorded_frames_and_the_phase_carry_over():
    """Each recording is one reference process: frame k + 1 starts from the last_phase frame k left behind."""
    frames = recorded_frames()
    parity = None
    for name, k, rate, mp, s in frames:
        p = start_parity(s)
        if k > 0:
            assert p == parity, (name, k)
        got, last = recipe(mp, rate, p)
        assert np.array_equal(got, s), (name, k)
        parity = last & 1
    assert [start_parity(s) for *_, s in frames] == [0] * 10 + [1, 0]       # frame 4 of the CCK recording starts at pi
