"""tests/mod11b_model.py, the per-brick models of the 802.11b modulation graph, on the CPU: composed they are tests/tx11b_model.py (which the compiled reference
modulator and the recorded waveforms pin) sample for sample and last_phase for last_phase; each stateful model cut anywhere equals itself uncut; the shaper's
whole-array form is the brick's loop from any record and any COMPLEX8."""
import numpy as np
import pytest

import mod11b_model as M
import tx11b_model as txm
from oracle.pyoracle import ReferenceGraph

RATES = (1000, 2000, 5500, 11000)


def frames():
    for kind in (0, 1):
        for rate in RATES:
            if txm.samples(1, rate, kind):
                yield rate, kind


@pytest.mark.parametrize("ln", [1, 2, 37, 1500, 4092])
def test_the_models_composed_are_the_whole_frame_model(ln):
    for rate, kind in frames():
        mp = np.random.default_rng([ln, rate, kind]).integers(0, 256, ln).astype(np.uint8).tobytes()
        for phase_in in range(4):
            got, phase = M.mod11b(mp, rate, phase_in, kind)
            want, wphase = txm.tx11b(mp, rate, phase_in, kind)
            assert got.dtype == want.dtype and np.array_equal(got, want), (rate, kind, ln, phase_in)
            assert phase == wphase, (rate, kind, ln, phase_in)


def test_the_models_composed_are_the_compiled_reference_modulator():
    from test_tx11b_cpu import ref_tx11b, start_parity
    g = ReferenceGraph()
    if not g.available():
        pytest.skip("oracle/_ref/libsora_refgraph.so not built (needs the reference tree)")
    rng = np.random.default_rng(1201)
    phase = None
    for ln in (1, 2, 37, 1500, 4092):
        for rate in RATES:
            mp = rng.integers(0, 256, ln).astype(np.uint8).tobytes()
            want = ref_tx11b(g, mp, rate)
            if phase is None:
                phase = 3 * start_parity(want)                                   # (what this process modulated before: only the low bit shows, and only it matters)
            assert phase & 1 == start_parity(want), (rate, ln)
            got, phase = M.mod11b(mp, rate, phase, 0)
            assert np.array_equal(got, want), (rate, ln)


def test_ppdu_is_the_whole_frame_models():
    for rate, kind in frames():
        for ln in (1, 2, 13, 14, 37, 1500, 4092):
            mp = bytes(np.random.default_rng(ln).integers(0, 256, ln).astype(np.uint8))
            assert M.ppdu(mp, rate, kind) == txm.ppdu_bytes(mp, rate, kind), (rate, kind, ln)


STREAM = bytes(np.random.default_rng(70).integers(0, 256, 70).astype(np.uint8))


@pytest.mark.parametrize("brick", ["sc741", "dbpsk", "dqpsk", "cck5", "cck11"])
def test_a_stream_cut_anywhere_is_the_stream_uncut(brick):
    fn = {"sc741": M.sc741, "dbpsk": M.dbpsk_spread, "dqpsk": M.dqpsk_spread, "cck5": M.cck5_encode, "cck11": M.cck11_encode}[brick]
    for state in {"sc741": [(0x6C,), (0x1B,), (0,), (0x7F,)], "cck11": [(p, e) for p in range(4) for e in (0, 1)]}.get(brick, [(p,) for p in range(4)]):
        whole = fn(STREAM, *state)
        for cut in range(len(STREAM) + 1):
            a = fn(STREAM[:cut], *state)
            b = fn(STREAM[cut:], *a[1:])
            assert b[1:] == whole[1:], (brick, state, cut)
            assert np.array_equal(np.concatenate([np.frombuffer(a[0], np.uint8), np.frombuffer(b[0], np.uint8)]) if brick == "sc741" else np.concatenate([a[0], b[0]]),
                                  np.frombuffer(whole[0], np.uint8) if brick == "sc741" else whole[0]), (brick, state, cut)


def test_sc741_is_the_whole_frame_models_and_reads_seven_bits():
    for reg in (0x6C, 0x1B, 0x00, 0x7F):
        assert M.sc741(STREAM, reg)[0] == txm.sc741(STREAM, reg)
        assert M.sc741(STREAM, reg | 0x80) == M.sc741(STREAM, reg)


def test_dbpsk_reads_one_bit_and_leaves_0_or_3():
    for p in range(4):
        out, last = M.dbpsk_spread(STREAM, p)
        ref, rlast = M.dbpsk_spread(STREAM, 3 * (p & 1))
        assert np.array_equal(out, ref) and last == rlast and last in (0, 3)


def shaper_cases():
    rng = np.random.default_rng(1203)
    unit = np.array([(1, 0), (0, 1), (-1, 0), (0, -1)], np.int8)[rng.integers(0, 4, 70)]
    full = rng.integers(-128, 128, (70, 2)).astype(np.int8); full[3] = (-128, 127); full[40] = (127, -128)
    zero = np.zeros((4, 4, 2), np.int16)
    left = M.quick_shape_loop(full[:9], zero)[1]
    rand = rng.integers(-32768, 32768, (4, 4, 2)).astype(np.int16)
    return [(x, s) for x in (unit, full) for s in (zero, left, rand)]


def test_the_shaper_in_whole_arrays_is_the_bricks_loop():
    for x, temps in shaper_cases():
        for n in (0, 1, 2, 3, 4, 5, 6, 70):
            for flush in (False, True):
                a, sa = M.pulse_shape(x[:n], temps, flush)
                b, sb = M.quick_shape_loop(x[:n], temps, flush)
                assert a.shape == (4 * (n + 5 * flush), 2) and np.array_equal(a, b) and np.array_equal(sa, sb), (n, flush)


def test_the_shaper_cut_anywhere_is_the_shaper_uncut():
    for x, temps in shaper_cases():
        whole, sw = M.pulse_shape(x, temps, True)
        for cut in range(len(x) + 1):
            a, sa = M.pulse_shape(x[:cut], temps)
            b, sb = M.pulse_shape(x[cut:], sa, True)
            assert np.array_equal(np.concatenate([a, b]), whole) and np.array_equal(sb, sw), cut
        assert not sw.any()                                                      # (Flush pushes everything out)
