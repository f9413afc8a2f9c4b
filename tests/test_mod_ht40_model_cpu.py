"""tests/mod_ht40_model.py, the stage-by-stage model of the 40 MHz HT modulation graph, against the three frame models that define the format
(tests/tx_ht40_model.py, ht40_joint_model.py, tx_ht40_gi_model.py): compose() equals them sample for sample on both chains; the interleaver and the parser are
the exact inverses of the receive models' maps.  No GPU, and nothing of the library."""
import numpy as np
import pytest

import ht40_joint_model as J
import mod_ht40_model as M
import tx_ht40_gi_model as G
import tx_ht40_model as T
from oracle import ht40_data_model as dm
from oracle import py_ht40 as m


def _mpdu(tag, n):
    return bytes(np.random.default_rng(tag).integers(0, 256, n).astype(np.uint8))


@pytest.mark.parametrize("length", [5, 200, 1496])
@pytest.mark.parametrize("mcs", range(8, 15))
def test_compose_is_the_frame_models(mcs, length):
    a, b = _mpdu([mcs, length, 0], length), _mpdu([mcs, length, 1], length)
    per = M.compose((a, b), mcs, M.PER_STREAM)
    assert np.array_equal(per, T.frame_int_nofcs(a, b, mcs))
    jnt = M.compose(a, mcs, M.JOINT)
    assert np.array_equal(jnt, J.frame_int_joint_nofcs(a, mcs))
    for gi in (0, 1):
        want = G.frame_int_nofcs((a, b), mcs, gi)
        assert np.array_equal(per if gi == 0 else M.compose((a, b), mcs, M.PER_STREAM, gi), want), gi
        want = G.frame_int_nofcs(a, mcs, gi, joint=True)
        assert np.array_equal(jnt if gi == 0 else M.compose(a, mcs, M.JOINT, gi), want), gi


@pytest.mark.parametrize("seed", [0x00, 0x01, 0x5B, 0xFF])
def test_compose_takes_the_models_seeds(seed):
    mcs, a, b = 12, _mpdu([seed, 0], 61), _mpdu([seed, 1], 61)
    assert np.array_equal(M.compose((a, b), mcs, M.PER_STREAM, 0, (seed, seed ^ 0x36)), T.frame_int_nofcs(a, b, mcs, (seed, seed ^ 0x36)))
    assert np.array_equal(M.compose(a, mcs, M.JOINT, 0, seed), J.frame_int_joint_nofcs(a, mcs, seed))
    assert np.array_equal(M.compose((a, b), mcs, M.PER_STREAM, 1, (seed, seed ^ 0x36)), G.frame_int_nofcs((a, b), mcs, 1, (seed, seed ^ 0x36)))
    assert np.array_equal(M.compose(a, mcs, M.JOINT, 1, seed), G.frame_int_nofcs(a, mcs, 1, seed, joint=True))


@pytest.mark.parametrize("iss", [0, 1])
@pytest.mark.parametrize("nb", [1, 2, 4, 6])
def test_interleave_is_the_inverse_of_the_receive_models_deinterleaver(nb, iss):
    ncb = 108 * nb
    bits = np.random.default_rng([nb, iss]).integers(0, 2, (5, ncb)).astype(np.uint8)
    rows = np.packbits(np.pad(bits, ((0, 0), (0, 8 * M.row_bytes(nb) - ncb))), axis=-1, bitorder="little")
    il = np.unpackbits(M.interleave(rows, nb, iss), axis=-1, bitorder="little")
    assert not il[:, ncb:].any()                                                 # BPSK's last half byte
    d = dm.permutation(nb, iss)                                                  # de-interleaved position k reads interleaved position d[k]
    assert sorted(d) == list(range(ncb))
    assert np.array_equal(il[:, :ncb][:, d], bits)
    assert np.array_equal(M.interleave_stream(np.packbits(bits.reshape(-1), bitorder="little"), 5, nb, iss), M.interleave(rows, nb, iss))


@pytest.mark.parametrize("nb", [1, 2, 4, 6])
def test_stream_parse_is_the_inverse_of_deparse(nb):
    ncb = 108 * nb
    bits = np.random.default_rng(nb).integers(0, 2, (3, 2 * ncb)).astype(np.uint8)
    p0, p1 = M.stream_parse(np.packbits(bits, axis=-1, bitorder="little"), nb)
    b0, b1 = (np.unpackbits(p, axis=-1, bitorder="little") for p in (p0, p1))
    assert not b0[:, ncb:].any() and not b1[:, ncb:].any()
    assert np.array_equal(J.deparse(b0[:, :ncb].reshape(-1), b1[:, :ncb].reshape(-1), nb), bits.reshape(-1))


def test_the_scrambler_stage_expresses_the_models_seed_and_tail():
    """T11aSc from register bitrev7(seed) << 1 is py_ht40.scramble_seq(seed); its TAIL_SCRAMBLE byte is the six zeroed tail bits"""
    import mod11a_model as A
    for seed in (0x00, 0x01, 0x5B, 0x5D, 0x7F, 0xFF):
        got = np.unpackbits(A.scramble(np.zeros(40, np.uint8), M.stage_seed(seed)), bitorder="little")
        assert np.array_equal(got, m.scramble_seq(seed & 0x7F, 320)), seed
    psdu = m.add_fcs(_mpdu(7, 9))
    want = m.stream_bits(psdu, 3, 2, 0, 0x5D)                                    # MCS 9: 108 bits per symbol
    sig, data, nbytes, tail, regs, nsym = M.fields((psdu[:-4], psdu[:-4]), 9)
    assert nsym == 2 and tail == 2 + len(psdu)
    got = np.unpackbits(A.scramble(data[0][:nbytes], regs[0], tail), bitorder="little")
    assert np.array_equal(got[:nsym * 108], want[:nsym * 108])
