"""TUpsample40MTo44M in closed form (Brick11/src/sampling.hpp:8-32, 40MTo44M.hpp), and an 802.11a frame at 44 MHz made from
one at 40 MHz.  A helper of tests/test_tx11a44_cpu.py, tests/test_gpu_tx11a44.py and tests/golden/make_reftx11a_44.py, not a test.

The brick turns each 160-sample block x of 16-bit samples into 176 samples y and carries nothing from block to block.
For I and Q apart, j = 11 m + r, r = 0..10, m = 0..15:
    mh(a, c) = (a * c + 16384) >> 15                                    (_mm_mulhrs_epi16)
    S(k)     = floor(k * 32767 / 11),  S(0) = 0,  S(11) = 32767
    y[j]     = int16(mh(x[j - m - 1], S(r)) + mh(x[j - m], S(11 - r)))
y[175] needs x[160].  The reference loads it from behind its input block (40MTo44M.hpp:112): the preamble's blocks 0..2 find the
next block's first sample there (the source hands all 640 samples on as one burst); block 3, the SIGNAL symbol and every data
symbol find whatever memory follows the pin queue's buffer.  The rule here, and in sora_hip_tx11a44: x[160] = 0 for those.
So sample 176 j + 175, j >= 3, of a frame is not compared with a recorded reference stream (`excluded`)."""
import numpy as np

S = np.array([k * 32767 // 11 for k in range(12)], np.int32)
_J = np.arange(176)
_M = _J // 11
_R = _J - 11 * _M
_HI = _J - _M                                          # 0..160
_LO = np.maximum(_HI - 1, 0)                           # (weight S(0) = 0 where j - m - 1 < 0)


def _mh(a, c):
    return (a.astype(np.int32) * c + 16384) >> 15


def up40to44(x16, sees_next):
    """x16: int16 [160 n, 2]; sees_next[b]: block b finds the next block's first sample behind its own last one (else 0).  -> int16 [176 n, 2]"""
    x = np.ascontiguousarray(x16, np.int16).reshape(-1, 160, 2)
    nb = len(x)
    xe = np.zeros((nb, 161, 2), np.int16)
    xe[:, :160] = x
    for b in range(nb - 1):
        if sees_next[b]:
            xe[b, 160] = x[b + 1, 0]
    y = _mh(xe[:, _LO], S[_R][None, :, None]) + _mh(xe[:, _HI], S[11 - _R][None, :, None])
    return y.astype(np.int16).reshape(-1, 2)           # (wraps like the brick's 16-bit add)


def sat8(y16):
    return np.clip(y16, -128, 127).astype(np.int8)     # _mm_packs_epi16 (TPackSample16to8)


def frame44(x16):
    """A whole frame (640-sample preamble, SIGNAL, data symbols) of 16-bit samples at 40 MHz -> COMPLEX8 at 44 MHz."""
    nb = len(x16) // 160
    assert len(x16) == 160 * nb and nb >= 5
    return sat8(up40to44(x16, [b < 3 for b in range(nb)]))


def has_rail(tx40):
    return bool(((tx40 == 127) | (tx40 == -128)).any())


def frame44_from_tx40(tx40, allow_rails=False):
    """From the COMPLEX8 stream at 40 MHz.  Exact only where no sample of it sits at a rail -- there the 8-bit value IS the 16-bit one the
    brick saw; allow_rails: the byte-fed model of a frame that has such samples, which is NOT what the reference sends (the brick runs
    in front of the pack)."""
    assert allow_rails or not has_rail(tx40), "a sample at the int8 rail: the 16-bit stream cannot be told from the bytes"
    return frame44(np.asarray(tx40).astype(np.int16))


def excluded(nsamples44):
    """Indices of a frame's 44 MHz samples where the reference read behind its input: 176 j + 175 for j >= 3 (nblocks - 3 of them)."""
    nb = nsamples44 // 176
    return 176 * np.arange(3, nb) + 175


def compared(nsamples44):
    keep = np.ones(nsamples44, bool)
    keep[excluded(nsamples44)] = False
    return keep


def capture44(tx44, tail=440):
    """`demod11 -c`'s expansion (COMPLEX8 << 8) of one frame at 44 MHz with `tail` samples of silence behind it, cut to whole 28-sample bursts."""
    seg = np.concatenate([np.asarray(tx44).astype(np.int16) << 8, np.zeros((tail, 2), np.int16)])
    return seg[:len(seg) // 28 * 28]


def rail_free_seed(oracle, mpdu, rate, first):
    """The first scrambler seed from `first` on (mod 256) with which the oracle's 40 MHz frame has no sample at a rail: frames on which
    frame44_from_tx40 is exact are chosen on the CPU, none is skipped.  (Seeds 0 and 1 -- the all-zero scrambler -- always reach a rail.)"""
    for k in range(256):
        seed = (first + k) & 255
        if not has_rail(oracle.tx(mpdu, rate, seed)):
            return seed
    raise AssertionError("no rail-free seed")
