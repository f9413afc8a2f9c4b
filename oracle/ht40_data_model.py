"""ht40_data_model.py -- TEST INFRASTRUCTURE.  An INTEGER model of the data field of a 40 MHz HT two-stream frame as sora_ht40_process_dev is asked to
decode it, from the detection weights on.  **Parity unpinned** as a whole -- the reference has no 40 MHz receive graph -- but nothing in it is new arithmetic:

  * every operation is one of the oracle's bricks, each held bit for bit to the compiled reference elsewhere (oracle/so_11n.c, so_dsp.c, so_rx11a.c):
    so_freq_comp11n (TFreqComp_11n), so_fft128 (FFT<128>), TMimoChannelEst's / TMimoChannelComp's per-carrier arithmetic, so_dsp_atan16 (dsp_math),
    T11nDemap*'s tables, so_viterbi_frame_ex(.., 192, 36) (T11aViterbi<.., 192, 36>), so_desc_sink (T11aDesc + TBB11aFrameSink);
  * the glue between them is what DESIGN.md section 7 g1 and oracle/py_ht40.py state, and is taken FROM py_ht40 (one statement of the format): the 40 MHz
    carrier plan (108 data carriers in demapping order, six pilots per stream sent as +1), the HT-LTF signs, the HT interleaver (N_COL 18, N_ROT 29);
  * per data symbol d: the 160 samples at offset + 320 + 160 d; TFreqComp_11n at phase n cfo - theta (n counts from the frame's first sample; the cyclic
    prefix is counted but dropped); FFT<128> per chain; x_s = sat((W y) >> 9); theta += ((sum of stream 0's six pilot arctangents / 6) + (stream 1's)) >> 1,
    C truncation, every step cast through int16, effective from the NEXT symbol; demapping I bits then Q bits; de-interleaving; then per stream the trellis
    and the descrambler / FCS sink.

The weights are an INPUT (the GPU's exported ones in tests/test_gpu_ht40_soft.py): the MMSE solve is single-precision float arithmetic with its own stated
tolerance.  zf_weights() is the zero-forcing case, where the weights are TMimoChannelEst's own and the model computes them itself, bit for bit.
tests/test_ht40_data_model.py holds this model to the numpy model of the format (it recovers what py_ht40 transmits), so that it is not an echo of the kernel."""
import ctypes

import numpy as np

from . import py_ht40 as m
from . import pyoracle

_P = pyoracle._P
DATA_BINS = np.array([m.bin_of(k) for k in m.DATA_CARRIERS], np.int16)
PILOT_BINS = np.array([m.bin_of(k) for k in m.PILOTS], np.int16)
LTF_SIGN = np.zeros(128, np.int8)
for _k in range(-58, 59):
    LTF_SIGN[m.bin_of(_k)] = m.HTLTF40[_k + 58]
OCCUPIED_BINS = np.array([m.bin_of(k) for k in range(-58, 59) if m.HTLTF40[k + 58] != 0], np.int16)            # 114
assert len(OCCUPIED_BINS) == 114

_oracle = None


def oracle():
    global _oracle
    if _oracle is None:
        _oracle = pyoracle.Oracle()
    return _oracle


def permutation(nbpsc, iss):
    """de-interleaver of spatial stream iss: output bit k of a symbol is demapped bit permutation(..)[k]"""
    return np.asarray(m.interleave_map(nbpsc, iss), np.uint16)


class Stream:
    """one spatial stream's decode: error_code (FRAME_OK / CRC32_FAIL), crc32 (the FCS as found in the frame), psdu (the bytes the sink leaves)"""
    def __init__(self, error_code, crc32, psdu):
        self.error_code, self.crc32, self.psdu = error_code, crc32, psdu


class Result:
    def __init__(self, soft, theta, xs, streams, nsym):
        self.soft, self.theta, self.xs, self.streams, self.nsym = soft, theta, xs, streams, nsym


def _frame(iq, offset, nsym):
    iq = np.asarray(iq)
    assert iq.dtype == np.int16 and iq.ndim == 3 and iq.shape[0] == 2 and iq.shape[2] == 2
    n = (2 + nsym) * 160
    assert 0 <= offset and offset + n <= iq.shape[1], "the frame does not lie inside the capture"
    return np.ascontiguousarray(iq[0, offset:offset + n]), np.ascontiguousarray(iq[1, offset:offset + n])


def zf_weights(iq, offset, cfo):
    """TMimoChannelEst's zero-forcing inverse x 2^16 from the two HT-LTF symbols -> int16 [4, 128, 2] (w00, w01, w10, w11 per bin).  Only the 114 occupied
    carriers (OCCUPIED_BINS) mean anything."""
    a, b = _frame(iq, offset, 0)
    w = np.zeros((4, 128, 2), np.int16)
    oracle().L.so_ht40_zf_weights(_P(a), _P(b), ctypes.c_int32(int(cfo)), _P(LTF_SIGN), _P(w))
    return w


def model(iq, offset, n_bpsc, code_rate, length, cfo, weights, decode=True):
    """iq int16 [2, n, 2]; offset: first sample (cyclic prefix) of HT-LTF 1; length: PSDU bytes of the two streams; cfo: the descriptor's phase step;
    weights int16 [4, 128, 2].  -> Result: soft[2] uint8 [nsym * 108 * n_bpsc], theta int16 [nsym + 1] (theta[d] compensates symbol d; the last entry is
    the phase after the last symbol), xs int16 [nsym, 2, 128, 2] (the detected symbols), streams[2] (Stream; None with decode=False)."""
    nsym = m.nsym_for(list(length), n_bpsc, code_rate)
    a, b = _frame(iq, offset, nsym)
    w = np.ascontiguousarray(weights, np.int16).reshape(4, 128, 2)
    per = nsym * 108 * n_bpsc
    soft = [np.zeros(per, np.uint8), np.zeros(per, np.uint8)]
    theta = np.zeros(nsym + 1, np.int16); xs = np.zeros((nsym, 2, 128, 2), np.int16)
    d0, d1 = permutation(n_bpsc, 0), permutation(n_bpsc, 1)
    O = oracle()
    n = O.L.so_ht40_data_field(_P(a), _P(b), ctypes.c_uint32(nsym), int(n_bpsc), ctypes.c_int32(int(cfo)), _P(w), _P(DATA_BINS), len(DATA_BINS),
                               _P(PILOT_BINS), len(PILOT_BINS), _P(d0), _P(d1), _P(soft[0]), _P(soft[1]), _P(theta), _P(xs))
    assert n == per, n
    streams = [None, None]
    if decode:
        for s in range(2):
            dec = O.viterbi_frame_ex(soft[s], code_rate, int(length[s]), 192, 36)
            e, psdu, crc = O.desc_sink(dec, int(length[s]))
            streams[s] = Stream(e & 0xFFFFFFFF, crc, psdu.tobytes())
    return Result(soft, theta, xs, streams, nsym)
