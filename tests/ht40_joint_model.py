"""ht40_joint_model.py -- TEST INFRASTRUCTURE: the JOINT coding of the 40 MHz HT 2x2 pair (sora_hip_tx_ht40_joint, sora_ht40_set_coding).

The format is oracle/py_ht40.py::tx_frame's, except that a frame carries ONE PSDU of LENGTH <= 4000 bytes:
  * bit field: SERVICE(16) + PSDU + tail(6) + pad up to N_SYM x N_DBPS bits, N_DBPS = 2 x 108 x N_BPSC x R, N_SYM = ceil((16 + 8 LENGTH + 6) / N_DBPS);
  * one scrambler (one seed, seven bits used, default 0x5D; the tail forced to zero after scrambling), one K = 7 encoder, the same three puncturing patterns;
  * the stream parser of the reference's 802.11n modulator: with s = max(1, N_BPSC / 2), coded bit kc (0 .. 2 N_CBPSS - 1) of a symbol goes to spatial stream
    (kc / s) & 1 and becomes that stream's bit (kc / 2s) s + kc % s;
  * from there on nothing differs: each stream's HT interleaver (py_ht40.interleave_map), mapper, carrier plan, pilots, HT-LTFs, preamble, HT-SIG bits.
Three models, all from pieces that exist: the float frame (tx_joint, tx_frame_joint) from py_ht40's; the integer frame (frame_int_joint) from tests/tx_ht40_model.py's
helpers; the integer receive model (rx_model) from oracle/ht40_data_model.py's per-stream soft bytes, de-parsed into one stream, decoded by the oracle's
T11aViterbi<.., 192, 36> and finished by its descrambler / FCS sink.  Nothing here imports the library under test."""
import ctypes

import numpy as np

from oracle import ht40_data_model as dm
from oracle import py_ht40 as m
import tx_ht40_model as T

SEED = 0x5D


def ndbps(nbpsc, code_rate):
    return 2 * m.ndbps(nbpsc, code_rate)


def nsym_for(length, nbpsc, code_rate):
    return -(-(16 + 8 * int(length) + 6) // ndbps(nbpsc, code_rate))


def parser_map(nbpsc):
    """-> (iss, k) int arrays over kc = 0 .. 2 N_CBPSS - 1: coded bit kc of a symbol is bit k of spatial stream iss"""
    s = max(1, nbpsc // 2)
    kc = np.arange(216 * nbpsc)
    return (kc // s) & 1, (kc // (2 * s)) * s + kc % s


def field_bits(psdu_with_fcs, nsym, nbpsc, code_rate, seed=SEED):
    n = nsym * ndbps(nbpsc, code_rate)
    data = np.zeros(n, np.uint8)
    payload = np.unpackbits(np.frombuffer(psdu_with_fcs, np.uint8), bitorder="little")
    data[16:16 + len(payload)] = payload
    scr = data ^ m.scramble_seq(seed & 0x7F, n)
    scr[16 + len(payload):16 + len(payload) + 6] = 0             # tail
    return scr


def stream_symbols(psdu_with_fcs, nbpsc, code_rate, seed=SEED):
    """-> uint8 [2 streams, nsym, N_CBPSS]: each stream's INTERLEAVED bits of every symbol (what its mapper takes)"""
    nsym = nsym_for(len(psdu_with_fcs), nbpsc, code_rate)
    a, b = m.encode(field_bits(psdu_with_fcs, nsym, nbpsc, code_rate, seed))
    coded = m.puncture(a, b, code_rate)
    ncb = 108 * nbpsc
    assert len(coded) == nsym * 2 * ncb
    iss, k = parser_map(nbpsc)
    out = np.zeros((2, nsym, ncb), np.uint8)
    imaps = [m.interleave_map(nbpsc, s) for s in range(2)]
    for d in range(nsym):
        blk = coded[d * 2 * ncb:(d + 1) * 2 * ncb]
        for s in range(2):
            st = np.zeros(ncb, np.uint8); st[k[iss == s]] = blk[iss == s]
            out[s, d, imaps[s]] = st
    return out


# ------------------------------------------------------------------ the float frame
def tx_joint(psdu_with_fcs, nbpsc, code_rate, seed=SEED):
    """as py_ht40.tx: complex128 [2, (2 + nsym) * 160] (HT-LTF x 2, then data), nsym"""
    il = stream_symbols(psdu_with_fcs, nbpsc, code_rate, seed)
    nsym = il.shape[1]
    X = np.zeros((2, 2 + nsym, 128), complex)
    for k in range(-58, 59):
        v = m.HTLTF40[k + 58]
        X[0, 0, m.bin_of(k)] = v;  X[0, 1, m.bin_of(k)] = -v       # P = [[1, -1], [1, 1]]
        X[1, 0, m.bin_of(k)] = v;  X[1, 1, m.bin_of(k)] = v
    car = [m.bin_of(k) for k in m.DATA_CARRIERS]
    pil = [m.bin_of(k) for k in m.PILOTS]
    for s in range(2):
        for d in range(nsym):
            X[s, 2 + d, car] = m.qam(il[s, d].astype(float), nbpsc) / 128.0
            X[s, 2 + d, pil] = (m.LEVEL[1] / 128.0) * 2.0
    x = np.fft.ifft(X, axis=2) * 128.0
    x = np.concatenate([x[:, :, -32:], x], axis=2)
    return x.reshape(2, -1), nsym


def _preamble_float(mcs, ht_length, nsym):
    """py_ht40.tx_frame's legacy part, HT-SIG and HT-STF for a frame of nsym data symbols -> complex128 [1280]"""
    l_length = max(1, -(-(36 + 4 * nsym + 4 - 20) // 4) * 3 - 3)
    stf = np.fft.ifft(m._dup40(m._STF)) * 128.0
    ltf = np.fft.ifft(m._dup40(m._LTF)) * 128.0
    parts = [np.tile(stf, 3)[:320], np.concatenate([ltf[-64:], ltf, ltf])]
    a, b = m.encode(m.l_sig_bits(l_length))
    sym = np.fft.ifft(m._dup40(m._leg_symbol(np.stack([a, b], 1).reshape(-1), False, 1.0))) * 128.0
    parts.append(np.concatenate([sym[-32:], sym]))
    a, b = m.encode(m.ht_sig_bits(mcs, ht_length))
    coded = np.stack([a, b], 1).reshape(-1)
    for h in range(2):
        sym = np.fft.ifft(m._dup40(m._leg_symbol(coded[48 * h:48 * h + 48], True, 1.0))) * 128.0
        parts.append(np.concatenate([sym[-32:], sym]))
    parts.append(np.tile(stf, 2)[:160])
    return np.concatenate(parts)


def tx_frame_joint(psdu_with_fcs, mcs, seed=SEED):
    """as py_ht40.tx_frame: (complex128 [2, n] @40 MHz, nsym, first sample of HT-LTF 1)"""
    nb, cr = m.MCS2[mcs]
    data, nsym = tx_joint(psdu_with_fcs, nb, cr, seed)
    pre = _preamble_float(mcs, len(psdu_with_fcs), nsym)
    return np.concatenate([np.stack([pre, pre]), data], axis=1), nsym, len(pre)


# ------------------------------------------------------------------ the integer frame
def frame_int_joint(psdu_with_fcs, mcs, seed=SEED, amp=T.A, oracle=None):
    """as tx_ht40_model.frame_int: (int16 [2 chains, n, 2], nsym, first sample of HT-LTF 1)"""
    nb, cr = m.MCS2[mcs]
    il = stream_symbols(psdu_with_fcs, nb, cr, seed)
    nsym = il.shape[1]
    d = T.level(nb, amp)
    car = np.array([m.bin_of(k) for k in m.DATA_CARRIERS]); pil = np.array([m.bin_of(k) for k in m.PILOTS])
    D = np.zeros((2, nsym, 128, 2), np.int64)
    for s in range(2):
        for n in range(nsym):
            odd = m.qam(il[s, n].astype(float), nb) / m.LEVEL[nb]
            D[s, n, car, 0] = np.rint(odd.real).astype(np.int64) * d
            D[s, n, car, 1] = np.rint(odd.imag).astype(np.int64) * d
            D[s, n, pil, 0] = 2 * T.level(1, amp)
    P = T.preamble_bins(mcs, len(psdu_with_fcs), nsym, amp)
    f = lambda bins: T.ifft128(bins, oracle)
    stf, ltf = f(P["stf"]), f(P["lltf"])
    pre = np.concatenate([np.tile(stf, (3, 1))[:320], ltf[-64:], ltf, ltf, T._cp(f(P["lsig"])), T._cp(f(P["htsig0"])), T._cp(f(P["htsig1"])),
                          np.tile(stf, (2, 1))[:160]])
    plus, minus = T._cp(f(T._htltf_bins(1, amp))), T._cp(f(T._htltf_bins(-1, amp)))
    chains = [np.concatenate([pre, plus, plus if s else minus] + [T._cp(f(D[s, n])) for n in range(nsym)]) for s in range(2)]
    return np.stack(chains).astype(np.int16), nsym, len(pre)


def frame_int_joint_nofcs(mpdu, mcs, seed=SEED, amp=T.A, oracle=None):
    """the same from an MPDU WITHOUT FCS (what sora_hip_tx_ht40_joint takes) -> int16 [2, n, 2]"""
    return frame_int_joint(m.add_fcs(mpdu), mcs, seed, amp, oracle)[0]


# ------------------------------------------------------------------ the integer receive model
def deparse(soft0, soft1, nbpsc):
    """the two streams' de-interleaved soft bytes [nsym * N_CBPSS] -> the one stream the decoder reads [nsym * 2 N_CBPSS]"""
    ncb = 108 * nbpsc
    nsym = len(soft0) // ncb
    iss, k = parser_map(nbpsc)
    per = np.stack([np.asarray(soft0).reshape(nsym, ncb), np.asarray(soft1).reshape(nsym, ncb)])
    return np.ascontiguousarray(per[iss, :, k].T).reshape(-1)               # [2 ncb, nsym] -> symbol after symbol


class Result:
    def __init__(self, soft, per_stream, theta, xs, error_code, crc32, psdu, nsym):
        self.soft, self.per_stream, self.theta, self.xs, self.error_code, self.crc32, self.psdu, self.nsym = soft, per_stream, theta, xs, error_code, crc32, psdu, nsym


def rx_model(iq, offset, n_bpsc, code_rate, length, cfo, weights, decode=True):
    """iq int16 [2, n, 2]; offset: first sample of HT-LTF 1; length: the PSDU's bytes; weights int16 [4, 128, 2].  The per-stream soft bytes are
    oracle/ht40_data_model.py's (so_ht40_data_field, called as its model() calls it, with the joint symbol count) -> Result: soft = the merged stream"""
    nsym = nsym_for(length, n_bpsc, code_rate)
    a, b = dm._frame(iq, offset, nsym)
    w = np.ascontiguousarray(weights, np.int16).reshape(4, 128, 2)
    per = nsym * 108 * n_bpsc
    soft = [np.zeros(per, np.uint8), np.zeros(per, np.uint8)]
    theta = np.zeros(nsym + 1, np.int16); xs = np.zeros((nsym, 2, 128, 2), np.int16)
    d0, d1 = dm.permutation(n_bpsc, 0), dm.permutation(n_bpsc, 1)
    O = dm.oracle(); P = dm._P
    n = O.L.so_ht40_data_field(P(a), P(b), ctypes.c_uint32(nsym), int(n_bpsc), ctypes.c_int32(int(cfo)), P(w), P(dm.DATA_BINS), len(dm.DATA_BINS),
                               P(dm.PILOT_BINS), len(dm.PILOT_BINS), P(d0), P(d1), P(soft[0]), P(soft[1]), P(theta), P(xs))
    assert n == per, n
    merged = deparse(soft[0], soft[1], n_bpsc)
    e = crc = psdu = None
    if decode:
        dec = O.viterbi_frame_ex(merged, code_rate, int(length), 192, 36)
        e, psdu, crc = O.desc_sink(dec, int(length))
        e &= 0xFFFFFFFF; psdu = psdu.tobytes()
    return Result(merged, soft, theta, xs, e, crc, psdu, nsym)
