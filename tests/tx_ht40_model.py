"""tx_ht40_model.py -- TEST INFRASTRUCTURE: the integer model of the 40 MHz HT 2x2 transmitter (sora_hip_tx_ht40, k_tx_ht40.hip).

oracle/py_ht40.py::tx_frame defines the format in float64 (field order and lengths, the duplicated legacy part with its upper half
rotated by +90 degrees, P = [[1, -1], [1, 1]], carrier plan, pilots, interleaver, Gray mapping, L-SIG / HT-SIG contents, N_SYM); a GPU
kernel cannot be sample-exact with np.fft.ifft.  This module restates the same frame in integers:
  * bins: every frequency-domain value of tx_frame (HT-LTF carrier = 1) times A, rounded with np.rint to a COMPLEX16 bin -- LTF and SIG
    carriers +-A, STF rint(A sqrt(13/12)) on I and Q, data levels d(N_BPSC) = rint(A LEVEL / 128) times the odd integers of qam(), data
    pilots 2 d(1); the upper half's rotation by j is exact;
  * transform: every symbol, the preamble's included, through the reference's fixed-point IFFT<128> (Oracle().fft(x, 128, inverse=True):
    natural order in and out, gain ~ 1/128), so frame_int(...) ~ tx_frame(...) * A / 128 to within the transform's rounding;
  * the 32-sample cyclic prefix is the last 32 of the 128; L-LTF is the last 64 plus the symbol twice; L-STF is the symbol tiled to 320
    samples and HT-STF to 160.
Bit-level helpers and tables come from oracle.py_ht40; nothing here imports the library under test."""
import numpy as np

from oracle import py_ht40 as m

A = 16384
_ORACLE = None


def _oracle():
    global _ORACLE
    if _ORACLE is None:
        from oracle.pyoracle import Oracle
        _ORACLE = Oracle()
    return _ORACLE


def level(nbpsc, amp=A):
    """the spacing / 2 of a data constellation in bin units"""
    return int(np.rint(amp * m.LEVEL[nbpsc] / 128.0))


def to_bins(X, amp=A):
    """complex spectrum in tx_frame's unit (HT-LTF carrier = 1) -> int64 [..., 128, 2] bins"""
    X = np.asarray(X, complex) * amp
    return np.stack([np.rint(X.real), np.rint(X.imag)], axis=-1).astype(np.int64)


def ifft128(bins, oracle=None):
    """int [128, 2] bins -> int16 [128, 2] time samples (natural order) through the reference's fixed-point IFFT<128>"""
    b = np.asarray(bins)
    assert b.shape == (128, 2) and np.abs(b).max() <= 32767
    return (oracle or _oracle()).fft(b.astype(np.int16), n=128, inverse=True)


def data_bins(psdus, nbpsc, code_rate, seeds=(0x5D, 0x2B), amp=A):
    """the data symbols' bins, int64 [2 streams, nsym, 128, 2]: py_ht40.tx's bit pipeline, integer levels"""
    nsym = m.nsym_for([len(p) for p in psdus], nbpsc, code_rate)
    d = level(nbpsc, amp)
    X = np.zeros((2, nsym, 128, 2), np.int64)
    ncbpss = 108 * nbpsc
    car = np.array([m.bin_of(k) for k in m.DATA_CARRIERS])
    pil = np.array([m.bin_of(k) for k in m.PILOTS])
    for s in range(2):
        a, b = m.encode(m.stream_bits(psdus[s], nsym, nbpsc, code_rate, seeds[s] & 0x7F))
        coded = m.puncture(a, b, code_rate)
        imap = m.interleave_map(nbpsc, s)
        for n in range(nsym):
            il = np.zeros(ncbpss, np.uint8); il[imap] = coded[n * ncbpss:(n + 1) * ncbpss]
            odd = m.qam(il.astype(float), nbpsc) / m.LEVEL[nbpsc]                    # the odd integers (+-1 on I alone for BPSK)
            X[s, n, car, 0] = np.rint(odd.real).astype(np.int64) * d
            X[s, n, car, 1] = np.rint(odd.imag).astype(np.int64) * d
            X[s, n, pil, 0] = 2 * level(1, amp)
    return X


def _htltf_bins(sign, amp=A):
    X = np.zeros(128, complex)
    for k in range(-58, 59):
        X[m.bin_of(k)] = sign * int(m.HTLTF40[k + 58])
    return to_bins(X, amp)


def preamble_bins(mcs, ht_length, nsym, amp=A):
    """-> dict of int64 [128, 2] bins: stf, lltf, lsig, htsig0, htsig1 (identical on both chains), as tx_frame builds them"""
    l_length = max(1, -(-(36 + 4 * nsym + 4 - 20) // 4) * 3 - 3)
    a, b = m.encode(m.l_sig_bits(l_length))
    out = {"stf": to_bins(m._dup40(m._STF), amp), "lltf": to_bins(m._dup40(m._LTF), amp),
           "lsig": to_bins(m._dup40(m._leg_symbol(np.stack([a, b], 1).reshape(-1), False, 1.0)), amp)}
    a, b = m.encode(m.ht_sig_bits(mcs, ht_length))
    coded = np.stack([a, b], 1).reshape(-1)
    for h in range(2):
        out["htsig%d" % h] = to_bins(m._dup40(m._leg_symbol(coded[48 * h:48 * h + 48], True, 1.0)), amp)
    return out


def _cp(t):
    return np.concatenate([t[-32:], t])


def frame_int(psdus, mcs, seeds=(0x5D, 0x2B), amp=A, oracle=None):
    """psdus: two byte strings WITH FCS, of equal length.  -> (int16 [2 chains, n, 2], nsym, first sample of HT-LTF 1): the integer frame"""
    assert len(psdus[0]) == len(psdus[1]) and mcs in m.MCS2
    nb, cr = m.MCS2[mcs]
    D = data_bins(psdus, nb, cr, seeds, amp)
    nsym = D.shape[1]
    P = preamble_bins(mcs, len(psdus[0]), nsym, amp)
    f = lambda bins: ifft128(bins, oracle)
    stf, ltf = f(P["stf"]), f(P["lltf"])
    pre = np.concatenate([np.tile(stf, (3, 1))[:320], ltf[-64:], ltf, ltf, _cp(f(P["lsig"])), _cp(f(P["htsig0"])), _cp(f(P["htsig1"])),
                          np.tile(stf, (2, 1))[:160]])
    plus, minus = _cp(f(_htltf_bins(1, amp))), _cp(f(_htltf_bins(-1, amp)))
    chains = []
    for s in range(2):                                                               # P = [[1, -1], [1, 1]]
        chains.append(np.concatenate([pre, plus, plus if s else minus] + [_cp(f(D[s, n])) for n in range(nsym)]))
    return np.stack(chains).astype(np.int16), nsym, len(pre)


def frame_int_nofcs(mpdu0, mpdu1, mcs, seeds=(0x5D, 0x2B), amp=A, oracle=None):
    """the same from two MPDUs WITHOUT FCS (what sora_hip_tx_ht40 takes) -> int16 [2, n, 2]"""
    return frame_int([m.add_fcs(mpdu0), m.add_fcs(mpdu1)], mcs, seeds, amp, oracle)[0]
