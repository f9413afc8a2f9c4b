"""tx_ht40_gi_model.py -- TEST INFRASTRUCTURE: the integer model of the 40 MHz HT 2x2 transmitter with a guard-interval kind (sora_hip_tx_ht40_gi,
sora_hip_tx_ht40_joint_gi), built on tests/tx_ht40_model.py and tests/ht40_joint_model.py.

Kind 0 is those models' frame.  Kind 1, the short guard interval, is the library's own definition of IEEE 802.11n-2009's HT-mixed short GI at 40 MHz:
  * the frame equals the long-GI frame of the same PSDUs, MCS and seeds up to and including HT-LTF 2 -- the legacy fields, HT-SIG, HT-STF and both HT-LTFs keep the
    32-sample cyclic prefix and 160-sample symbols -- except for the L-SIG and the HT-SIG symbols:
      - HT-SIG bit 31 (Short GI) is 1 and the CRC-8 over bits 0..33 follows;
      - L-SIG LENGTH follows py_ht40.tx_frame's rule with 4 N_SYM replaced by 4 ceil(9 N_SYM / 10): 3.6 us symbols rounded up to whole 4 us;
  * every data symbol is 144 samples: the last 16 of the symbol's 128 transformed samples, then the 128; a frame is 1600 + 144 N_SYM samples per chain;
  * N_SYM, scrambling, coding, puncturing, stream parsing, interleaving, mapping and pilots are unchanged: the 128 transformed samples of every data symbol are the long
    frame's.
Nothing here imports the library under test."""
import numpy as np

from oracle import py_ht40 as m
import ht40_joint_model as J
import tx_ht40_model as T

SYM_SHORT, CP_SHORT = 144, 16


def ht_sig_bits(mcs, length, gi):
    """py_ht40.ht_sig_bits with bit 31 = gi and the CRC-8 over bits 0..33 recomputed (T11nSigParser's: reflected, polynomial 0xE0, complemented)"""
    b = m.ht_sig_bits(mcs, length).copy()
    b[31] = 1 if gi else 0
    crc = 0xFF
    for i in range(34):
        crc ^= int(b[i])
        crc = (crc >> 1) ^ 0xE0 if crc & 1 else crc >> 1
    c = (~crc) & 0xFF
    for i in range(8):
        b[34 + i] = (c >> i) & 1
    return b


def l_length(nsym, gi):
    """py_ht40.tx_frame's L-SIG LENGTH; short GI: the data field's symbols counted as ceil(9 nsym / 10) symbols of 4 us"""
    n4 = -(-9 * nsym // 10) if gi else nsym
    return max(1, -(-(36 + 4 * n4 + 4 - 20) // 4) * 3 - 3)


def sig_symbols(mcs, ht_length, nsym, gi, amp=T.A, oracle=None):
    """-> int16 [480, 2]: the L-SIG and the two HT-SIG symbols (160 samples each, prefix 32) as tx_ht40_model.preamble_bins builds them, from the bits above"""
    out = []
    a, b = m.encode(m.l_sig_bits(l_length(nsym, gi)))
    out.append(T._cp(T.ifft128(T.to_bins(m._dup40(m._leg_symbol(np.stack([a, b], 1).reshape(-1), False, 1.0)), amp), oracle)))
    a, b = m.encode(ht_sig_bits(mcs, ht_length, gi))
    coded = np.stack([a, b], 1).reshape(-1)
    for h in range(2):
        out.append(T._cp(T.ifft128(T.to_bins(m._dup40(m._leg_symbol(coded[48 * h:48 * h + 48], True, 1.0)), amp), oracle)))
    return np.concatenate(out)


def frame_int(psdus, mcs, gi, seeds=None, joint=False, amp=T.A, oracle=None):
    """psdus: two byte strings WITH FCS of equal length (per-stream coding), or ONE (joint=True); seeds: (s0, s1) / one seed, None: the models' defaults.
    -> (int16 [2 chains, n, 2], nsym, first sample of HT-LTF 1)"""
    assert gi in (0, 1)
    if joint:
        long, nsym, ltf = J.frame_int_joint(psdus, mcs, J.SEED if seeds is None else seeds, amp, oracle)
        ht_length = len(psdus)
    else:
        long, nsym, ltf = T.frame_int(psdus, mcs, (0x5D, 0x2B) if seeds is None else seeds, amp, oracle)
        ht_length = len(psdus[0])
    if gi == 0:
        return long, nsym, ltf
    assert ltf == 1280 and long.shape[1] == 1600 + 160 * nsym
    sig = sig_symbols(mcs, ht_length, nsym, 1, amp, oracle).astype(np.int16)
    chains = []
    for c in range(2):
        head = long[c, :1600].copy()
        head[640:1120] = sig
        parts = [head]
        for d in range(nsym):
            t = long[c, 1600 + 160 * d + 32:1600 + 160 * d + 160]                    # the symbol's 128 transformed samples
            parts.append(np.concatenate([t[-CP_SHORT:], t]))
        chains.append(np.concatenate(parts))
    return np.stack(chains).astype(np.int16), nsym, ltf


def frame_int_nofcs(mpdus, mcs, gi, seeds=None, joint=False, amp=T.A, oracle=None):
    """the same from MPDUs WITHOUT FCS (what the entry points take): two (per-stream) or one (joint) -> int16 [2, n, 2]"""
    ps = m.add_fcs(mpdus) if joint else [m.add_fcs(mpdus[0]), m.add_fcs(mpdus[1])]
    return frame_int(ps, mcs, gi, seeds, joint, amp, oracle)[0]


def respace(frame, nsym, offset=1280):
    """a short-GI frame (or capture: [2, n, 2] with HT-LTF 1 at `offset`) -> the same with every 144-sample data symbol widened to 160 by putting its samples 112..127
    (useful samples 96..111) in front: what a long-GI receiver model reads (it never looks at the prefix).  What follows the frame is kept behind it."""
    x = np.asarray(frame)
    at = offset + 320
    parts = [x[:, :at]]
    for d in range(nsym):
        s = x[:, at + SYM_SHORT * d:at + SYM_SHORT * (d + 1)]
        parts.append(np.concatenate([s[:, 112:128], s], axis=1))
    parts.append(x[:, at + SYM_SHORT * nsym:])
    return np.ascontiguousarray(np.concatenate(parts, axis=1))
