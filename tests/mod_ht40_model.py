"""mod_ht40_model.py -- TEST INFRASTRUCTURE: the bricks of the 40 MHz HT 2x2 modulation graph (include/sora_hip.h: sora_hip_*_ht40 behind sora_hip_tx_ht40;
sora_amd/csrc/k_mod_ht40.hip), one numpy function per stage, in the stages' port formats: bits packed in bytes, LSB first, N_b40 = ceil(108 n_bpsc / 8) bytes per
stream and symbol.  The truth of tests/test_gpu_mod_ht40_stages.py; tests/test_mod_ht40_model_cpu.py pins compose() to the three frame models without a GPU.

The reference has no 40 MHz graph: each function computes what its stage is DEFINED to compute, from the tables that define the format -- the interleaver map, the
Gray map, the carrier plan, the SIG bit fields and the legacy symbol's layout are oracle.py_ht40's, the parser's rule is ht40_joint_model.parser_map, the transform is
tx_ht40_model.ifft128 -- and not from the closed forms of the kernels.  The scrambler, the encoder and the SIG symbols' interleaver are the 802.11a stages
(mod11a_model).  Nothing here imports the library under test."""
import zlib

import numpy as np

from oracle import py_ht40 as m
import ht40_joint_model as J
import mod11a_model as A
import tx_ht40_gi_model as G
import tx_ht40_model as T
from mod11a_model import _bits, _bytes

SIG_AMP = T.A                                                                    # an L-SIG / HT-SIG carrier and their pilots
PILOT = 2 * T.level(1)                                                           # 12288
PER_STREAM, JOINT = 0, 1


def row_bytes(n_bpsc):
    return (108 * n_bpsc + 7) // 8


def stage_seed(seed):
    """the register T11aSc (sora_hip_scramble11a) starts from for py_ht40.scramble_seq's seed: seed bit i = x[-1 - i] sits at register bit 7 - i"""
    return sum(((int(seed) >> i) & 1) << (7 - i) for i in range(7))


# ---- the stream parser on the 216 n_bpsc coded bits of a symbol
def stream_parse(sym, n_bpsc):
    """sym uint8 [n, 27 n_bpsc] -> (uint8 [n, N_b40], the same): spatial streams 0 and 1"""
    bits = _bits(np.asarray(sym, np.uint8).reshape(-1, 27 * n_bpsc))
    iss, k = J.parser_map(n_bpsc)
    out = []
    for s in (0, 1):
        o = np.zeros((len(bits), 8 * row_bytes(n_bpsc)), np.uint8)
        o[:, k[iss == s]] = bits[:, iss == s]
        out.append(_bytes(o))
    return out[0], out[1]


# ---- the HT interleaver for 40 MHz
def interleave(sym, n_bpsc, iss):
    """sym uint8 [..., N_b40] -> the same shape: input bit k < 108 n_bpsc goes to bit interleave_map(k); BPSK's input bits 108..111 are not read"""
    bits = _bits(sym)
    out = np.zeros_like(bits)
    out[..., m.interleave_map(n_bpsc, iss)] = bits[..., :108 * n_bpsc]
    return _bytes(out)


def interleave_stream(stream, nsym, n_bpsc, iss):
    """stream uint8 [>= ceil(108 n_bpsc nsym / 8)]: one frame's coded bits, contiguous -> uint8 [nsym, N_b40]"""
    ncb = 108 * n_bpsc
    bits = _bits(np.asarray(stream, np.uint8))[:nsym * ncb].reshape(nsym, ncb)
    out = np.zeros((nsym, 8 * row_bytes(n_bpsc)), np.uint8)
    out[:, m.interleave_map(n_bpsc, iss)] = bits
    return _bytes(out)


# ---- the mapper
def map40(sym, n_bpsc):
    """sym uint8 [n, N_b40] -> int16 [n, 108, 2]: py_ht40.qam's odd integers times tx_ht40_model.level(n_bpsc)"""
    sym = np.asarray(sym, np.uint8).reshape(-1, row_bytes(n_bpsc))
    bits = _bits(sym)[:, :108 * n_bpsc]
    d = T.level(n_bpsc)
    out = np.zeros((len(sym), 108, 2), np.int16)
    for i, b in enumerate(bits):
        odd = m.qam(b.astype(float), n_bpsc) / m.LEVEL[n_bpsc]
        out[i, :, 0] = np.rint(odd.real).astype(np.int64) * d
        out[i, :, 1] = np.rint(odd.imag).astype(np.int64) * d
    return out


# ---- L-SIG + HT-SIG
def sig_map(b18):
    """uint8 [n, 18]: three interleaved BPSK symbols of 48 bits per frame -> int16 [n, 3, 128, 2]: py_ht40._leg_symbol behind its interleaver, _dup40, times A"""
    bits = _bits(np.asarray(b18, np.uint8).reshape(-1, 18)).reshape(-1, 3, 48)
    out = np.zeros((len(bits), 3, 128, 2), np.int16)
    for f in range(len(bits)):
        for h in range(3):
            s = np.zeros(53, complex)
            for c, kk in enumerate(m._LEG_DATA):
                v = 2.0 * bits[f, h, c] - 1.0
                s[kk + 26] = 1j * v if h else v                                  # L-SIG on I, HT-SIG on Q
            for kk, p in zip((-21, -7, 7, 21), (1, 1, 1, -1)):
                s[kk + 26] = p
            out[f, h] = T.to_bins(m._dup40(s), SIG_AMP)
    return out


# ---- data carriers and pilots onto the 128 bins
def add_pilot(car):
    """int16 [n, 108, 2] -> int16 [n, 128, 2]"""
    car = np.asarray(car, np.int16)
    out = np.zeros((len(car), 128, 2), np.int16)
    out[:, [m.bin_of(k) for k in m.DATA_CARRIERS]] = car
    out[:, [m.bin_of(k) for k in m.PILOTS]] = (PILOT, 0)
    return out


# ---- the reference's fixed-point IFFT<128>, natural order
def ifft(bins):
    """int16 [n, 128, 2] -> int16 [n, 128, 2]"""
    bins = np.asarray(bins, np.int16)
    out = np.zeros_like(bins)
    for i, b in enumerate(bins):
        # (tx_ht40_model.ifft128 refuses -32768, which no frame holds; the rail test goes to the oracle transform it wraps)
        out[i] = T.ifft128(b) if b.min() > -32768 else T._oracle().fft(np.ascontiguousarray(b), n=128, inverse=True)
    return out


# ---- the guard interval
def add_gi(x, gi):
    """int16 [n, 128, 2] -> int16 [n, 160, 2] (gi 0) or [n, 144, 2] (gi 1)"""
    x = np.asarray(x, np.int16)
    cp = G.CP_SHORT if gi else 32
    return np.concatenate([x[:, 128 - cp:], x], axis=1)


# ---- the fixed fields
def preamble(field):
    """field 0: L-STF, L-LTF -> (int16 [640, 2], the same) for TX chains 0 and 1; field 1: HT-STF, HT-LTF1, HT-LTF2 -> 480 each; as tx_ht40_model.frame_int builds them"""
    P = T.preamble_bins(8, 5, 1)                                                 # (stf and lltf depend on no argument)
    stf, ltf = T.ifft128(P["stf"]), T.ifft128(P["lltf"])
    if field == 0:
        x = np.concatenate([np.tile(stf, (3, 1))[:320], ltf[-64:], ltf, ltf]).astype(np.int16)
        return x, x.copy()
    plus, minus = T._cp(T.ifft128(T._htltf_bins(1))), T._cp(T.ifft128(T._htltf_bins(-1)))
    hs = np.tile(stf, (2, 1))[:160]
    return np.concatenate([hs, plus, minus]).astype(np.int16), np.concatenate([hs, plus, plus]).astype(np.int16)


# ---- the host's share
def fields(mpdus, mcs, coding=PER_STREAM, gi=0, seeds=None):
    """mpdus: (mpdu0, mpdu1) WITHOUT FCS (per-stream coding) or one MPDU (joint).  -> (the 9 SIG bytes; a list of one field per encoder -- SERVICE + PSDU + FCS + tail +
    pad up to N_SYM x N_DBPS bits, then zeros up to the encoder stage's whole bursts; the bytes of each field that are scrambled; the index of the tail byte; the
    scrambler stage's register per field; N_SYM)"""
    nb, cr = m.MCS2[mcs]
    ps = [m.add_fcs(mpdus)] if coding == JOINT else [m.add_fcs(mpdus[0]), m.add_fcs(mpdus[1])]
    ln = len(ps[0])
    nd = J.ndbps(nb, cr) if coding == JOINT else m.ndbps(nb, cr)
    nsym = -(-(16 + 8 * ln + 6) // nd)
    sig = _bytes(np.concatenate([m.l_sig_bits(G.l_length(nsym, gi)), G.ht_sig_bits(mcs, ln, gi)]))
    nbytes = (nsym * nd + 7) // 8
    data = []
    for p in ps:
        d = np.zeros(-(-nbytes // (cr + 1)) * (cr + 1), np.uint8)
        d[2:2 + ln] = np.frombuffer(p, np.uint8)
        data.append(d)
    if seeds is None:
        seeds = (J.SEED,) if coding == JOINT else (0x5D, 0x2B)
    seeds = [seeds] if np.ndim(seeds) == 0 else list(seeds)
    return sig, data, nbytes, 2 + ln, [stage_seed(s) for s in seeds], nsym


def compose(mpdus, mcs, coding=PER_STREAM, gi=0, seeds=None):
    """the chains of include/sora_hip.h, stage by stage -> int16 [2 chains, n, 2]"""
    nb, cr = m.MCS2[mcs]
    sig, data, nbytes, tail, regs, nsym = fields(mpdus, mcs, coding, gi, seeds)
    s = A.interleave(A.conv_encode(sig, A.CR_12).reshape(3, 6), 1)
    sig_t = add_gi(ifft(sig_map(s.reshape(1, 18)).reshape(3, 128, 2)), 0).reshape(-1, 2)
    coded = []
    for d, reg in zip(data, regs):
        d = d.copy()
        d[:nbytes] = A.scramble(d[:nbytes], reg, tail)
        coded.append(A.conv_encode(d, cr))
    if coding == JOINT:
        rows = stream_parse(coded[0][:nsym * 27 * nb].reshape(nsym, 27 * nb), nb)
        il = [interleave(rows[i], nb, i) for i in (0, 1)]
    else:
        il = [interleave_stream(coded[i], nsym, nb, i) for i in (0, 1)]
    l, h = preamble(0), preamble(1)
    chains = []
    for i in (0, 1):
        t = add_gi(ifft(add_pilot(map40(il[i], nb))), gi).reshape(-1, 2)
        chains.append(np.concatenate([l[i], sig_t, h[i], t]))
    return np.stack(chains).astype(np.int16)
