"""mod11n_model.py -- TEST INFRASTRUCTURE: the bricks of the 802.11n 2x2 modulation graphs (kernel/bb/demod11/fb11nmod_config.hpp: CreatePreambleGraph11n,
CreateSigGraph11n, CreateModGraph11n) that tests/mod11a_model.py does not already hold, one numpy function per brick, in the bricks' own port formats: bits
packed in bytes, LSB first, as the pins carry them.  The truth of tests/test_gpu_mod11n_stages.py; tests/test_mod11n_model.py pins it to the recorded and the
compiled reference modulator without a GPU.

Each function restates its brick the way the brick computes -- the parsers through their `split` and byte loops, the interleaver through the loop that builds its
table (k over whole input bytes), the pilots through the bricks' tables -- and not the closed forms of sora_amd/csrc/k_mod11n.hip.  Taken from elsewhere: the
scrambler, the encoder, the SIG graph's T11aInterleaveBPSK and T11aAddPilot (mod11a_model), the fixed-point IFFT<128> (Oracle().fft), and the fixed fields of
LSrc / HTSrc, which are read from the recorded frames (tests/golden/refgraph_11n.npz).  Nothing here imports the library under test."""
import os
import zlib

import numpy as np

import mod11a_model as A
from mod11a_model import CR_12, CR_23, CR_34, _bits, _bytes, _qam_level

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BPSK_MOD = 30339
MOD_OF = {1: 30339, 2: 21453, 4: 9594, 6: 4681}                                  # fb11nmod_config.hpp:121-128
# MCS -> (N_BPSC, code rate, N_DBPS)            DOT11N_RATE_PARAMS, BB11nGetCodingRateFromMcsIndex (ieee80211n_cmn.h:7-25)
MCS = {8: (1, CR_12, 52), 9: (2, CR_12, 104), 10: (2, CR_34, 156), 11: (4, CR_12, 208), 12: (4, CR_34, 312), 13: (6, CR_23, 416), 14: (6, CR_34, 468)}


def row_bytes(n_bpsc):
    return (52 * n_bpsc + 7) // 8                                                # N_b = ceiling_div<N_CBPS, 8>


# ---- TStreamParser{BPSK,QPSK,QAM16,QAM64}_12 (streamparser.hpp, _b_stream_parser.h)
def _split1(b):                                                                  # stream_paser_bpsk_2ss::split, _qpsk_2ss::split (:34-47, :103-114)
    lb = (b & 0x01) | ((b & 0x4) >> 1) | ((b & 0x10) >> 2) | ((b & 0x40) >> 3)
    hb = ((b & 0x02) >> 1) | ((b & 0x8) >> 2) | ((b & 0x20) >> 3) | ((b & 0x80) >> 4)
    return lb, hb


def _split2(b):                                                                  # stream_paser_16qam_2ss::split (:167-174)
    return (b & 0x03) | ((b & 0x30) >> 2), ((b & 0x0C) >> 2) | ((b & 0xC0) >> 4)


def _split3(b):                                                                  # stream_paser_64qam_2ss::split over 12 bits (:249-256)
    return (b & 0x0007) | ((b & 0x01C0) >> 3), ((b & 0x0038) >> 3) | ((b & 0x0E00) >> 6)


def stream_parse(sym, n_bpsc):
    """sym uint8 [n, 13 n_bpsc] -> (uint8 [n, N_b], the same): outputs 0 and 1"""
    x = np.asarray(sym, np.uint8).astype(np.int64)
    n, nb = len(x), row_bytes(n_bpsc)
    o = [np.zeros((n, nb + 1), np.int64), np.zeros((n, nb + 1), np.int64)]     # (+ 1: the 64-QAM parser's last 32-bit store runs one byte over the port)
    if n_bpsc in (1, 2, 4):
        split = _split2 if n_bpsc == 4 else _split1
        npair = 6 if n_bpsc == 1 else 13 * n_bpsc // 2
        for j in range(npair):                                                   # lookuptable[b1][b2] = ((lb2 << 4) | lb1, (hb2 << 4) | hb1)
            l1, h1 = split(x[:, 2 * j]); l2, h2 = split(x[:, 2 * j + 1])
            o[0][:, j] = (l2 << 4) | l1; o[1][:, j] = (h2 << 4) | h1
        if n_bpsc == 1:                                                          # lookuptable2: the half byte, its upper four bits 0 (:24-25, :63-64)
            o[0][:, 6], o[1][:, 6] = split(x[:, 12])
    else:
        w = x[:, 0::2] | (x[:, 1::2] << 8)                                       # psInput: 39 little-endian words
        for i in range(0, 39, 3):                                                # (:216-242) four 12-bit groups -> 6 bits each, 24 bits per output and turn
            g = [w[:, i] & 0x0FFF, (w[:, i] >> 12) | ((w[:, i + 1] & 0x00FF) << 4), (w[:, i + 1] >> 8) | ((w[:, i + 2] & 0x000F) << 8), w[:, i + 2] >> 4]
            for s in (0, 1):
                v = sum(_split3(gk)[s] << (6 * k) for k, gk in enumerate(g))
                for b in range(4):                                               # *piOutput = ...: a 32-bit store at byte j = i
                    o[s][:, i + b] = (v >> (8 * b)) & 0xFF
    return o[0][:, :nb].astype(np.uint8), o[1][:, :nb].astype(np.uint8)


# ---- T11nInterleave*_S1 / _S2 = T11Interleave<52 N_BPSC, N_BPSC, 13, 11, I_SS> (interleave.hpp:17-123)
def interleave_targets(n_bpsc, iss):
    """r(k) for k = 0 .. 8 N_b - 1: the table is built over whole input bytes (:37-57), so for BPSK k runs to 55.  iss = I_SS - 1."""
    n_cbps, n_col, n_rot, n_s = 52 * n_bpsc, 13, 11, max(n_bpsc // 2, 1)
    out = []
    for k in range(8 * row_bytes(n_bpsc)):
        i = n_cbps // n_col * (k % n_col) + k // n_col
        j = n_s * (i // n_s) + (i + n_cbps - n_col * i // n_cbps) % n_s
        out.append((n_cbps + j - ((iss * 2) % 3 + 3 * (iss // 3)) * n_rot * n_bpsc) % n_cbps)
    return np.array(out)


def interleave(sym, n_bpsc, iss):
    """sym uint8 [..., N_b] -> the same shape: lut[kbyte][vbyte][r / 32] |= bit << r % 32, the tables of a symbol's bytes ORed (:91-99)"""
    bits = _bits(sym)
    out = np.zeros(bits.shape[:-1] + (32 * ((52 * n_bpsc + 31) // 32),), np.uint8)
    for k, r in enumerate(interleave_targets(n_bpsc, iss)):
        out[..., r] |= bits[..., k]
    return _bytes(out)[..., :row_bytes(n_bpsc)]


# ---- TMap11a*<MOD> as the 11n graph instantiates them (mapper11a.hpp:8-300), the BPSK brick's last four carriers dropped by T11nAddPilot's ipin.clear()
def map11n(sym, n_bpsc, mod=0):
    """sym uint8 [n, N_b] -> int16 [n, 52, 2]"""
    mod = mod or MOD_OF[n_bpsc]
    bits = _bits(sym)
    out = np.zeros((len(sym), 52, 2), np.int16)
    if n_bpsc == 1:                                                              # MapBPSK per byte: 56 carriers, of which pilot_11n.hpp:78-79 keeps 52
        out[..., 0] = np.where(bits == 1, mod, -mod)[:, :52]
        return out
    M = n_bpsc // 2
    bits = bits.reshape(len(sym), 52, n_bpsc)
    lv = np.array([_qam_level(v, M, mod) for v in range(1 << M)], np.int16)
    w = 1 << np.arange(M)
    out[..., 0] = lv[(bits[..., :M] * w).sum(-1)]
    out[..., 1] = lv[(bits[..., M:] * w).sum(-1)]
    return out


# ---- TSigMap11n (mapper11n.hpp)
def sig_map(b18):
    """uint8 [n, 18] -> int16 [n, 144, 2]: bytes 0..5 MapBPSK, bytes 6..17 MapQBPSK, TMapperCore<30339>"""
    lv = np.where(_bits(b18) == 1, BPSK_MOD, -BPSK_MOD).astype(np.int16)
    out = np.zeros((len(lv), 144, 2), np.int16)
    out[:, :48, 0] = lv[:, :48]; out[:, 48:, 1] = lv[:, 48:]
    return out


# ---- T11nAddPilot<iss> (pilot_11n.hpp:7-82), dot11_ofdm_pilot (_b_dot11_pilot.h:3-43)
PILOT = np.array([[[1, 1, -1, -1], [1, -1, -1, 1]], [[1, -1, -1, 1], [-1, -1, 1, 1]], [[-1, -1, 1, 1], [-1, 1, 1, -1]], [[-1, 1, 1, -1], [1, 1, -1, -1]]])
PILOT_SIGN = np.array([
    1, 1, 1, -1, -1, -1, 1, -1, -1, -1, -1, 1, 1, -1, 1, -1, -1, 1, 1, -1, 1, 1, -1, 1, 1, 1, 1, 1, 1, -1, 1, 1,
    1, -1, 1, 1, -1, -1, 1, 1, 1, -1, 1, -1, -1, -1, 1, -1, 1, -1, -1, 1, -1, -1, 1, 1, 1, 1, 1, -1, -1, 1, 1, -1,
    -1, 1, -1, 1, -1, 1, 1, -1, -1, -1, 1, 1, -1, -1, -1, -1, 1, -1, -1, 1, -1, 1, 1, 1, 1, -1, 1, -1, 1, -1, 1, -1,
    -1, -1, -1, -1, 1, -1, 1, 1, -1, 1, -1, 1, 1, 1, -1, -1, 1, -1, -1, -1, 1, 1, 1, -1, -1, -1, -1, -1, -1, -1, 1])


class AddPilot:
    def __init__(self, iss):
        self.iss = iss
        self.reset()

    def reset(self):
        self.index = 0                                                           # _init (:22-24)

    def process(self, car):
        """car int16 [n, 52, 2], symbols of one frame in order -> int16 [n, 64, 2]"""
        out = np.zeros((len(car), 64, 2), np.int16)                              # opin().zerobuf() (:36)
        for s, c in enumerate(np.asarray(car, np.int16)):
            p = PILOT_SIGN[(self.index + 3) % 127] * PILOT[self.index & 3][self.iss]   # _pilot_tracker(iss, pilot_index, _pilots)
            k = 0
            for i in list(range(64 - 28, 64)) + list(range(1, 29)):              # :55-66
                if i in (64 - 7, 64 - 21, 7, 21):
                    continue
                out[s, i] = c[k]; k += 1
            for i, v in zip((64 - 21, 64 - 7, 7, 21), p):                        # :68-71
                out[s, i] = (BPSK_MOD * v, 0)
            self.index += 1
        return out


def add_pilot(car, iss, pos0=0):
    """the symbols of ONE frame from position pos0 on (pos0 = 0: a brick after Reset)"""
    ap = AddPilot(iss); ap.index = pos0
    return ap.process(car)


# ---- TIFFTxOnly (fft.hpp:63-103)
def ifft_only(bins, ifft128=None):
    """bins int16 [n, 64, 2] -> int16 [n, 128, 2]"""
    f = ifft128 or A._ifft128
    bins = np.asarray(bins, np.int16)
    out = np.zeros((len(bins), 128, 2), np.int16)
    for s, b in enumerate(bins):
        t = np.zeros((128, 2), np.int16)
        t[:32] = b[:32]; t[96:] = b[32:]                                         # oversampled_ifft (:93-102)
        out[s] = np.asarray(f(t), np.int16)
    return out


# ---- TCSD<ncsd> (csd.hpp:38-52)
def csd(x, ncsd):
    """int16 [n, 128, 2] -> the same shape"""
    v = np.asarray(x, np.int16).reshape(len(x), 32, 4, 2)                        # vcs: four samples
    out = np.zeros_like(v)
    i = 0
    while i < 32 - ncsd:
        out[:, i + ncsd] = v[:, i]; i += 1
    j = 0
    while i < 32:
        out[:, j] = v[:, i]; i += 1; j += 1
    return out.reshape(len(x), 128, 2)


# ---- TAddGI (gi.hpp:32-41)
def add_gi(x):
    """int16 [n, 128, 2] -> int16 [n, 160, 2]"""
    x = np.asarray(x, np.int16)
    return np.concatenate([x[:, 128 - 32:], x], axis=1)


# ---- LSrc / HTSrc (preamble11n.hpp): fixed samples, read from a recorded frame
def preamble(field):
    """field 0: L-STF, L-LTF -> (int16 [640, 2], the same) for TX chains 0 and 1; field 1: HT-STF, HT-LTF1, HT-LTF2 -> 480 each"""
    z = np.load(os.path.join(GOLD, "refgraph_11n.npz"))
    sl = slice(0, 640) if field == 0 else slice(1120, 1600)
    return z["tx0_0"][sl].astype(np.int16), z["tx0_1"][sl].astype(np.int16)


# ---- TBB11nSigSrc and TBB11nSrc (PHY_11n.hpp:81-133, 251-278; ieee80211n_cmn.h:33-55; _b_lsig.h; _b_htsig.h; CRC8.h)
def _crc8(data, nbytes, ntail):
    lut = []
    for v in range(256):                                                         # LUT_CRC8: eight steps of the tail loop below
        for _ in range(8):
            v = (v >> 1) ^ 0xE0 if v & 1 else v >> 1
        lut.append(v)
    assert lut[1] == 0x91 and lut[255] == 0xCF                                   # CRC8.h:17, :24
    crc = 0xFF
    for i in range(nbytes):
        crc = lut[crc ^ data[i]]
    crc ^= data[nbytes] & ((1 << ntail) - 1)
    for _ in range(ntail):
        crc = (crc >> 1) ^ 0xE0 if crc & 1 else crc >> 1
    return ~crc & 0xFF


def fields(mpdu, mcs):
    """-> (the 9 SIG bytes; SERVICE + MPDU + FCS + tail + pad as TBB11nSrc emits them; the index of the tail byte; the symbols the graph emits)"""
    nb, cr, nd = MCS[mcs]
    mpdu = bytes(mpdu)
    ln = len(mpdu) + 4
    nstd = -(-(ln * 8 + 16 + 6) // nd)                                           # ht_symbol_count
    lsig = 0xB | ((((nstd + 5) * 24 - 16 - 6) // 8) << 5)                        # L_SIG::update(DOT11A_RATE_6M, lsig_frame_length)
    par = lsig ^ (lsig >> 16); par ^= par >> 8; par ^= par >> 4; par ^= par >> 2; par ^= par >> 1
    lsig |= (par & 1) << 17
    ht = [mcs & 0xFF, ln & 0xFF, ln >> 8, 3, 0, 0]                               # HT_SIG::update
    crc = _crc8(ht, 4, 2)
    ht[4] |= (crc << 2) & 0xFF; ht[5] |= crc >> 6
    total_bits = nstd * nd                                                       # ht_padding_bytes
    total_bytes = total_bits // 8 + (1 if total_bits % 8 else 0)
    npad = (total_bytes - ln - 2) - 1
    data = np.zeros(2 + ln + 1 + npad, np.uint8)
    data[2:2 + len(mpdu)] = np.frombuffer(mpdu, np.uint8)
    data[2 + len(mpdu):2 + ln] = np.frombuffer((zlib.crc32(mpdu) & 0xFFFFFFFF).to_bytes(4, "little"), np.uint8)
    gin = cr + 1                                                                 # Flush: the encoder's last burst, then the parser's last symbol, padded with zeros
    ngroups = -(-len(data) // gin)
    nsym = -(-(gin + 1) * ngroups // (13 * nb))
    return np.array([lsig & 255, (lsig >> 8) & 255, lsig >> 16] + ht, np.uint8), data, 2 + ln, nsym


def compose(mpdu, mcs, seed=0xAB):
    """CreatePreambleGraph11n + CreateSigGraph11n + CreateModGraph11n as Test11N_FB_Mod drives them -> (int16 [n, 2] for TX chain 0, the same for chain 1)"""
    nb, cr, nd = MCS[mcs]
    sig, data, tail, nsym = fields(mpdu, mcs)
    # SIG graph
    s = A.interleave(A.conv_encode(sig, CR_12).reshape(3, 6), 1)
    t = ifft_only(A.add_pilot(sig_map(s.reshape(1, 18)).reshape(3, 48, 2), BPSK_MOD))
    sig0, sig1 = add_gi(t), add_gi(csd(t, 2))
    # data graph
    scr = A.scramble(data, seed, tail)
    gin = cr + 1
    scr = np.concatenate([scr, np.zeros(-len(scr) % gin, np.uint8)])
    coded = A.conv_encode(scr, cr)
    coded = np.concatenate([coded, np.zeros(nsym * 13 * nb - len(coded), np.uint8)]).reshape(nsym, 13 * nb)
    p = stream_parse(coded, nb)
    t0 = ifft_only(add_pilot(map11n(interleave(p[0], nb, 0), nb), 0))
    t1 = ifft_only(add_pilot(map11n(interleave(p[1], nb, 1), nb), 1))
    d0, d1 = add_gi(t0), add_gi(csd(t1, 4))
    l, h = preamble(0), preamble(1)
    return (np.concatenate([l[0], sig0.reshape(-1, 2), h[0], d0.reshape(-1, 2)]), np.concatenate([l[1], sig1.reshape(-1, 2), h[1], d1.reshape(-1, 2)]))
