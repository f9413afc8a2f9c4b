"""mod11a_model.py -- TEST INFRASTRUCTURE: the bricks of the 802.11a modulation graph (kernel/bb/demod11/fb11amod_config.hpp:74-110), one numpy
function per brick, in the bricks' own port formats: bits packed in bytes, LSB first, as the pins carry them.  The truth of tests/test_gpu_mod_stages.py;
tests/test_mod11a_model.py pins it to the oracle's transmitter (and through it to the compiled reference modulator) without a GPU.

Each function restates its brick the way the brick computes -- the scrambler and the encoder through the bricks' own tables and registers, serially --
and not the closed forms of sora_amd/csrc/k_mod.hip.  The one piece taken from elsewhere is the fixed-point IFFT<128> (Oracle().fft, pinned to the
reference's by tests/test_oracle_vs_reference.py); nothing here imports the library under test."""
import zlib

import numpy as np

BPSK_MOD = 10720                                                                 # mapper11a.hpp:8-11
MOD_OF = {1: BPSK_MOD, 2: int(BPSK_MOD / 1.414), 4: int(BPSK_MOD / 3.162), 6: int(BPSK_MOD / 6.481)}
CR_12, CR_23, CR_34 = 0, 1, 2
# rate -> (N_BPSC, code rate, N_DBPS, RATE field)            ieee80211a_cmn.h:65-149, ieee80211const.h:3-10
RATES = {6000: (1, CR_12, 24, 0xB), 9000: (1, CR_34, 36, 0xF), 12000: (2, CR_12, 48, 0xA), 18000: (2, CR_34, 72, 0xE),
         24000: (4, CR_12, 96, 0x9), 36000: (4, CR_34, 144, 0xD), 48000: (6, CR_23, 192, 0x8), 54000: (6, CR_34, 216, 0xC)}

PILOT_SGN = np.array([                                                           # pilot.hpp:10-28 (nonzero = polarity -1)
    0, 0, 0, 1, 1, 1, 0, 1, 1, 1, 1, 0, 0, 1, 0, 1, 1, 0, 0, 1, 0, 0, 1, 0, 0, 0, 0, 0, 0, 1, 0, 0,
    0, 1, 0, 0, 1, 1, 0, 0, 0, 1, 0, 1, 1, 1, 0, 1, 0, 1, 1, 0, 1, 1, 0, 0, 0, 0, 0, 1, 1, 0, 0, 1,
    1, 0, 1, 0, 1, 0, 0, 1, 1, 1, 0, 0, 1, 1, 1, 1, 0, 1, 1, 0, 1, 0, 0, 0, 0, 1, 0, 1, 0, 1, 0, 1,
    1, 1, 1, 1, 0, 1, 0, 0, 1, 0, 1, 0, 0, 0, 1, 1, 0, 1, 1, 1, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 0, 0], np.uint8)
LTS_POSITIVE = np.array([                                                        # ieee80211const.h:23-28
    0, 1, 0, 0, 1, 1, 0, 1, 0, 1, 0, 0, 0, 0, 0, 1, 1, 0, 0, 1, 0, 1, 0, 1, 1, 1, 1, 0, 0, 0, 0, 0,
    0, 0, 0, 0, 0, 0, 1, 1, 0, 0, 1, 1, 0, 1, 0, 1, 1, 1, 1, 1, 1, 0, 0, 1, 1, 0, 1, 0, 1, 1, 1, 1], np.uint8)

_ORACLE = None


def _ifft128(x):
    global _ORACLE
    if _ORACLE is None:
        from oracle.pyoracle import Oracle
        _ORACLE = Oracle()
    return _ORACLE.fft(np.ascontiguousarray(x, np.int16), n=128, inverse=True)


# ---- T11aSc (Brick11/src/scramble.hpp:170-261)
def _scr_lut():
    lut = np.zeros(128, np.uint8)
    for i in range(128):                                                         # :192-201
        x = (i << 1) & 0xFF
        for _ in range(8):
            o1 = ((x >> 1) ^ (x >> 4)) & 1
            x = (x >> 1) | (o1 << 7)
        lut[i] = x
    return lut


SCR_LUT = _scr_lut()


def scramble(data, seed, tail=None):
    """data uint8 [n]; the register starts at `seed` (the brick after Reset); byte `tail` (if < n) is TAIL_SCRAMBLE, every other DO_SCRAMBLE (:233-258)"""
    out = np.zeros(len(data), np.uint8)
    reg = int(seed) & 0xFF
    for i, b in enumerate(np.asarray(data, np.uint8)):
        reg = int(SCR_LUT[reg >> 1])
        code = int(b) ^ reg
        if tail is not None and i == tail:
            code &= 0xC0
        out[i] = code
    return out


# ---- TConvEncode_12 / _23 / _34 (conv_enc.hpp:6-330)
def _g0(x, s): return (x ^ (s >> 4) ^ (s >> 3) ^ (s >> 1) ^ s) & 1
def _g1(x, s): return (x ^ s ^ (s >> 3) ^ (s >> 4) ^ (s >> 5)) & 1


def _enc_luts():
    l12 = np.zeros((64, 256), np.uint16); l23 = np.zeros((64, 256), np.uint16); l34 = np.zeros((64, 64), np.uint16)
    for j in range(64):
        for i in range(256):
            s, x, o = j, i, 0                                                    # :31-45
            for _ in range(8):
                o = ((o >> 2) | (_g0(x, s) << 14) | (_g1(x, s) << 15)) & 0xFFFF
                s = (s >> 1) | ((x & 1) << 5); x >>= 1
            l12[j, i] = o
            s, x, o = j, i, 0                                                    # :113-131
            for _ in range(4):
                o = ((o >> 2) | (_g0(x, s) << 14) | (_g1(x, s) << 15)) & 0xFFFF
                s = (s >> 1) | ((x & 1) << 5); x >>= 1
                o = ((o >> 1) | (_g0(x, s) << 15)) & 0xFFFF
                s = (s >> 1) | ((x & 1) << 5); x >>= 1
            l23[j, i] = o >> 4
        for i in range(64):
            s, x, o = j, i, 0                                                    # :201-224
            for _ in range(2):
                o = ((o >> 2) | (_g0(x, s) << 14) | (_g1(x, s) << 15)) & 0xFFFF
                s = (s >> 1) | ((x & 1) << 5); x >>= 1
                o = ((o >> 1) | (_g0(x, s) << 15)) & 0xFFFF
                s = (s >> 1) | ((x & 1) << 5); x >>= 1
                o = ((o >> 1) | (_g1(x, s) << 15)) & 0xFFFF
                s = (s >> 1) | ((x & 1) << 5); x >>= 1
            l34[j, i] = o >> 8
    return l12, l23, l34


_ENC = None


def conv_encode(data, code_rate):
    """data uint8 [n] -> uint8: bursts of 1 / 2 / 3 bytes give 2 / 3 / 4; the register is 0 at the first byte; bytes behind the last whole burst stay queued"""
    global _ENC
    if _ENC is None:
        _ENC = _enc_luts()
    l12, l23, l34 = _ENC
    c = [int(v) for v in np.asarray(data, np.uint8)]
    out = []
    reg = 0
    if code_rate == CR_12:                                                       # :79-95
        for b in c:
            code = int(l12[reg, b]); out += [code & 255, code >> 8]; reg = b >> 2
    elif code_rate == CR_23:                                                     # :165-183
        for k in range(0, len(c) // 2 * 2, 2):
            s0 = int(l23[reg, c[k]]); s1 = int(l23[c[k] >> 2, c[k + 1]])
            out += [s0 & 255, (((s1 & 0xF) << 4) | (s0 >> 8)) & 255, (s1 >> 4) & 255]; reg = c[k + 1] >> 2
    else:                                                                        # :258-279
        for k in range(0, len(c) // 3 * 3, 3):
            c0 = c[k] & 0x3F; c1 = ((c[k + 1] & 0xF) << 2) | (c[k] >> 6); c2 = ((c[k + 2] & 0x3) << 4) | (c[k + 1] >> 4); c3 = c[k + 2] >> 2
            out += [int(l34[reg, c0]) & 255, int(l34[c0, c1]) & 255, int(l34[c1, c2]) & 255, int(l34[c2, c3]) & 255]; reg = c3
    return np.array(out, np.uint8)


# ---- T11aInterleave{BPSK,QPSK,QAM16,QAM64} = T11Interleave<48 N_BPSC, N_BPSC, 16, 11, 1> (interleave.hpp:16-114)
def interleave_map(n_bpsc):
    """r(k): where input bit k of a symbol goes (:41-50, I_SS = 1: the third permutation is the identity)"""
    n_cbps, n_s = 48 * n_bpsc, max(n_bpsc // 2, 1)
    k = np.arange(n_cbps)
    i = n_cbps // 16 * (k % 16) + k // 16
    return n_s * (i // n_s) + (i + n_cbps - 16 * i // n_cbps) % n_s


def _bits(b):
    return np.unpackbits(np.ascontiguousarray(b, np.uint8), axis=-1, bitorder="little")


def _bytes(bits):
    return np.packbits(np.ascontiguousarray(bits, np.uint8), axis=-1, bitorder="little")


def interleave(sym, n_bpsc):
    """sym uint8 [..., 6 n_bpsc] -> the same shape"""
    bits = _bits(sym)
    out = np.zeros_like(bits)
    out[..., interleave_map(n_bpsc)] = bits
    return _bytes(out)


# ---- TMap11a{BPSK,QPSK,QAM16,QAM64}<MOD> (mapper11a.hpp:8-300)
def _qam_level(rg, M, kmod):
    """InitQamMapLut (:16-43) for one axis: rg = its M bits, the first at bit 0"""
    g = int("{:0{w}b}".format(rg, w=M)[::-1], 2)                                 # BitReverseN
    b, sh = g, g >> 1
    while sh:                                                                    # GrayToBinary
        b ^= sh; sh >>= 1
    return np.int16(np.int32((b * 2 - ((1 << M) - 1)) * kmod).astype(np.int16))  # (short)(l * kmod)


def map11a(sym, n_bpsc, mod=0):
    """sym uint8 [n, 6 n_bpsc] -> int16 [n, 48, 2]; mod = the brick's MOD (0: the 802.11a amplitude of n_bpsc)"""
    mod = mod or MOD_OF[n_bpsc]
    bits = _bits(sym).reshape(len(sym), 48, n_bpsc)
    out = np.zeros((len(sym), 48, 2), np.int16)
    if n_bpsc == 1:                                                              # TMapperCore::MapBPSK (:72-86)
        out[..., 0] = np.where(bits[..., 0] == 1, mod, -mod)
        return out
    M = n_bpsc // 2
    lv = np.array([_qam_level(v, M, mod) for v in range(1 << M)], np.int16)
    w = 1 << np.arange(M)
    out[..., 0] = lv[(bits[..., :M] * w).sum(-1)]
    out[..., 1] = lv[(bits[..., M:] * w).sum(-1)]
    return out


# ---- T11aAddPilot<BPSK_MOD> (pilot.hpp:30-118)
class AddPilot:
    def __init__(self, bpsk_mod=BPSK_MOD):
        self.mod = bpsk_mod
        self.reset()

    def reset(self):
        self.index = 127                                                         # _init (:41-43)

    def process(self, car):
        """car int16 [n, 48, 2], symbols of one frame in order -> int16 [n, 64, 2]"""
        out = np.zeros((len(car), 64, 2), np.int16)                              # opin().zerobuf() (:54)
        for s, c in enumerate(np.asarray(car, np.int16)):
            k = 0
            for i in list(range(64 - 26, 64)) + list(range(1, 27)):              # :82-93
                if i in (64 - 7, 64 - 21, 7, 21):
                    continue
                out[s, i] = c[k]; k += 1
            p = -self.mod if PILOT_SGN[self.index] else self.mod                 # :95-108
            out[s, 7] = (p, 0); out[s, 21] = (-p, 0); out[s, 64 - 7] = (p, 0); out[s, 64 - 21] = (p, 0)
            self.index += 1                                                      # :69-71
            if self.index >= 127:
                self.index = 0
        return out


def add_pilot(car, bpsk_mod=BPSK_MOD):
    """the symbols of ONE frame from its first on (a brick after Reset)"""
    return AddPilot(bpsk_mod).process(car)


# ---- TIFFTx (fft.hpp:7-61)
def ifftx(bins, ifft128=None):
    """bins int16 [n, 64, 2] -> int16 [n, 160, 2]"""
    f = ifft128 or _ifft128
    bins = np.asarray(bins, np.int16)
    out = np.zeros((len(bins), 160, 2), np.int16)
    for s, b in enumerate(bins):
        t = np.zeros((128, 2), np.int16)
        t[:32] = b[:32]; t[96:] = b[32:]                                         # oversampled_ifft (:48-59)
        out[s, 32:] = np.asarray(f(t), np.int16) >> 4
        out[s, :32] = out[s, 128:]                                               # add GI (:31)
        for i in (0, 1, 158, 159):                                               # windowing (:34-39)
            out[s, i] >>= 1
    return out


# ---- TPackSample16to8 (brick/inc/stdbrick.hpp:415-445): _mm_packs_epi16
def pack16to8(x):
    return np.clip(np.asarray(x, np.int16), -128, 127).astype(np.int8)


# ---- TTS11aSrc (preamble11a.hpp:19-140)
def preamble(ifft128=None):
    """-> int16 [640, 2] at 40 MHz"""
    f = ifft128 or _ifft128
    sts_mod = int(1.0 * BPSK_MOD * 1.472) & 0xFFFF
    lut = np.zeros((640, 2), np.int16)
    x = np.zeros((128, 2), np.int16)
    for i, sg in zip((4, 8, 12, 16, 20, 24, 104, 108, 112, 116, 120, 124), (-1, -1, 1, 1, 1, 1, 1, -1, 1, -1, -1, 1)):
        x[i] = np.int16(np.int32(sg * sts_mod).astype(np.int16))
    t = np.asarray(f(x), np.int16) >> 4
    lut[:320] = np.tile(t, (3, 1))[:320]
    x = np.zeros((128, 2), np.int16)
    for i in range(1, 27):
        x[i, 0] = BPSK_MOD if LTS_POSITIVE[i] else -BPSK_MOD
    for i in range(64 - 26, 64):
        x[i + 64, 0] = BPSK_MOD if LTS_POSITIVE[i] else -BPSK_MOD
    t = np.asarray(f(x), np.int16) >> 4
    lut[384:512] = t; lut[512:640] = t; lut[320:384] = t[64:]
    for i in (0, 1, 318, 319, 320, 321, 638, 639):
        lut[i] >>= 1
    return lut


# ---- TBB11aSrc::Process (PHY_11a.hpp:111-202) and the whole graph
def fields(mpdu, rate_kbps):
    """-> (3 SIGNAL bytes; SERVICE + MPDU + FCS + tail + pad of whole symbols, two at 9 Mbps; index of the tail byte)"""
    nb, cr, nd, rc = RATES[rate_kbps]
    mpdu = bytes(mpdu)
    sig = rc | ((len(mpdu) + 4) << 5)
    sig |= (bin(sig).count("1") & 1) << 17                                       # ieee80211a_cmn.h:8-26
    ndp = nd * 2 if rate_kbps == 9000 else nd
    dbytes = 2 + len(mpdu) + 4 + 1
    rem = dbytes * 8 % ndp
    nbytes = dbytes + ((ndp - rem if rem else 0) + 7) // 8
    data = np.zeros(nbytes, np.uint8)
    data[2:2 + len(mpdu)] = np.frombuffer(mpdu, np.uint8)
    data[2 + len(mpdu):6 + len(mpdu)] = np.frombuffer((zlib.crc32(mpdu) & 0xFFFFFFFF).to_bytes(4, "little"), np.uint8)
    return np.array([sig & 255, (sig >> 8) & 255, sig >> 16], np.uint8), data, dbytes - 1


def frame16(mpdu, rate_kbps, seed=0xFF):
    """The 16-bit stream in front of TPackSample16to8 (or TUpsample40MTo44M): preamble, SIGNAL, data symbols -> int16 [n, 2] at 40 MHz"""
    nb, cr, nd, rc = RATES[rate_kbps]
    sig, data, tail = fields(mpdu, rate_kbps)
    sig_sym = map11a(interleave(conv_encode(sig, CR_12).reshape(1, 6), 1), 1)                     # unscrambled, the 6 Mbps path
    coded = conv_encode(scramble(data, seed, tail), cr)                                           # a fresh encoder register
    car = map11a(interleave(coded.reshape(-1, 6 * nb), nb), nb)
    sym = ifftx(add_pilot(np.concatenate([sig_sym, car])))
    return np.concatenate([preamble(), sym.reshape(-1, 2)])


def frame40(mpdu, rate_kbps, seed=0xFF):
    """CreatePreamble11a_40M + CreateModGraph11a_40M -> int8 [n, 2]"""
    return pack16to8(frame16(mpdu, rate_kbps, seed))


def frame44(mpdu, rate_kbps, seed=0xFF):
    """CreatePreamble11a_44M + CreateModGraph11a_44M -> int8 [n, 2]: the preamble's blocks 0..2 see the next block (one burst), every other block ends in x[160] = 0"""
    from tx11a44_model import up40to44
    x = frame16(mpdu, rate_kbps, seed)
    return pack16to8(up40to44(x, [b < 3 for b in range(len(x) // 160)]))
