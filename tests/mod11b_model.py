"""Integer models of the bricks of the 802.11b modulation graph (kernel/bb/demod11/fb11bmod_config.hpp:28-50), one function per brick with the brick's state as an
explicit argument and result, each written from the brick's source -- its look-up tables built the way the brick builds them, its Process loop walked unit by unit:
    ppdu           TBB11bSrc           PHY_11b.hpp:19-206        (the short preamble with the constants of kernel/inc/dot11_plcp.h, as tests/tx11b_model.py)
    sc741          TSc741              scramble.hpp:7-88
    dbpsk_spread   TBB11bDBPSKSpread   barkerspread.hpp:9-111
    dqpsk_spread   TBB11bDQPSKSpread   barkerspread.hpp:113-225
    cck5_encode    TCCK5Encode         cck.hpp:880-953
    cck11_encode   TCCK11Encode        cck.hpp:782-870
    quick_shape_loop / pulse_shape     TQuickPulseShaper, pulse.hpp:254-384: the brick's loop literally, and the same in whole-array form
    pack16to8      TPackSample16to8
mod11b composes them as CreateModGraph does, TBB11bMRSelect's routing included.  tests/test_mod11b_model_cpu.py holds the composition to tests/tx11b_model.py (and
through it to the compiled reference modulator).  TEST INFRASTRUCTURE: what the stage entry points sora_hip_*11b of k_mod11b.hip are compared with."""
import math
import zlib

import numpy as np

from tx11b_model import CHIPS_PER_BYTE, SIGNAL, TAPS, preamble_plan, samples

# ---------------------------------------------------------------- TBB11bSrc


def crc16(b):
    """CalcCRC16: reflected 0x8408 from 0xFFFF, inverted"""
    c = 0xFFFF
    for x in b:
        c ^= x
        for _ in range(8):
            c = (c >> 1) ^ 0x8408 if c & 1 else c >> 1
    return ~c & 0xFFFF


def ppdu(mpdu, rate, preamble=0):
    """-> the bytes the source brick emits: m_header (sync_data, sfd, plcp: Signal, Service, Length, CRC), the MPDU, crc32"""
    nsync, sync, sfd, _ = preamble_plan(preamble)
    size = len(mpdu) + 4                                                         # GetPPDULength
    ext = 0
    if rate == 1000: us = size << 3
    elif rate == 2000: us = size << 2
    elif rate == 5500: us = ((size << 4) - 1) // 11 + 1
    else:
        us = ((size << 3) - 1) // 11 + 1
        if us * 11 - (size << 3) >= 8:
            ext += 1
    plcp = bytes([SIGNAL[rate], ext << 7, us & 0xFF, (us >> 8) & 0xFF])
    c = crc16(plcp)
    return bytes([sync] * nsync) + bytes([sfd & 0xFF, sfd >> 8]) + plcp + bytes([c & 0xFF, c >> 8]) + bytes(mpdu) + zlib.crc32(bytes(mpdu)).to_bytes(4, "little")


# ---------------------------------------------------------------- TSc741
def _sc741_lut():
    lut = np.zeros((256, 128), np.uint8)
    for i in range(256):
        for j in range(128):
            x, s, o = i, j, 0
            for _ in range(8):
                o1 = (x ^ s ^ (s >> 3)) & 1
                s = (s >> 1) | (o1 << 6)
                o = (o >> 1) | (o1 << 7)
                x >>= 1
            lut[i, j] = o
    return lut


_LUTS = {}


def _lut(name, make):
    if name not in _LUTS:
        _LUTS[name] = make()
    return _LUTS[name]


def sc741(data, reg):
    """-> (bytes, m_Reg).  reg: 7 bits (the brick's table has 128 columns)"""
    lut = _lut("sc741", _sc741_lut)
    reg &= 0x7F
    out = bytearray(len(data))
    for k, b in enumerate(data):
        code = int(lut[b, reg])
        reg = code >> 1
        out[k] = code
    return bytes(out), reg


# ---------------------------------------------------------------- the Barker spreaders
BARKER11 = [1, -1, 1, 1, -1, 1, 1, 1, -1, -1, -1]


def _dbpsk_luts():
    coding = np.zeros((256, 2), np.uint8)
    spread = np.zeros((256, 88, 2), np.int8)
    for i in range(256):
        x, phase, v = i, 0, 0
        for k in range(8):
            phase = phase ^ 1 if x & 1 else phase
            v |= phase << k
            x >>= 1
        coding[i, 0] = v; coding[i, 1] = v ^ 0xFF
        x = i
        for j in range(8):
            c = -1 if x & 1 else 1
            x >>= 1
            for k in range(11):
                spread[i, j * 11 + k] = (c * BARKER11[k], 0)
    return coding, spread


def dbpsk_spread(data, last_phase):
    """-> (int8 [88 n, 2], last_phase)"""
    coding, spread = _lut("dbpsk", _dbpsk_luts)
    out = np.zeros((len(data), 88, 2), np.int8)
    for k, b in enumerate(data):
        code = int(coding[b, last_phase & 1])
        last_phase = code >> 7
        last_phase = (last_phase << 1) | last_phase
        out[k] = spread[code]
    return out.reshape(-1, 2), last_phase


def _dqpsk_luts():
    rotate = [[0, 1, 2, 3], [1, 3, 0, 2], [2, 0, 3, 1], [3, 2, 1, 0]]
    coding = np.zeros((256, 4), np.uint8)
    spread = np.zeros((256, 44, 2), np.int8)
    for i in range(256):
        for j in range(4):
            x, phase, v = i, j, 0
            for k in range(0, 8, 2):
                phase = rotate[phase][x & 3]
                v |= phase << k
                x >>= 2
            coding[i, j] = v
        x = i
        for j in range(4):
            re, im = [(1, 0), (0, -1), (0, 1), (-1, 0)][x & 3]
            x >>= 2
            for k in range(11):
                spread[i, j * 11 + k] = (re * BARKER11[k], im * BARKER11[k])
    return coding, spread


def dqpsk_spread(data, last_phase):
    """-> (int8 [44 n, 2], last_phase)"""
    coding, spread = _lut("dqpsk", _dqpsk_luts)
    out = np.zeros((len(data), 44, 2), np.int8)
    for k, b in enumerate(data):
        code = int(coding[b, last_phase & 3])
        last_phase = code >> 6
        out[k] = spread[code]
    return out.reshape(-1, 2), last_phase


# ---------------------------------------------------------------- the CCK encoders (Gaussian integers as Python complex numbers: exact)
DQPSK_ENCODE = [1, -1j, 1j, -1]
CCK11_D3D2 = [1, -1, 1j, -1j]
CCK5_D3D2 = [[1j, 1, 1j, -1, 1j, 1, -1j, 1], [-1j, 1, -1j, -1, -1j, 1, 1j, 1], [-1j, -1, -1j, 1, 1j, 1, -1j, 1], [1j, -1, 1j, 1, -1j, 1, 1j, 1]]


def _c8(values):
    return np.array([(int(v.real), int(v.imag)) for v in values], np.int8)


def _cck5_lut():
    val = np.zeros((256, 4, 16, 2), np.int8); ref = np.zeros((256, 4), np.uint8)
    for d in range(256):
        for prev in range(4):
            v = [0] * 16
            halfd = d % 16
            m1 = DQPSK_ENCODE[halfd % 4]; m0 = DQPSK_ENCODE[prev]
            for i in range(8):
                v[i] = m0 * m1 * CCK5_D3D2[halfd // 4][i]
            halfd = d // 16
            m1 = DQPSK_ENCODE[halfd % 4]; m0 = v[7]
            for i in range(8):
                v[i + 8] = -m0 * m1 * CCK5_D3D2[halfd // 4][i]
            val[d, prev] = _c8(v); ref[d, prev] = DQPSK_ENCODE.index(v[15])
    return val, ref


def cck5_encode(data, last_phase):
    """-> (int8 [16 n, 2], last_phase).  The brick indexes its table with last_phase as it is: 0..3"""
    val, ref = _lut("cck5", _cck5_lut)
    last_phase &= 3
    out = np.zeros((len(data), 16, 2), np.int8)
    for k, b in enumerate(data):
        out[k] = val[b, last_phase]
        last_phase = int(ref[b, last_phase])
    return out.reshape(-1, 2), last_phase


def _cck11_lut():
    val = np.zeros((256, 4, 2, 8, 2), np.int8); ref = np.zeros((256, 4, 2), np.uint8)
    for d in range(256):
        for prev in range(4):
            m0 = DQPSK_ENCODE[prev]; m1 = DQPSK_ENCODE[d % 4]
            m2 = CCK11_D3D2[(d >> 2) % 4]; m3 = CCK11_D3D2[(d >> 4) % 4]; m4 = CCK11_D3D2[(d >> 6) % 4]
            v = [m0 * m1 * m2 * m3 * m4, m0 * m1 * m3 * m4, m0 * m1 * m2 * m4, -m0 * m1 * m4, m0 * m1 * m2 * m3, m0 * m1 * m3, -m0 * m1 * m2, m0 * m1]
            odd = [-x for x in v]                                                # all odd-numbered symbols of the PSDU are given an extra 180 degree rotation
            val[d, prev, 0] = _c8(v); val[d, prev, 1] = _c8(odd)
            ref[d, prev, 0] = DQPSK_ENCODE.index(v[7]); ref[d, prev, 1] = DQPSK_ENCODE.index(odd[7])
    return val, ref


def cck11_encode(data, last_phase, is_even):
    """-> (int8 [8 n, 2], last_phase, bEven).  is_even is the brick's bEven: 0 after Reset, the index of the table's rotated half"""
    val, ref = _lut("cck11", _cck11_lut)
    last_phase &= 3; is_even &= 1
    out = np.zeros((len(data), 8, 2), np.int8)
    for k, b in enumerate(data):
        out[k] = val[b, last_phase, is_even]
        last_phase = int(ref[b, last_phase, is_even])
        is_even = (is_even + 1) & 1
    return out.reshape(-1, 2), last_phase, is_even


# ---------------------------------------------------------------- TQuickPulseShaper
def _taps():
    """_init_taps: lut[j][k] for the rows j = 0..4 and the columns k = 0..3 (each column stands twice in the brick's table, for re and im)"""
    pi, power_level = 3.141593, 80
    lut = np.zeros((5, 4), np.int64)
    ii = 8
    for j in range(5):
        for k in range(4):
            i = ii - k
            x = 1.0 if i in (1, -1) else 4 * math.cos(pi * i / 2) / pi / (1 - i * i)
            lut[j, k] = int(x * power_level + .5)                               # (short): truncation towards zero
        ii -= 4
    return lut


def _wrap16(a):
    return ((np.asarray(a, np.int64) + 32768) & 0xFFFF) - 32768


def quick_shape_loop(x, temps, flush=False):
    """The brick literally.  x int8 [n, 2]; temps int16 [4, 4, 2] = m_temps[0..3] -> (int16 [4 N, 2], m_temps[0..3]); N = n, and five more at Flush"""
    taps = _lut("taps", _taps)
    stores = np.zeros((5, 4, 2), np.int64); stores[:4] = temps                   # m_temps[tap_cnt]: the fifth row is never written
    xs = [tuple(int(v) for v in s) for s in np.asarray(x).reshape(-1, 2)] + ([(0, 0)] * 5 if flush else [])
    out = np.zeros((len(xs), 4, 2), np.int64)
    for m, (re, im) in enumerate(xs):
        vi = np.array([re, im], np.int64)[None, :]                               # set_all(m_input, ss)
        tt = _wrap16(vi * taps[0][:, None])                                      # mul_low
        out[m] = _wrap16(tt + stores[0])
        for i in range(4):
            tt = _wrap16(vi * taps[i + 1][:, None])
            stores[i] = _wrap16(stores[i + 1] + tt)
    return out.reshape(-1, 2).astype(np.int16), stores[:4].astype(np.int16)


def pulse_shape(x, temps, flush=False):
    """quick_shape_loop over whole arrays (a frame at 1 Mbps has 362560 chips): burst m is the stored partial sum, if the call started with one for it, plus the
    products of the inputs m - 4 .. m; the stores left are the bursts the brick has begun.  Held to the loop by tests/test_mod11b_model_cpu.py."""
    taps = _lut("taps", _taps)
    x = np.asarray(x, np.int64).reshape(-1, 2)
    n = len(x) + (5 if flush else 0)
    xp = np.zeros((n + 8, 2), np.int64); xp[4:4 + len(x)] = x                    # x[m] at xp[m + 4]
    acc = np.zeros((n + 4, 4, 2), np.int64)
    acc[:4] = temps
    for j in range(5):
        acc += xp[4 - j:4 - j + n + 4, None, :] * taps[j][None, :, None]
    out = _wrap16(acc[:n])                                                       # (xp is 0 behind the inputs: rows n .. n + 3 hold the bursts begun so far)
    return out.reshape(-1, 2).astype(np.int16), _wrap16(acc[n:n + 4]).astype(np.int16)


def pack16to8(x):
    """TPackSample16to8: saturate to 8 bits, no shift"""
    return np.clip(np.asarray(x, np.int64), -128, 127).astype(np.int8)


# ---------------------------------------------------------------- CreateModGraph
def mod11b(mpdu, rate, phase_in=0, preamble=0):
    """one frame through the bricks -> (int8 [n, 2] COMPLEX8 at 44 MHz, last_phase after it): what tx11b_model.tx11b returns"""
    assert samples(len(mpdu), rate, preamble), (len(mpdu), rate, preamble)
    nsync, _, _, seed = preamble_plan(preamble)
    scr, _ = sc741(ppdu(mpdu, rate, preamble), seed)
    hb1 = nsync + 2 + (6 if preamble == 0 else 0)                                # TBB11bMRSelect: the bytes in front of the payload go to the DBPSK spreader,
    hb = nsync + 8                                                               # the short preamble's PLCP header to the DQPSK one
    chips = []
    c, phase = dbpsk_spread(scr[:hb1], phase_in); chips.append(c)
    if hb > hb1:
        c, phase = dqpsk_spread(scr[hb1:hb], phase); chips.append(c)
    if rate == 1000: c, phase = dbpsk_spread(scr[hb:], phase)
    elif rate == 2000: c, phase = dqpsk_spread(scr[hb:], phase)
    elif rate == 5500: c, phase = cck5_encode(scr[hb:], phase)
    else: c, phase, _ = cck11_encode(scr[hb:], phase, 0)
    chips.append(c)
    wide, _ = pulse_shape(np.concatenate(chips), np.zeros((4, 4, 2), np.int16), flush=True)
    wide = np.concatenate([wide, np.zeros((-len(wide) % 8, 2), np.int16)])       # the last burst of eight of TPackSample16to8, padded
    assert (np.asarray(_lut("taps", _taps)).ravel() == TAPS).all() and CHIPS_PER_BYTE[rate] * (len(mpdu) + 4) == len(c)
    return pack16to8(wide), phase
