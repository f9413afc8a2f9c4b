"""An integer model of the 802.11b modulation graph (kernel/bb/demod11/fb11bmod_config.hpp:28-50), brick by brick, with the preamble kind as
an argument: TBB11bSrc's PPDU bytes, TSc741, the DBPSK / DQPSK / CCK spreaders on the shared CF_DifferentialMap::last_phase,
TQuickPulseShaper's 20 taps and TPackSample16to8's saturating pack.  Everything is integer arithmetic.

preamble = 0 is the reference's frame: tests/test_11b_short_cpu.py pins it, sample for sample, to the compiled reference modulator and to
the recorded waveforms under tests/golden/.  preamble = 1 is the SHORT preamble the reference's source brick refuses (PHY_11b.hpp:115-119)
with the constants the reference already holds (kernel/inc/dot11_plcp.h): 7 SYNC bytes of 0x00, SFD 0x05CF, scrambler register 0x1B, SYNC
and SFD at 1 Mbps DBPSK, the six PLCP header bytes at 2 Mbps DQPSK, MPDU + FCS at 2, 5.5 or 11 Mbps -- the differential phase running on
through SFD, header and payload.  TEST INFRASTRUCTURE: what sora_hip_tx11b_pre is compared with."""
import zlib

import numpy as np

SIGNAL = {1000: 0x0A, 2000: 0x14, 5500: 0x37, 11000: 0x6E}
CHIPS_PER_BYTE = {1000: 88, 2000: 44, 5500: 16, 11000: 8}
# last_phase code <-> quarter turns counter-clockwise (0: 0, 1: -pi/2, 2: pi/2, 3: pi)
TURNS_OF_CODE = (0, 3, 1, 2)
CODE_OF_TURNS = (0, 2, 3, 1)
DQ = np.array([0, 3, 1, 2])                    # DQPSKEncode: dibit d0 + 2 d1 -> 1, -j, j, -1 (also CCK's phi1)
CQ = np.array([0, 2, 1, 3])                    # CCK 11 Mbps phi2..phi4: dibit -> 1, -1, j, -j
BARKER = np.array([0, 2, 0, 0, 2, 0, 0, 0, 2, 2, 2])   # quarter turns of the Barker word +1 -1 +1 +1 -1 +1 +1 +1 -1 -1 -1
TAPS = np.array([-1, 0, 3, 0, -6, 0, 34, 80, 102, 80, 34, 0, -6, 0, 3, 0, -1, 0, 1, 0], np.int64)     # pulse.hpp:254-293, i = 8 .. -11


def preamble_plan(preamble):
    """-> (SYNC bytes, SYNC value, SFD, scrambler register) of the kind"""
    if preamble == 0:
        return 16, 0xFF, 0xF3A0, 0x6C
    if preamble == 1:
        return 7, 0x00, 0x05CF, 0x1B
    raise ValueError("preamble kind %r" % (preamble,))


def samples(ln, rate, preamble=0):
    """the sample count of a frame, 0 for one that is not accepted"""
    if not 1 <= ln <= 4092 or rate not in SIGNAL or preamble not in (0, 1) or (preamble == 1 and rate == 1000):
        return 0
    hdr = 192 if preamble == 0 else 72 + 24
    return hdr * 44 + (ln + 4) * CHIPS_PER_BYTE[rate] * 4 + 24


def crc16(b):
    c = 0xFFFF
    for x in b:
        c ^= x
        for _ in range(8):
            c = (c >> 1) ^ 0x8408 if c & 1 else c >> 1
    return ~c & 0xFFFF


def ppdu_bytes(mpdu, rate, preamble=0):
    """TBB11bSrc (PHY_11b.hpp:80-200): SYNC, SFD (LSB first), SIGNAL, SERVICE, LENGTH in microseconds, CRC-16, MPDU, FCS"""
    nsync, sync, sfd, _ = preamble_plan(preamble)
    size = len(mpdu) + 4
    ext = 0
    if rate == 1000: us = size * 8
    elif rate == 2000: us = size * 4
    elif rate == 5500: us = (size * 16 + 10) // 11
    else:
        us = (size * 8 + 10) // 11
        ext = 1 if us * 11 - size * 8 >= 8 else 0
    h = bytes([SIGNAL[rate], ext << 7, us & 0xFF, us >> 8])
    c = crc16(h)
    return bytes([sync] * nsync + [sfd & 0xFF, sfd >> 8]) + h + bytes([c & 0xFF, c >> 8]) + bytes(mpdu) + zlib.crc32(bytes(mpdu)).to_bytes(4, "little")


def sc741(data, reg):
    """TSc741 (scramble.hpp:7-88): s[n] = b[n] ^ s[n-4] ^ s[n-7], the register holding the last seven output bits (oldest in bit 0)"""
    out = bytearray(len(data))
    for k, x in enumerate(data):
        o = 0
        for i in range(8):
            b = ((x >> i) ^ reg ^ (reg >> 3)) & 1
            reg = (reg >> 1) | (b << 6)
            o |= b << i
        out[k] = o
    return bytes(out)


def symbols(scr, rate, preamble=0):
    """the spreaders: per symbol the quarter turns it adds to last_phase and its chips' turns relative to the new phase -> (inc [S], list of
    (first symbol, chip offsets [n, chips]))"""
    nsync = preamble_plan(preamble)[0]
    v = np.frombuffer(scr, np.uint8).astype(np.int64)
    hb1 = nsync + 2 + (6 if preamble == 0 else 0)            # bytes through TBB11bDBPSKSpread before the payload
    hb = nsync + 8
    incs, offs = [], []

    def dbpsk(x):
        bits = (x[:, None] >> np.arange(8)) & 1
        incs.append((2 * bits).ravel()); offs.append(np.tile(BARKER, (8 * len(x), 1)))

    def dqpsk(x):
        d = (x[:, None] >> (2 * np.arange(4))) & 3
        incs.append(DQ[d].ravel()); offs.append(np.tile(BARKER, (4 * len(x), 1)))

    dbpsk(v[:hb1])
    if hb > hb1:
        dqpsk(v[hb1:hb])                                       # the short preamble's header: 2 Mbps
    p = v[hb:]
    if rate == 1000: dbpsk(p)
    elif rate == 2000: dqpsk(p)
    elif rate == 5500:                                         # TCCK5Encode: two symbols a byte, the second one odd
        w = np.stack([p & 15, p >> 4], 1).ravel(); odd = np.tile([0, 1], len(p))
        incs.append(DQ[w & 3] + 2 * odd)
        p2 = 1 + 2 * ((w >> 2) & 1); p3 = np.zeros_like(w); p4 = 2 * ((w >> 3) & 1)
        offs.append(np.stack([p2 + p3 + p4, p3 + p4, p2 + p4, p4 + 2, p2 + p3, p3, p2 + 2, 0 * w], 1))
    else:                                                      # TCCK11Encode: odd symbols of the PSDU get pi more
        odd = np.arange(len(p)) & 1
        incs.append(DQ[p & 3] + 2 * odd)
        p2, p3, p4 = CQ[(p >> 2) & 3], CQ[(p >> 4) & 3], CQ[(p >> 6) & 3]
        offs.append(np.stack([p2 + p3 + p4, p3 + p4, p2 + p4, p4 + 2, p2 + p3, p3, p2 + 2, 0 * p], 1))
    return incs, offs


def shape_and_pack(turns):
    """TQuickPulseShaper (pulse.hpp:254-340): sample s of chip step m = sum_j x[m - j] tap[4 j + s], five more steps at Flush;
    TPackSample16to8: saturate to 8 bits, the last burst of eight padded -> int8 [4 n + 24, 2]"""
    n = len(turns)
    re = np.array([1, 0, -1, 0], np.int64)[turns]; im = np.array([0, 1, 0, -1], np.int64)[turns]
    out = np.zeros((n + 6, 4, 2), np.int64)
    for j in range(5):
        for c, x in enumerate((re, im)):
            xp = np.zeros(n + 6, np.int64); xp[j:j + n] = x
            out[:, :, c] += xp[:, None] * TAPS[4 * j:4 * j + 4][None, :]
    return np.clip(out.reshape(-1, 2), -128, 127).astype(np.int8)


def tx11b(mpdu, rate, phase_in=0, preamble=0):
    """one frame -> (int8 [n, 2] COMPLEX8 at 44 MHz, last_phase after the frame).  phase_in: last_phase before it; the DBPSK spreader
    the frame starts with reads only its low bit (m_Coding_LUT[b][m_reg & 1]), so the frame starts at 0 or at pi."""
    assert samples(len(mpdu), rate, preamble), (len(mpdu), rate, preamble)
    scr = sc741(ppdu_bytes(mpdu, rate, preamble), preamble_plan(preamble)[3])
    incs, offs = symbols(scr, rate, preamble)
    phase = (2 * (phase_in & 1) + np.cumsum(np.concatenate(incs))) & 3
    turns, s0 = [], 0
    for o in offs:
        turns.append(((phase[s0:s0 + len(o), None] + o) & 3).ravel()); s0 += len(o)
    out = shape_and_pack(np.concatenate(turns))
    assert len(out) == samples(len(mpdu), rate, preamble)
    return out, CODE_OF_TURNS[int(phase[-1])]
