"""The 40 MHz HT receiver's stage entry points (sora_hip_*_ht40, include/sora_hip.h) as a per-brick integer model: each function is one stage on one frame, symbol or
stream over numpy arrays, built on the oracle library's exported, reference-pinned bricks (so_freq_comp11n, so_fft128, so_mimo_comp11n on halves, so_dsp_atan16, so_demap11n,
so_viterbi_frame_ex, so_desc_sink) with the glue in numpy; the carrier plan, the HT-LTF signs and the permutation come from oracle/ht40_data_model.py.  The two float solves
-- TMimoChannelEst's inverse and the unbiased MMSE -- are restated in numpy float32, operation for operation (numpy rounds every elementwise operation on its own: no
contraction); tests/test_ht40_stage_model_cpu.py holds the first to so_ht40_zf_weights bit for bit and the second to a float64 evaluation within +-1 LSB.  ModelOps runs
sora_amd.capi.rx_ht40_stages -- the composition the GPU runs -- over these bricks.  It never reads the library under test.  TEST INFRASTRUCTURE: only tests/ use it."""
import ctypes
import zlib

import numpy as np

from oracle import ht40_data_model as dm
from sora_amd import capi

E_FRAME_OK, E_CRC32_FAIL = 1, 0x80000006
PILOT_BINS = [int(b) for b in dm.PILOT_BINS]
DATA_BINS = np.asarray(dm.DATA_BINS, np.int64)
OCC = np.asarray(dm.OCCUPIED_BINS, np.int64)
# so_demap11n's carrier order over a 64-bin burst: -28..-1 then 1..28 without the pilots at +-7, +-21
_SLOTS52 = [i for i in list(range(36, 64)) + list(range(1, 29)) if i not in (43, 57, 7, 21)]


def _c16(x):
    return np.ascontiguousarray(x, np.int16).reshape(-1, 2)


def _sat16(v):
    return np.clip(v, -32768, 32767)


def _w16(v):
    return ((np.asarray(v, np.int64) + 32768) & 0xFFFF) - 32768


def oracle():
    O = dm.oracle()
    O.L.so_dsp_atan16.restype = ctypes.c_int16
    return O


# ------------------------------------------------------------------ front end
def downsample(x, n, m0=0):
    """kept sample m = x[2m], negated with int16 saturation when m0 + m is odd -> int16 [n, 2]"""
    k = _c16(x)[0:2 * n:2].astype(np.int64)
    assert len(k) == n
    odd = ((np.arange(n) + m0) & 1).astype(bool)
    k[odd] = _sat16(-k[odd])
    return k.astype(np.int16)


def noise_S(l0, l1):
    """l_r int16 [128, 2] = the two L-LTF symbols of chain r after FFT<64> -> S, the exact integer (tests/cxx/ht40_front_model.c's loop)"""
    S = 0
    for l in (l0, l1):
        a = _c16(l).astype(np.int64)
        for k in range(1, 64):
            if 27 <= k < 38:
                continue
            dr = int(a[k, 0] - a[64 + k, 0]); di = int(a[k, 1] - a[64 + k, 1])
            S += dr * dr + di * di
    return S


def noise_var(S):
    """S / 416 (float64 of an integer below 2^53), rounded once to float32"""
    return np.float32(S / 416.0)


# ------------------------------------------------------------------ data field
def data_symbol(x, nsym):
    """nsym symbols of 160 samples -> their samples 32..159, [nsym * 128, 2]"""
    return _c16(x)[:160 * nsym].reshape(nsym, 160, 2)[:, 32:].reshape(-1, 2).copy()


def mimo_h(l0, l1):
    """l_r int16 [256, 2] = HT-LTF 1 | HT-LTF 2 of chain r after FFT<128> -> h int16 [4, 128, 2] (h00, h01, h10, h11): TMimoChannelEst's combination (p - q) / 2,
    (p + q) / 2, negated where the HT-LTF is -1; 0 outside the occupied carriers"""
    h = np.zeros((4, 128, 2), np.int64)
    for r, l in enumerate((l0, l1)):
        a = _c16(l).astype(np.int64); p, q = a[:128], a[128:]
        h[2 * r] = _sat16(p - q) >> 1; h[2 * r + 1] = _sat16(p + q) >> 1
    neg = np.asarray(dm.LTF_SIGN) != 1
    h[:, neg] = _w16(-h[:, neg])
    out = np.zeros((4, 128, 2), np.int16); out[:, OCC] = h[:, OCC]
    return out


def _cf(v):
    return v[..., 0].astype(np.float32), v[..., 1].astype(np.float32)


def _mul(a, b):
    """vcf mul: every product and every sum rounded on its own"""
    return (a[0] * b[0]) - (a[1] * b[1]), (a[1] * b[0]) + (a[0] * b[1])


def _pack(ws):
    """cvtps2dq (nearest even; 0x80000000 out of range or NaN) then packssdw -> int16 [4, n, 2]"""
    out = np.zeros((4, len(ws[0][0]), 2), np.int16)
    for m, (re, im) in enumerate(ws):
        for c, v in enumerate((re, im)):
            ok = (v >= np.float32(-2147483648.0)) & (v < np.float32(2147483648.0))
            r = np.where(ok, np.rint(np.where(ok, v, 0)).astype(np.int64), -2147483648)
            out[m, :, c] = _sat16(r).astype(np.int16)
    return out


def zf_solve(h):
    """mimo_inverse (sora_matrix.h:134-148,305-313) on h int16 [4, n, 2], float32 -> int16 [4, n, 2]"""
    f32 = np.float32
    with np.errstate(all="ignore"):
        a00, a01, a10, a11 = (_cf(h[k]) for k in range(4))
        ad, bc = _mul(a00, a11), _mul(a01, a10)
        det = (ad[0] - bc[0], ad[1] - bc[1])
        n = ((det[0] * det[0]) + (det[1] * det[1])) / f32(65536.0)
        ds = (det[0], -det[1]); m01 = (-a01[0], -a01[1]); m10 = (-a10[0], -a10[1])
        rr = [_mul(a11, ds), _mul(m01, ds), _mul(m10, ds), _mul(a00, ds)]
        return _pack([(r[0] / n, r[1] / n) for r in rr])


def mmse_solve(h, s2, dtype=np.float32):
    """the handle's unbiased MMSE (k_ht40.hip's solve), operation for operation in `dtype` -> int16 [4, n, 2]; dtype float64: the evaluation the +-1 LSB tolerance is
    stated against"""
    f = dtype
    with np.errstate(all="ignore"):
        a00, a01, a10, a11 = ((h[k][..., 0].astype(f), h[k][..., 1].astype(f)) for k in range(4))
        s2 = f(s2)
        cj = lambda a: (a[0], -a[1])
        n2 = lambda a: (a[0] * a[0]) + (a[1] * a[1])
        g00 = (n2(a00) + n2(a10)) + s2; g11 = (n2(a01) + n2(a11)) + s2
        t0, t1 = _mul(cj(a00), a01), _mul(cj(a10), a11)
        g01 = (t0[0] + t1[0], t0[1] + t1[1])
        det = ((g00 * g11) - n2(g01)) / f(65536.0)

        def row0(hc0, hc1):
            u = _mul(g01, hc1); return ((g11 * hc0[0]) - u[0]) / det, ((g11 * hc0[1]) - u[1]) / det

        def row1(hc0, hc1):
            u = _mul(cj(g01), hc0); return ((g00 * hc1[0]) - u[0]) / det, ((g00 * hc1[1]) - u[1]) / det
        w00, w01 = row0(cj(a00), cj(a01)), row0(cj(a10), cj(a11))
        w10, w11 = row1(cj(a00), cj(a01)), row1(cj(a10), cj(a11))
        e0, e1, e2, e3 = _mul(w00, a00), _mul(w01, a10), _mul(w10, a01), _mul(w11, a11)
        b0 = (e0[0] + e1[0]) / f(65536.0); b1 = (e2[0] + e3[0]) / f(65536.0)
        ws = [(w00[0] / b0, w00[1] / b0), (w01[0] / b0, w01[1] / b0), (w10[0] / b1, w10[1] / b1), (w11[0] / b1, w11[1] / b1)]
        if dtype is np.float64:                                                # (rounded like the float path: nearest even, saturating)
            out = np.zeros((4, len(b0), 2), np.int16)
            for m, (re, im) in enumerate(ws):
                for c, v in enumerate((re, im)):
                    ok = np.isfinite(v) & (np.abs(v) < 2147483648.0)
                    out[m, :, c] = _sat16(np.where(ok, np.rint(np.where(ok, v, 0)), -2147483648.0)).astype(np.int16)
            return out
        return _pack(ws)


def mimo_est(l0, l1, s2=0.0):
    """-> (h, w) int16 [4, 128, 2]: the stage's two outputs, 0 outside the occupied carriers"""
    h = mimo_h(l0, l1)
    w = np.zeros((4, 128, 2), np.int16)
    hh = np.ascontiguousarray(h[:, OCC])
    w[:, OCC] = zf_solve(hh) if float(s2) == 0.0 else mmse_solve(hh, np.float32(s2))
    return h, w


def mimo_comp(w, y0, y1):
    """x = sat((W y) >> 9) over 128 bins through so_mimo_comp11n on the two halves -> (x0, x1) int16 [128, 2]"""
    O = oracle(); w = np.asarray(w, np.int16).reshape(4, 128, 2); y0 = _c16(y0); y1 = _c16(y1)
    xs = np.zeros((2, 128, 2), np.int16)
    for half in range(2):
        sl = slice(64 * half, 64 * half + 64)
        hinv = np.stack([np.concatenate([w[0, sl], w[1, sl]]), np.concatenate([w[2, sl], w[3, sl]])])
        xs[0, sl], xs[1, sl] = O.mimo_comp11n(hinv, y0[sl], y1[sl])
    return xs[0], xs[1]


def pilot_inc(x0, x1):
    """the increment of theta one symbol's two detected streams give"""
    O = oracle(); t = []
    for x in (_c16(x0), _c16(x1)):
        tot = sum(int(O.L.so_dsp_atan16(ctypes.c_int16(int(x[b, 0])), ctypes.c_int16(int(x[b, 1])))) for b in PILOT_BINS)
        t.append(int(_w16(int(tot / 6))))                                     # C truncation
    return int(_w16((t[0] + t[1]) >> 1))


def demap(x, nb):
    """T11nDemap* over the 108 data carriers in DATA_BINS order, I bits then Q bits per carrier: so_demap11n on bursts that hold 52 of them -> uint8 [108 nb]"""
    O = oracle(); x = _c16(x); raw = []
    for c0 in range(0, 108, 52):
        bins = DATA_BINS[c0:c0 + 52]
        burst = np.zeros((64, 2), np.int16); burst[_SLOTS52[:len(bins)]] = x[bins]
        raw.append(O.demap11n(nb, burst)[:len(bins) * nb])
    return np.concatenate(raw)


def deinterleave(s, nb, iss):
    return np.ascontiguousarray(s, np.uint8)[dm.permutation(nb, iss)]


def stream_join(s0, s1, nb):
    """[n, 108 nb] x 2 -> [n, 216 nb], groups of s = max(nb / 2, 1) bytes alternating stream 0, stream 1"""
    s = max(nb // 2, 1)
    a = np.ascontiguousarray(s0, np.uint8).reshape(-1, 108 * nb // s, 1, s); b = np.ascontiguousarray(s1, np.uint8).reshape(-1, 108 * nb // s, 1, s)
    return np.concatenate([a, b], axis=2).reshape(-1, 216 * nb)


def frame_sink(b, length):
    """TBB11aFrameSink on `length` descrambled bytes -> (error_code, frame_crc32); below 4 bytes the brick never decides"""
    if length < 4:
        return 0, 0
    b = bytes(bytearray(b[:length]))
    fcs = int.from_bytes(b[-4:], "little")
    return (E_FRAME_OK if zlib.crc32(b[:-4]) == fcs else E_CRC32_FAIL), fcs


class ModelOps:
    """sora_amd.capi.rx_ht40_stages' bricks: the batch tables walked frame by frame over numpy buffers"""
    VOUT = 4352

    def __init__(self):
        self.o = oracle(); self.comp = None

    @staticmethod
    def _u(a):
        return np.asarray(a).astype(np.int64) & 0xFFFFFFFF

    def host(self, a):
        return np.asarray(a)

    def state(self, rec):
        return np.array(rec, np.int16)

    def concat(self, parts):
        return np.concatenate([np.asarray(p).reshape(-1) for p in parts])

    def freq_comp(self, x0, x1, first, nbursts, state):
        if self.comp is None:
            self.comp = (np.zeros_like(x0), np.zeros_like(x1))
        for f, (a, k) in enumerate(zip(self._u(first), self._u(nbursts))):
            if k:
                state[f], self.comp[0][a:a + 8 * k], self.comp[1][a:a + 8 * k] = self.o.freq_comp11n(state[f], x0[a:a + 8 * k], x1[a:a + 8 * k])
        return self.comp

    def data_symbol(self, x0, x1, first, nsym, out_first, total):
        o0 = np.zeros((total * 128, 2), np.int16); o1 = np.zeros_like(o0)
        for a, k, o in zip(self._u(first), self._u(nsym), self._u(out_first)):
            o0[128 * o:128 * (o + k)] = data_symbol(x0[a:a + 160 * k], k); o1[128 * o:128 * (o + k)] = data_symbol(x1[a:a + 160 * k], k)
        return o0, o1

    def fft128(self, x):
        return np.concatenate([self.o.fft(s, 128) for s in x.reshape(-1, 128, 2)]).reshape(-1, 2).astype(np.int16)

    def mimo_est(self, l0, l1, noise_var):
        r = [mimo_est(a, b, s2) for a, b, s2 in zip(l0.reshape(-1, 256, 2), l1.reshape(-1, 256, 2), noise_var)]
        return np.stack([h for h, _ in r]), np.stack([w for _, w in r])

    def mimo_comp(self, w, y0, y1, frame_index):
        r = [mimo_comp(w[f], a, b) for f, a, b in zip(self._u(frame_index), y0.reshape(-1, 128, 2), y1.reshape(-1, 128, 2))]
        return np.stack([a for a, _ in r]), np.stack([b for _, b in r])

    def pilot_track(self, x0, x1, first, nsym, state):
        th = np.zeros(len(x0), np.int16)
        for f, (a, k) in enumerate(zip(self._u(first), self._u(nsym))):
            for s in range(a, a + k):
                state[f, 16:] = _w16(state[f, 16:].astype(np.int64) + pilot_inc(x0[s], x1[s])).astype(np.int16)
                th[s] = state[f, 16]
        return th

    def demap(self, x, nb):
        return np.stack([demap(s, nb) for s in x.reshape(-1, 128, 2)])

    def deinterleave(self, s, nb, iss):
        return np.stack([deinterleave(r, nb, iss) for r in s])

    def stream_join(self, s0, s1, nb):
        return stream_join(s0, s1, nb)

    def viterbi(self, soft, soft_off, nsoft, lens, code_rate):
        out = np.zeros((len(lens), self.VOUT), np.uint8)
        for i, (a, k, n) in enumerate(zip(self._u(soft_off), self._u(nsoft), lens)):
            d = self.o.viterbi_frame_ex(soft[a:a + k], int(code_rate), int(n), 192, 36)
            out[i, :int(n) + 2] = d[:int(n) + 2]
        return out.reshape(-1)

    def desc(self, dec, off, lens, out_off, total):
        out = np.zeros(max(total, 1), np.uint8)
        for a, n, o in zip(self._u(off), self._u(lens), self._u(out_off)):
            out[o:o + n] = self.o.desc_sink(dec[a:a + n + 2], int(n))[1]
        return out

    def frame_sink(self, x, off, lens):
        return np.array([frame_sink(x[a:a + n], int(n)) for a, n in zip(self._u(off), self._u(lens))], np.int64).reshape(-1, 2)


def by_stages(iq, frames, coding=0):
    """iq int16 [2, n, 2] -> sora_amd.capi.rx_ht40_stages over the model's bricks"""
    iq = np.ascontiguousarray(iq, np.int16)
    return capi.rx_ht40_stages(ModelOps(), iq[0], iq[1], frames, coding)


def front_ops():
    """sora_amd.capi.rx_ht40_front_stages' bricks: tests/rx11n_stage_model.ModelOps (the 802.11n stages' model) with the front end's two own stages"""
    import rx11n_stage_model as n

    class FrontOps(n.ModelOps):
        data_symbol11n = n.ModelOps.data_symbol

        def downsample(self, iq0, iq1, first, nn, m0, out_first, total):
            o = [np.zeros((total, 2), np.int16), np.zeros((total, 2), np.int16)]
            for a, k, p, of in zip(self._u(first), self._u(nn), self._u(m0), self._u(out_first)):
                o[0][of:of + k] = downsample(np.asarray(iq0)[a:], k, p); o[1][of:of + k] = downsample(np.asarray(iq1)[a:], k, p)
            return o[0], o[1]

        def noise_var(self, l0, l1):
            S = [noise_S(a, b) for a, b in zip(np.asarray(l0).reshape(-1, 128, 2), np.asarray(l1).reshape(-1, 128, 2))]
            return np.array(S, np.int64), np.array([noise_var(s) for s in S], np.float32)
    n.load()
    return FrontOps()


def front_by_stages(iq0, iq1, descs, coding=0):
    return capi.rx_ht40_front_stages(front_ops(), _c16(iq0), _c16(iq1), descs, coding)
