"""The bricks that complete the 802.11n receive graph, one by one: tests/cxx/rx11n_stage_model.c (TCCA11n, T11aDesc, TBB11aFrameSink in the reference bricks' own
form) compiled beside its source and bound here, T11nDataSymbol and TStreamJoin + TStreamConcat as numpy index arithmetic, all over the records of include/sora_hip.h
as int32 words.  `first_events` composes the whole graph through sora_amd.capi.rx11n_stages -- the very walk sora_amd.rx11n_by_stages runs over the GPU's stages --
with these bricks and, for the eleven older ones, the reference-pinned functions of oracle.pyoracle.Oracle in place of the kernels.
TEST INFRASTRUCTURE: only tests/ and tools/bench_11n_rx_stages.py use it."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

from oracle import pyoracle
from sora_amd import capi

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cxx", "rx11n_stage_model.c")
WORDS = capi.CCA11N_WORDS
BRANCHES = ("detect_lane0", "detect_lane1", "detect_lane2", "detect_lane3", "fake_plateau", "too_many_peaks", "timeout_rearmed", "timeout_standing", "llmax_ring",
            "sqnorm_wrapped", "silent_sample", "slipped_ring_entry")

_lib = None


def _build():
    """-> path of the compiled model (tests/cxx/_build/, or a temporary directory where the tree is read-only)"""
    for d in (os.path.join(HERE, "cxx", "_build"), os.path.join(tempfile.gettempdir(), "sora_rx11n_stage_model_%d" % os.getuid())):
        so = os.path.join(d, "librx11n_stage_model.so")
        try:
            os.makedirs(d, exist_ok=True)
            if os.path.exists(so) and os.path.getmtime(so) >= os.path.getmtime(SRC):
                return so
            tmp = "%s.%d" % (so, os.getpid())
            subprocess.check_call(["cc", "-O2", "-std=c11", "-fPIC", "-shared", "-Wall", "-Werror", SRC, "-o", tmp])
            os.replace(tmp, so)
            return so
        except OSError:
            continue
    raise RuntimeError("tests/cxx/rx11n_stage_model.c could not be built")


def load():
    global _lib
    if _lib is None:
        L = ctypes.CDLL(_build())
        vp, u32 = ctypes.c_void_p, ctypes.c_uint32
        L.st11n_cca.argtypes = [vp, vp, u32, u32, vp, vp]; L.st11n_cca.restype = u32
        L.st11a_desc.argtypes = [vp, u32, vp]; L.st11a_desc.restype = None
        L.st11a_frame_sink.argtypes = [vp, u32, vp]; L.st11a_frame_sink.restype = None
        _lib = L
    return _lib


def _c16(x):
    return np.ascontiguousarray(x, np.int16).reshape(-1, 2)


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


# ---- one stream / frame each; records are int32 words and are not modified
def cca(x0, x1, state, flags=0, branches=None):
    """TCCA11n over the bursts of x0 / x1 (int16 [4 n, 2]) -> (state after, bursts consumed); branches: a uint32 [16] array that accumulates BRANCHES"""
    a = _c16(x0); b = _c16(x1); assert len(a) == len(b)
    s = (np.asarray(state, np.int64) & 0xFFFFFFFF).astype(np.uint32).view(np.int32).reshape(WORDS).copy()
    used = int(load().st11n_cca(_p(a), _p(b), len(a) // 4, int(flags), _p(s), _p(branches) if branches is not None else None))
    return s, used


def data_symbol(x, nsym):
    """T11nDataSymbol on one chain: nsym symbols of 80 samples -> [nsym * 64, 2]"""
    return _c16(x)[:80 * nsym].reshape(nsym, 80, 2)[:, 16:].reshape(-1, 2).copy()


def stream_join(s0, s1, nb):
    """TStreamJoin<2, 52 nb> -> TStreamConcat<2, s>, s = max(nb / 2, 1): [n, 52 nb] x 2 -> [n, 104 nb]"""
    s = max(nb // 2, 1)
    a = np.ascontiguousarray(s0, np.uint8).reshape(-1, 52 * nb // s, 1, s); b = np.ascontiguousarray(s1, np.uint8).reshape(-1, 52 * nb // s, 1, s)
    return np.concatenate([a, b], axis=2).reshape(-1, 104 * nb)


def desc(dec, length):
    d = np.ascontiguousarray(dec, np.uint8); assert len(d) >= length + 2
    out = np.zeros(max(length, 1), np.uint8)
    load().st11a_desc(_p(d), int(length), _p(out))
    return out[:length]


def frame_sink(x, length):
    b = np.ascontiguousarray(x, np.uint8); rec = np.zeros(2, np.uint32); assert len(b) >= (length & 0xFFFF)
    load().st11a_frame_sink(_p(b), int(length), _p(rec))
    return rec


class ModelOps:
    """sora_amd.capi.rx11n_stages' bricks: the batch tables walked stream by stream over numpy buffers"""

    def __init__(self):
        self.o = pyoracle.Oracle(); self.comp = None; self.branches = np.zeros(16, np.uint32)

    @staticmethod
    def _u(a):
        return np.asarray(a).astype(np.int64) & 0xFFFFFFFF

    def host(self, a):
        return np.asarray(a)

    def downsample2(self, iq):
        x = _c16(iq)
        return x[:len(x) // 8 * 8:2].copy()                                      # as sora_hip_ingest: whole groups of 8 raw samples

    def cca(self, x0, x1, first, n, state, flags):
        st = np.array(state, np.int32); used = np.zeros(len(st), np.int32)
        for f, (a, k) in enumerate(zip(self._u(first), self._u(n))):
            st[f], used[f] = cca(x0[a:a + 4 * k], x1[a:a + 4 * k], st[f], flags, self.branches)
        return st, used

    def take(self, x, starts, length):
        return np.concatenate([x[a:a + length] for a in self._u(starts)]) if len(starts) else x[:0]

    def rows(self, a, idx):
        return a[np.asarray(idx, np.int64)]

    def concat(self, parts):
        return np.concatenate([np.asarray(p).reshape(-1) for p in parts])

    def cfo_est(self, l0, l1):
        return np.stack([self.o.cfo_est11n(a, b) for a, b in zip(l0.reshape(-1, 128, 2), l1.reshape(-1, 128, 2))])

    def freq_comp(self, x0, x1, first, nbursts, state):
        if self.comp is None:
            self.comp = (np.zeros_like(x0), np.zeros_like(x1))
        for f, (a, k) in enumerate(zip(self._u(first), self._u(nbursts))):
            if k:
                state[f], self.comp[0][a:a + 8 * k], self.comp[1][a:a + 8 * k] = self.o.freq_comp11n(state[f], x0[a:a + 8 * k], x1[a:a + 8 * k])
        return self.comp

    def data_symbol(self, x0, x1, first, nsym, out_first, total):
        o0 = np.zeros((total * 64, 2), np.int16); o1 = np.zeros_like(o0)
        for a, k, o in zip(self._u(first), self._u(nsym), self._u(out_first)):
            o0[64 * o:64 * (o + k)] = data_symbol(x0[a:a + 80 * k], k); o1[64 * o:64 * (o + k)] = data_symbol(x1[a:a + 80 * k], k)
        return o0, o1

    def fft64(self, x):
        return np.concatenate([self.o.fft(s, 64) for s in x.reshape(-1, 64, 2)]).reshape(-1, 2).astype(np.int16)

    def siso_est(self, l0, l1):
        return np.stack([self.o.siso_est11n(a, b) for a, b in zip(l0.reshape(-1, 128, 2), l1.reshape(-1, 128, 2))])

    def siso_comp_mrc(self, ch, y0, y1, frame_index):
        return np.concatenate([self.o.siso_comp11n(ch[f], a, b)[2] for f, a, b in zip(self._u(frame_index), y0.reshape(-1, 64, 2), y1.reshape(-1, 64, 2))])

    def sig_demap(self, mrc):
        return np.stack([self.o.sig_demap11n(s) for s in mrc.reshape(-1, 3, 64, 2)])

    def sig_decode(self, soft):
        rec = np.zeros((len(soft), 12), np.uint32)
        for i, s in enumerate(soft):
            ok, o9, f = self.o.sig_decode11n(s)
            b = [int(x) for x in o9]
            rec[i] = [int(x) for x in f] + [b[0] | b[1] << 8 | b[2] << 16, b[3] | b[4] << 8 | b[5] << 16 | b[6] << 24, b[7] | b[8] << 8]
        return rec

    def mimo_est(self, l0, l1):
        return np.stack([self.o.mimo_est11n(a, b)[1] for a, b in zip(l0.reshape(-1, 128, 2), l1.reshape(-1, 128, 2))])

    def mimo_comp(self, hinv, y0, y1, frame_index):
        r = [self.o.mimo_comp11n(hinv[f], a, b) for f, a, b in zip(self._u(frame_index), y0.reshape(-1, 64, 2), y1.reshape(-1, 64, 2))]
        return np.stack([a for a, _ in r]), np.stack([b for _, b in r])

    def pilot_track(self, x0, x1, first, nsym, state):
        for f, (a, k) in enumerate(zip(self._u(first), self._u(nsym))):
            for s in range(a, a + k):
                state[f, 16:] = self.o.pilot_track11n(state[f, 16:], x0[s], x1[s])

    def demap_deint(self, x, nb, iss):
        return np.stack([self.o.deinterleave11n(nb, iss, self.o.demap11n(nb, s)) for s in x.reshape(-1, 64, 2)])

    def stream_join(self, s0, s1, nb):
        return stream_join(s0, s1, nb)

    def viterbi(self, soft, soft_off, nsoft, lens, code_rate):
        out = np.zeros((len(lens), 2560), np.uint8)
        for i, (a, k, n) in enumerate(zip(self._u(soft_off), self._u(nsoft), lens)):
            d = self.o.viterbi_frame_ex(soft[a:a + k], int(code_rate), int(n), 192, 36)
            out[i, :int(n) + 2] = d[:int(n) + 2]
        return out.reshape(-1)

    def desc(self, dec, off, lens, out_off, total):
        out = np.zeros(max(total, 1), np.uint8)
        for a, n, o in zip(self._u(off), self._u(lens), self._u(out_off)):
            out[o:o + n] = desc(dec[a:a + n + 2], int(n))
        return out

    def frame_sink(self, x, off, lens):
        return np.stack([frame_sink(x[a:a + n], int(n)) for a, n in zip(self._u(off), self._u(lens))])


def first_events(iq0, iq1, descs, mcs_max=10, trace=None, ops=None):
    """the first event of every capture (descs: [(first sample, samples)] over the two chains at 40 MHz) -- sora_amd.rx11n_by_stages over the model's bricks"""
    load()
    return capi.rx11n_stages(ops or ModelOps(), _c16(iq0), _c16(iq1), descs, mcs_max, trace)
