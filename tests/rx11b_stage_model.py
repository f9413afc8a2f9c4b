"""The bricks of the 802.11b receive graph one by one: tests/cxx/rx11b_stage_model.c compiled beside its source and bound here, array in, array and state out, with the
records of include/sora_hip.h as int32 words (sora_amd.capi.STATE11B_WORDS).  `first_event` composes them through sora_amd.capi.rx11b_stages -- the very walk
sora_amd.rx11b_by_stages runs over the GPU's stages -- with this module's bricks in place of the kernels.  The oracle library is loaded first, with global symbols, for
so_init and the CRC table; the model links against nothing.  TEST INFRASTRUCTURE: only tests/ and tools/bench_11b_stages.py use it."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

from oracle import pyoracle
from sora_amd import capi

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cxx", "rx11b_stage_model.c")
PER = {"dbpsk": 8, "dqpsk": 4, "cck5p5": 16, "cck11": 8}

_lib = None


def _build():
    """-> path of the compiled model (tests/cxx/_build/, or a temporary directory where the tree is read-only)"""
    inc = os.path.join(os.path.dirname(HERE), "oracle")
    deps = [SRC, os.path.join(inc, "so_oracle.h"), os.path.join(inc, "so_internal.h")]
    for d in (os.path.join(HERE, "cxx", "_build"), os.path.join(tempfile.gettempdir(), "sora_rx11b_stage_model_%d" % os.getuid())):
        so = os.path.join(d, "librx11b_stage_model.so")
        try:
            os.makedirs(d, exist_ok=True)
            if os.path.exists(so) and os.path.getmtime(so) >= max(os.path.getmtime(f) for f in deps):
                return so
            tmp = "%s.%d" % (so, os.getpid())
            subprocess.check_call(["cc", "-O2", "-std=c11", "-fPIC", "-shared", "-Wall", "-Werror", "-I", inc, SRC, "-o", tmp])
            os.replace(tmp, so)
            return so
        except OSError:
            continue
    raise RuntimeError("tests/cxx/rx11b_stage_model.c could not be built")


def load():
    global _lib
    if _lib is None:
        pyoracle.build()
        o = ctypes.CDLL(pyoracle.ORACLE_SO, mode=ctypes.RTLD_GLOBAL)        # so_init and the CRC table the model reads
        o.so_init()
        L = ctypes.CDLL(_build())
        vp, u32 = ctypes.c_void_p, ctypes.c_uint32
        L.st11b_dc_remove.argtypes = [vp, u32, u32, vp]; L.st11b_dc_remove.restype = None
        for fn in ("st11b_energy_detect", "st11b_barker_sync"):
            getattr(L, fn).argtypes = [vp, u32, vp]; getattr(L, fn).restype = u32
        L.st11b_sfd_sync.argtypes = [vp, u32, ctypes.c_int, vp]; L.st11b_sfd_sync.restype = u32
        L.st11b_symtiming.argtypes = [vp, u32, vp, vp, vp]; L.st11b_symtiming.restype = u32
        L.st11b_despread.argtypes = [vp, u32, vp]; L.st11b_despread.restype = None
        for fn in ("st11b_dbpsk_demap", "st11b_dqpsk_demap", "st11b_cck5p5_decode", "st11b_cck11_decode", "st11b_desc741"):
            getattr(L, fn).argtypes = [vp, u32, vp, vp]; getattr(L, fn).restype = None
        L.st11b_plcp_parse.argtypes = [vp, vp]; L.st11b_plcp_parse.restype = None
        L.st11b_frame_sink.argtypes = [vp, u32, vp]; L.st11b_frame_sink.restype = None
        _lib = L
    return _lib


def _c16(x):
    return np.ascontiguousarray(x, np.int16).reshape(-1, 2)


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _st(state, words):
    return (np.asarray(state, np.int64) & 0xFFFFFFFF).astype(np.uint32).view(np.int32).reshape(words).copy()


# ---- one stream each: -> (output, state after) or (state after, count); `state` is the record's int32 words and is not modified
def dc_remove(x, dc_word):
    x = _c16(x); out = np.empty_like(x)
    load().st11b_dc_remove(_p(x), len(x) // 4, int(dc_word) & 0xFFFFFFFF, _p(out))
    return out


def energy_detect(x, state):
    x = _c16(x); s = _st(state, 17)
    return s, int(load().st11b_energy_detect(_p(x), len(x) // 4, _p(s)))


def symtiming(x, state, trace=False):
    """-> (chips int16 [k, 2], state after[, m_index behind each block])"""
    x = _c16(x); s = _st(state, 2); nb = len(x) // 28
    out = np.zeros((8 * nb + 1, 2), np.int16); tr = np.zeros(nb + 1, np.int32)
    k = int(load().st11b_symtiming(_p(x), nb, _p(s), _p(out), _p(tr)))
    return (out[:k], s, tr[:nb]) if trace else (out[:k], s)


def barker_sync(x, state):
    x = _c16(x); s = _st(state, 15)
    return s, int(load().st11b_barker_sync(_p(x), len(x), _p(s)))


def sfd_sync(x, state, mode=0):
    x = _c16(x); s = _st(state, 9)
    return s, int(load().st11b_sfd_sync(_p(x), len(x), int(mode), _p(s)))


def despread(x):
    x = _c16(x); out = np.zeros((len(x) // 11, 2), np.int16)
    load().st11b_despread(_p(x), len(x) // 11, _p(out))
    return out


def stream_stage(kind, x, state):
    """kind: dbpsk, dqpsk, cck5p5, cck11 (x = symbols or chips) or desc741 (x = bytes) -> (bytes uint8, state after)"""
    s = _st(state, 4)
    if kind == "desc741":
        x = np.ascontiguousarray(x, np.uint8); n = len(x)
    else:
        x = _c16(x); n = len(x) // PER[kind]
    out = np.zeros(max(n, 1), np.uint8)
    fn = {"dbpsk": "st11b_dbpsk_demap", "dqpsk": "st11b_dqpsk_demap", "cck5p5": "st11b_cck5p5_decode", "cck11": "st11b_cck11_decode", "desc741": "st11b_desc741"}[kind]
    getattr(load(), fn)(_p(x), n, _p(s), _p(out))
    return out[:n], s


def plcp_parse(hdr):
    h = np.ascontiguousarray(hdr, np.uint8); rec = np.zeros(4, np.int32)
    load().st11b_plcp_parse(_p(h), _p(rec))
    return rec


def frame_sink(x, length):
    """x: at least length - 1 descrambled bytes"""
    b = np.ascontiguousarray(x, np.uint8); rec = np.zeros(2, np.int32)
    if length >= 4:
        assert len(b) >= (length & 0xFFFF) - 1
    load().st11b_frame_sink(_p(b), int(length), _p(rec))
    return rec


class ModelOps:
    """sora_amd.capi.rx11b_stages' bricks: the batch tables walked stream by stream over numpy buffers"""

    def alloc_c16(self, n):
        return np.zeros((max(int(n), 1), 2), np.int16)

    def alloc_u8(self, n):
        return np.zeros(max(int(n), 1), np.uint8)

    def host_u8(self, buf, a, b):
        return buf[a:b].tobytes()

    @staticmethod
    def _u(a):
        return np.asarray(a).astype(np.int64) & 0xFFFFFFFF

    def dc_remove(self, x, first, n, out_first, dc, out):
        for f, (a, k, o) in enumerate(zip(self._u(first), self._u(n), self._u(out_first))):
            out[o:o + 4 * k] = dc_remove(x[a:a + 4 * k], dc[f])

    def _search(self, fn, per, x, first, n, state, *extra):
        st = np.array(state, np.int32); used = np.zeros(len(st), np.int32)
        for f, (a, k) in enumerate(zip(self._u(first), self._u(n))):
            st[f], used[f] = fn(x[a:a + per * k], st[f], *extra)
        return st, used

    def energy_detect(self, x, first, n, state):
        return self._search(energy_detect, 4, x, first, n, state)

    def barker_sync(self, x, first, n, state):
        return self._search(barker_sync, 1, x, first, n, state)

    def sfd_sync(self, x, first, n, state, mode):
        return self._search(sfd_sync, 1, x, first, n, state, mode)

    def symtiming(self, x, first, n, out_first, state, out):
        st = np.array(state, np.int32); nch = np.zeros(len(st), np.int32)
        for f, (a, k, o) in enumerate(zip(self._u(first), self._u(n), self._u(out_first))):
            chips, st[f] = symtiming(x[a:a + 28 * k], st[f])
            out[o:o + len(chips)] = chips; nch[f] = len(chips)
        return st, nch

    def despread(self, x, first, n, out_first, out):
        for a, k, o in zip(self._u(first), self._u(n), self._u(out_first)):
            out[o:o + k] = despread(x[a:a + 11 * k])

    def stream_stage(self, kind, x, first, n, out_first, state, out):
        st = np.array(state, np.int32)
        per = PER.get(kind, 1)
        for f, (a, k, o) in enumerate(zip(self._u(first), self._u(n), self._u(out_first))):
            out[o:o + k], st[f] = stream_stage(kind, x[a:a + per * k], st[f])
        return st

    def plcp_parse(self, hdr, nhdr):
        return np.stack([plcp_parse(hdr[6 * f:6 * f + 6]) for f in range(nhdr)])

    def frame_sink(self, x, first, length):
        return np.stack([frame_sink(x[a:a + max(int(k) - 1, 0)], int(k)) for a, k in zip(self._u(first), self._u(length))])


def first_events(iq, descs, mode=0):
    """the first event of every capture (descs: [(first sample, samples)] over iq int16 [n, 2]) -- sora_amd.rx11b_by_stages over the model's bricks"""
    load()
    return capi.rx11b_stages(ModelOps(), _c16(iq), descs, mode)


def first_event(iq, mode=0):
    """the first event the graph reports over one capture, or None: error_code, rate_kbps, length, crc32, flags, mpdu"""
    a = _c16(iq)
    return first_events(a, [(0, len(a))], mode)[0]
