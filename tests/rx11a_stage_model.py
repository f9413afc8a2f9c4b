"""The front-end bricks of the 802.11a receive graph, one by one: tests/cxx/rx11a_stage_model.c (TDCRemoveEx<4>, TDCEstimator, TCCA11a, the three as a loop,
T11aViterbiSig, T11aPLCPParser in the reference bricks' own form, and the harness's source-call rules around carrier sense) compiled beside its source and bound here,
T11aDataSymbol as numpy index arithmetic, all over the records of include/sora_hip.h as int32 words.  Branches are counted in the classes of so_cs_counters.
TEST INFRASTRUCTURE: only tests/ and tools/bench_11a_rx_stages.py use it."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

from oracle import pyoracle
from sora_amd import capi

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cxx", "rx11a_stage_model.c")
COUNTERS = pyoracle.CS_COUNTERS
CCA, DCE, CS = capi.CCA11A_WORDS, capi.DCEST11A_WORDS, capi.CS11A_WORDS

_lib = None


def _build():
    """-> path of the compiled model (tests/cxx/_build/, or a temporary directory where the tree is read-only)"""
    for d in (os.path.join(HERE, "cxx", "_build"), os.path.join(tempfile.gettempdir(), "sora_rx11a_stage_model_%d" % os.getuid())):
        so = os.path.join(d, "librx11a_stage_model.so")
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
    raise RuntimeError("tests/cxx/rx11a_stage_model.c could not be built")


def load():
    global _lib
    if _lib is None:
        L = ctypes.CDLL(_build())
        vp, u32 = ctypes.c_void_p, ctypes.c_uint32
        L.st11a_set_pattern.argtypes = [vp]; L.st11a_set_pattern.restype = None
        L.st11a_dc_remove.argtypes = [vp, u32, u32, vp]; L.st11a_dc_remove.restype = None
        L.st11a_dc_estimate.argtypes = [vp, u32, vp]; L.st11a_dc_estimate.restype = None
        L.st11a_cca.argtypes = [vp, u32, u32, vp, vp, vp, vp]; L.st11a_cca.restype = u32
        L.st11a_carrier_sense.argtypes = [vp, u32, u32, vp, vp]; L.st11a_carrier_sense.restype = u32
        L.st11a_sense_walk.argtypes = [vp, u32, u32, vp, vp, u32, vp, u32, vp, vp, vp, u32, vp]; L.st11a_sense_walk.restype = u32
        L.st11a_viterbi_sig.argtypes = [vp]; L.st11a_viterbi_sig.restype = u32
        L.st11a_plcp_parse.argtypes = [u32, vp]; L.st11a_plcp_parse.restype = None
        pat = np.ascontiguousarray(pyoracle.Oracle().sts_pattern(), np.int16)      # cca.hpp:268-277; the library's own copy is pinned to it by tests/test_table_pins.py
        L.st11a_set_pattern(pat.ctypes.data_as(vp))
        _lib = L
    return _lib


def _c16(x):
    return np.ascontiguousarray(x, np.int16).reshape(-1, 2)


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


def _words(state, n):
    return (np.asarray(state, np.int64) & 0xFFFFFFFF).astype(np.uint32).view(np.int32).reshape(n).copy()


def pack(c):
    """int16 (re, im) -> the record's packed word"""
    return int(np.array(c, np.int16).view(np.uint32)[0])


def new_counters():
    return np.zeros(len(COUNTERS), np.uint64)


# ---- one stream each; records are int32 words and are not modified
def dc_remove(x, dc):
    a = _c16(x); out = np.zeros_like(a)
    load().st11a_dc_remove(_p(a), len(a) // 4, pack(dc), _p(out))
    return out


def dc_estimate(x, state):
    a = _c16(x); s = _words(state, DCE)
    load().st11a_dc_estimate(_p(a), len(a) // 4, _p(s))
    return s


def cca(x, state, flags=0, counters=None):
    """TCCA11a over DC-removed bursts -> (state after, bursts consumed, the gated bursts int16 [4 npass, 2])"""
    a = _c16(x); s = _words(state, CCA); out = np.zeros((len(a) + 4, 2), np.int16); npass = np.zeros(1, np.uint32)
    used = int(load().st11a_cca(_p(a), len(a) // 4, int(flags), _p(s), _p(out), _p(npass), _p(counters)))
    return s, used, out[:4 * int(npass[0])].copy()


def carrier_sense(x, state, flags=0, counters=None):
    """TDCRemoveEx -> TCCA11a -> TDCEstimator over raw bursts -> (state after, bursts consumed)"""
    a = _c16(x); s = _words(state, CS)
    used = int(load().st11a_carrier_sense(_p(a), len(a) // 4, int(flags), _p(s), _p(counters)))
    return s, used


def carrier_sense_split(x, state, flags=0):
    """the same from the three separate bricks, cut at each DC update: dc_remove over the bursts up to the next update, cca over them, dc_estimate over what it passed"""
    a = _c16(x); s = _words(state, CS); c = s[:CCA].copy(); d = s[CCA:].copy()
    used = 0; nb = len(a) // 4
    while used < nb and c[0] != 1:
        k = min(nb - used, int(d[0]) + 1)                                         # the update needs update_cnt + 1 gated bursts: no cut can come sooner
        dcv = np.array([d[2]], np.int32).view(np.int16)
        pi = dc_remove(a[4 * used:4 * (used + k)], dcv)
        before = c[1]
        c, u, gated = cca(pi, c, flags)
        d = dc_estimate(gated, d)
        used += u
        if (flags & capi.CCA11A_STOP_ON_TIMEOUT) and c[1] != before and np.uint32(c[1]) == capi.E_CS_TIMEOUT:
            break
    return np.concatenate([c, d]), used


def sense_walk(x20, rows, thr=1000 * 1000, counters=None):
    """the harness around carrier sense over one capture at the 20 MHz rate; rows: the oracle's events (where each frame's event falls is theirs)
    -> (frame starts, resume positions, records [n, 48])"""
    a = _c16(x20); n20 = len(a)
    st = np.array([r["start_sample"] for r in rows], np.uint32); en = np.array([r["end_sample"] for r in rows], np.uint32)
    cap = n20 // 14 + 2
    det = np.zeros(len(rows) + 8, np.uint32); nd = np.zeros(1, np.uint32); pos = np.zeros(cap, np.uint32); rec = np.zeros((cap, CS), np.uint32)
    n = int(load().st11a_sense_walk(_p(a), n20, int(thr), _p(st), _p(en), len(st), _p(det), len(det), _p(nd), _p(pos), _p(rec), cap, _p(counters)))
    assert n <= cap and nd[0] <= len(det)
    return det[:int(nd[0])].copy(), pos[:n], rec[:n]


def sense_walk_by(step, n20, rows, thr=1000 * 1000):
    """sense_walk's rules in Python over any carrier-sense entry, one call per source call: step(sample, bursts, state, flags) -> (state, used).  For the GPU's entry
    (tests/test_gpu_11a_rx_stages.py).  -> (frame starts, [(resume position, record)])"""
    ends = {int(r["start_sample"]): int(r["end_sample"]) for r in rows}
    st = capi.cs11a_states(1, thr)[0]; p = 0; det = []; pts = []
    plain = lambda s: s[0] == 0 and s[1] == 0 and s[5] == 0 and s[6] == 0
    while p + 4 <= n20:
        if p % 14 == 0 and plain(st):
            pts.append((p, st.copy()))
        m = min(((p + 4 + 13) // 14 * 14 - p) // 4, (n20 - p) // 4)              # the bursts that fit into this source call
        st, u = step(p, m, st, 0)
        p += 4 * u
        if st[0] == 1:
            det.append(p)
            if p not in ends:
                p = n20 + 4; break
            p = (ends[p] + 13) // 14 * 14
            capi.cca11a_reset(st.reshape(1, -1))
        elif np.uint32(st[1]) == capi.E_CS_TIMEOUT:                              # RxThread at the end of the call: ResetCarrierSense + Reset
            capi.cca11a_reset(st.reshape(1, -1))
    if p == n20 and n20 % 14 == 0 and plain(st):
        pts.append((p, st.copy()))
    return det, pts


class ModelOps:
    """sora_amd.capi.rx11a_stages' bricks: the batch tables walked stream by stream over numpy buffers.  The seven front-end bricks are this module's; the older
    stages (T11aLTS, the symbol chain, the trellis, the tail) are the reference-pinned functions of oracle.pyoracle.Oracle.  A frame's context is the oracle's."""

    def __init__(self):
        import rx11n_stage_model as tail
        self.o = pyoracle.Oracle(); self.tail = tail; self.counters = new_counters()

    @staticmethod
    def _u(a):
        return np.asarray(a).astype(np.int64) & 0xFFFFFFFF

    def downsample2(self, iq):
        return _c16(iq)[::2].copy()

    def carrier_sense(self, x, first, n, state, flags):
        st = np.array(state, np.int32); used = np.zeros(len(st), np.int32)
        for f, (a, k) in enumerate(zip(self._u(first), self._u(n))):
            st[f], used[f] = carrier_sense(x[a:a + 4 * k], st[f], flags, self.counters)
        return st, used

    def lts(self, x, starts):
        ctxs = []
        for a in self._u(starts):
            k = self.o.new_ctx(); self.o.lts(k, x[a:a + 144]); ctxs.append(k)
        return ctxs, np.array([k.CFO_est for k in ctxs])

    def symbols(self, x, starts, ctxs):
        """T11aDataSymbol (this module's) -> TFreqCompensation -> TFFT64 -> TChannelEqualization (the oracle's sym_front drops the prefix itself: hand it the symbol
        with the prefix this module's brick kept out put back as it was)"""
        out = []
        for a, k in zip(self._u(starts), ctxs):
            sym = x[a:a + 80]
            assert np.array_equal(data_symbol(sym, 1), sym[8:72])
            out.append(self.o.sym_front(k, sym))
        return np.stack(out)

    def track(self, eq, ctxs):
        return np.stack([self.o.sym_track(k, e) for k, e in zip(ctxs, eq)])

    def demap_deint(self, x, nb):
        return np.stack([self.o.deinterleave(nb, self.o.demap(nb, s)) for s in x])

    def rows(self, a, idx):
        return a[np.asarray(idx, np.int64)]

    def concat(self, parts):
        return np.concatenate([np.asarray(q).reshape(-1) for q in parts])

    def viterbi_sig(self, soft):
        return np.array([viterbi_sig(s) for s in soft], np.uint32)

    def plcp_parse(self, sig):
        return np.stack([plcp_parse(w) for w in sig])

    def viterbi(self, soft, soft_off, nsoft, lens, code_rate):
        out = np.zeros((len(lens), 2560), np.uint8)
        for i, (a, k, n) in enumerate(zip(self._u(soft_off), self._u(nsoft), lens)):
            d = self.o.viterbi_frame(soft[a:a + k], int(code_rate), int(n))
            out[i, :min(len(d), int(n) + 2)] = d[:int(n) + 2]
        return out.reshape(-1)

    def desc(self, dec, off, lens, out_off, total):
        out = np.zeros(max(total, 1), np.uint8)
        for a, n, o in zip(self._u(off), self._u(lens), self._u(out_off)):
            out[o:o + n] = self.tail.desc(dec[a:a + n + 2], int(n))
        return out

    def frame_sink(self, x, off, lens):
        return np.stack([self.tail.frame_sink(x[a:a + n], int(n)) for a, n in zip(self._u(off), self._u(lens))])

    def host(self, a):
        return np.asarray(a)


def events(iq, descs, rate_mhz=40, ops=None):
    """every event of every capture -- sora_amd.rx11a_by_stages over the model's bricks"""
    load()
    return capi.rx11a_stages(ops or ModelOps(), _c16(iq), descs, rate_mhz)


def data_symbol(x, nsym):
    """T11aDataSymbol: nsym symbols of 80 samples -> [nsym * 64, 2]: samples 8 .. 71 of each"""
    return _c16(x)[:80 * nsym].reshape(nsym, 80, 2)[:, 8:72].reshape(-1, 2).copy()


def viterbi_sig(soft48):
    a = np.ascontiguousarray(soft48, np.uint8); assert a.size == 48
    return int(load().st11a_viterbi_sig(_p(a)))


def plcp_parse(sig):
    rec = np.zeros(5, np.uint32)
    load().st11a_plcp_parse(int(sig) & 0xFFFFFFFF, _p(rec))
    return rec
