"""The 802.11b receive graph with TSFDSync extended to the short preamble (sora_rx11b_set_preamble): tests/cxx/rx11b_ext_model.c compiled beside its
source and bound here, and the channel the loop-back checks share.  The C file restates oracle/so_rx11b.c's walk with a `mode` argument; this module
loads the oracle library first, with global symbols, so the model links against nothing.  TEST INFRASTRUCTURE: only tests/ and
tools/bench_11b_short.py use it."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

from oracle import pyoracle

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cxx", "rx11b_ext_model.c")
E_FRAME_OK, E_CRC32_FAIL = 0x1, 0x80000006
ROW_SHORT_PREAMBLE = 2

_lib = None


def _build():
    """-> path of the compiled model (tests/cxx/_build/, or a temporary directory where the tree is read-only)"""
    inc = os.path.join(os.path.dirname(HERE), "oracle")
    deps = [SRC, os.path.join(inc, "so_oracle.h"), os.path.join(inc, "so_internal.h")]
    for d in (os.path.join(HERE, "cxx", "_build"), os.path.join(tempfile.gettempdir(), "sora_rx11b_ext_model_%d" % os.getuid())):
        so = os.path.join(d, "librx11b_ext_model.so")
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
    raise RuntimeError("tests/cxx/rx11b_ext_model.c could not be built")


def load():
    global _lib
    if _lib is None:
        pyoracle.build()
        o = ctypes.CDLL(pyoracle.ORACLE_SO, mode=ctypes.RTLD_GLOBAL)        # so_init and the CRC table the model reads
        o.so_init()
        _lib = ctypes.CDLL(_build())
    return _lib


def rx11b(iq44, mode=0, max_frames=16):
    """events of the graph over one int16 [n,2] capture @44 MHz, as Oracle.rx11b_capture reports them, plus "flags" (ROW_SHORT_PREAMBLE)"""
    L = load()
    a = np.ascontiguousarray(iq44, np.int16).reshape(-1, 2)
    res = (pyoracle.FrameResult * max_frames)(); mp = np.zeros(max_frames * 4096, np.uint8)
    n = L.rx11b_ext_capture(a.ctypes.data_as(ctypes.c_void_p), len(a), int(mode), res, max_frames, mp.ctypes.data_as(ctypes.c_void_p), mp.size)
    out = []
    for r in res[:n]:
        d = {f: getattr(r, f) for f, _ in pyoracle.FrameResult._fields_}
        d["flags"] = d.pop("reserved")
        d["mpdu"] = mp[r.mpdu_offset:r.mpdu_offset + r.length].tobytes() if r.error_code in (E_FRAME_OK, E_CRC32_FAIL) else b""
        out.append(d)
    return out


def capture(rng, waves, leads, sigma, scale=96, tail=600):
    """The loop-back channel: the COMPLEX8 waveforms `waves` (int8 [n,2]) scaled by `scale`, waves[i] behind leads[i] samples of silence, white
    noise of `sigma` over everything -> int16 [m,2], m a multiple of 28."""
    n = sum(leads) + sum(len(w) for w in waves) + tail
    n = (n + 27) // 28 * 28
    z = np.zeros((n, 2), np.float64); at = 0
    for w, lead in zip(waves, leads):
        at += lead
        z[at:at + len(w)] = w.astype(np.float64) * scale; at += len(w)
    z += rng.normal(0, sigma, z.shape)
    return np.clip(np.rint(z), -32768, 32767).astype(np.int16)


def key(r):
    """what two reports of one event must agree on"""
    return (r["error_code"], r["end_sample"], r["rate_kbps"], r["length"], r["crc32"], r.get("flags", 0), r["mpdu"])
