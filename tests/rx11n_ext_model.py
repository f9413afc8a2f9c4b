"""The 802.11n 2x2 receive graph with T11nSigParser's MCS gate at `mcs_max` (sora_rx11n_set_mcs_max): tests/cxx/rx11n_ext_model.c compiled beside its
source and bound here.  The C file walks the graph as oracle/so_rx11n.c does and calls nothing but the oracle library's exported stage functions; this
module loads that library first, with global symbols, so the model links against nothing.  TEST INFRASTRUCTURE: only tests/ and tools/bench_rx11n_mcs.py use it."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

from oracle import pyoracle

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cxx", "rx11n_ext_model.c")
E_FRAME_OK, E_PLCP_HEADER_FAIL, E_CRC32_FAIL = 0x1, 0x80000005, 0x80000006

_lib = None


def _build():
    """-> path of the compiled model (tests/cxx/_build/, or a temporary directory where the tree is read-only)"""
    inc = os.path.join(os.path.dirname(HERE), "oracle")
    for d in (os.path.join(HERE, "cxx", "_build"), os.path.join(tempfile.gettempdir(), "sora_rx11n_ext_model_%d" % os.getuid())):
        so = os.path.join(d, "librx11n_ext_model.so")
        try:
            os.makedirs(d, exist_ok=True)
            if os.path.exists(so) and os.path.getmtime(so) >= max(os.path.getmtime(SRC), os.path.getmtime(os.path.join(inc, "so_oracle.h"))):
                return so
            tmp = "%s.%d" % (so, os.getpid())
            subprocess.check_call(["cc", "-O2", "-std=c11", "-fPIC", "-shared", "-Wall", "-Werror", "-I", inc, SRC, "-o", tmp])
            os.replace(tmp, so)
            return so
        except OSError:
            continue
    raise RuntimeError("tests/cxx/rx11n_ext_model.c could not be built")


def load():
    global _lib
    if _lib is None:
        pyoracle.build()
        o = ctypes.CDLL(pyoracle.ORACLE_SO, mode=ctypes.RTLD_GLOBAL)        # the stage functions the model calls
        o.so_init()
        _lib = ctypes.CDLL(_build())
    return _lib


def rx11n(iq0, iq1, mcs_max=10, max_frames=16):
    """events of the graph over two int16 [n,2] captures @40 MHz, as Oracle.rx11n_capture reports them (rate_kbps = MCS index)"""
    L = load()
    a = np.ascontiguousarray(iq0, np.int16).reshape(-1, 2); b = np.ascontiguousarray(iq1, np.int16).reshape(-1, 2)
    assert len(a) == len(b)
    res = (pyoracle.FrameResult * max_frames)(); mp = np.zeros(max_frames * 4096, np.uint8)
    n = L.rx11n_ext_capture(a.ctypes.data_as(ctypes.c_void_p), b.ctypes.data_as(ctypes.c_void_p), len(a), int(mcs_max), res, max_frames,
                            mp.ctypes.data_as(ctypes.c_void_p), mp.size)
    out = []
    for r in res[:n]:
        d = {f: getattr(r, f) for f, _ in pyoracle.FrameResult._fields_}
        d["mpdu"] = mp[r.mpdu_offset:r.mpdu_offset + r.length].tobytes() if r.error_code in (E_FRAME_OK, E_CRC32_FAIL) else b""
        out.append(d)
    return out


def parser_disagreements():
    """SIG fields seen so far on which the model's parser at gate 10 and so_sig_decode11n differed (0: they are one parser there)"""
    return load().rx11n_ext_parser_disagreements()


def clean_channel(rng, s0, s1, sigma, lead=None, tail=600):
    """The channel of the loop-back checks: unit gain, a random phase per chain, cross-talk 0 or 0.1, CFO up to 2e-4 rad/sample, white noise of `sigma`.
    s0, s1: the two TX chains' int16 [n,2] waveforms -> two int16 [m,2] captures, m a multiple of 28."""
    lead = int(rng.integers(200, 1500)) if lead is None else lead
    x = float(rng.choice([0.0, 0.1])); ph = np.exp(1j * rng.uniform(0, 2 * np.pi, 2)); cfo = rng.uniform(-2e-4, 2e-4)
    c0 = s0[:, 0].astype(np.float64) + 1j * s0[:, 1]; c1 = s1[:, 0].astype(np.float64) + 1j * s1[:, 1]; k = np.arange(len(c0))
    r0 = (ph[0] * c0 + x * c1) * np.exp(1j * cfo * k); r1 = (ph[1] * c1 + x * c0) * np.exp(1j * cfo * k)
    n = (lead + len(r0) + tail + 27) // 28 * 28
    out = []
    for r in (r0, r1):
        z = np.zeros(n, complex); z[lead:lead + len(r)] = r
        z = z + rng.normal(0, sigma, n) + 1j * rng.normal(0, sigma, n)
        out.append(np.stack([np.clip(np.rint(z.real), -32768, 32767), np.clip(np.rint(z.imag), -32768, 32767)], 1).astype(np.int16))
    return out[0], out[1]


def fcs(mpdu_nofcs):
    import zlib
    return (zlib.crc32(bytes(mpdu_nofcs)) & 0xFFFFFFFF).to_bytes(4, "little")
