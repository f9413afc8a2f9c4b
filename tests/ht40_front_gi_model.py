"""The front end of the 40 MHz HT receiver with a guard flag (k_scan_ht40_gi, k_scan_ht40_stream_gi: a handle in SORA_HT40_GUARD_SIGNALLED) as an
integer model: tests/cxx/ht40_front_gi_model.c compiled beside its source, the way tests/ht40_front_model.py builds its C file, and bound here.  The C file calls nothing
but the oracle library's exported stage functions; this module loads that library first, with global symbols, so the model links against nothing and never reads the
library under test.  With guard off -- and with it on, on captures whose HT-SIG bit 31 is clear -- its records are tests/ht40_front_model.py's, field for field
(tests/test_ht40_gi_front_model_cpu.py).  TEST INFRASTRUCTURE: only tests/ use it."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

from oracle import pyoracle

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cxx", "ht40_front_gi_model.c")
JOINT, GUARD = 8, 16
SHORT_GI = 0x100                                 # SORA_HT40_SHORT_GI: what sora_ht40_found.mcs carries on top of the MCS of a recorded short-GI frame


class Event(ctypes.Structure):
    _fields_ = [("a20", ctypes.c_uint32), ("mcs", ctypes.c_uint32), ("ht_len", ctypes.c_uint32), ("nsym", ctypes.c_uint32), ("cfo", ctypes.c_int32),
                ("end_sample", ctypes.c_uint32), ("error_code", ctypes.c_uint32), ("short_gi", ctypes.c_uint32), ("S", ctypes.c_int64)]


_lib = None


def _build():
    """-> path of the compiled model (tests/cxx/_build/, or a temporary directory where the tree is read-only)"""
    inc = os.path.join(os.path.dirname(HERE), "oracle")
    for d in (os.path.join(HERE, "cxx", "_build"), os.path.join(tempfile.gettempdir(), "sora_ht40_front_gi_model_%d" % os.getuid())):
        so = os.path.join(d, "libht40_front_gi_model.so")
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
    raise RuntimeError("tests/cxx/ht40_front_gi_model.c could not be built")


def load():
    global _lib
    if _lib is None:
        pyoracle.build()
        o = ctypes.CDLL(pyoracle.ORACLE_SO, mode=ctypes.RTLD_GLOBAL)        # the stage functions the model calls
        o.so_init()
        _lib = ctypes.CDLL(_build())
        _lib.ht40_front_gi_capture.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int, ctypes.POINTER(Event), ctypes.c_int]
    return _lib


def front(iq0, iq1, guard=False, joint=False, max_events=64):
    """events of the front end over two int16 [n, 2] captures @40 MHz (n a multiple of 28), ALL the capture raises (the library keeps the first
    max_frames_per_capture of them): [{a20, mcs, ht_len, nsym, cfo, end_sample, error_code, short_gi, S}].  mcs is HT-SIG's; `found` below states the record the
    library reports."""
    L = load()
    a = np.ascontiguousarray(iq0, np.int16).reshape(-1, 2); b = np.ascontiguousarray(iq1, np.int16).reshape(-1, 2)
    assert len(a) == len(b) and len(a) % 28 == 0
    ev = (Event * max_events)()
    n = L.ht40_front_gi_capture(a.ctypes.data_as(ctypes.c_void_p), b.ctypes.data_as(ctypes.c_void_p), len(a), (GUARD if guard else 0) | (JOINT if joint else 0), ev, max_events)
    assert 0 <= n <= max_events, n
    return [{f: int(getattr(r, f)) for f, _ in Event._fields_} for r in ev[:n]]


def found(ev):
    """a model event -> the sora_ht40_found fields the library reports for it, but noise_var (S / 416, see tests/ht40_front_model.noise_var_of): a recorded short-GI
    frame carries SORA_HT40_SHORT_GI on its MCS"""
    return {"a20": ev["a20"], "mcs": ev["mcs"] | (SHORT_GI if ev["short_gi"] else 0), "ht_len": ev["ht_len"], "nsym": ev["nsym"], "cfo": ev["cfo"],
            "end_sample": ev["end_sample"], "error_code": ev["error_code"]}
