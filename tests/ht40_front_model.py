"""The front end of the 40 MHz HT receiver (k_scan_ht40 up to its records, then k_ht40_plan's translation of a record into a frame descriptor) as an integer
model: tests/cxx/ht40_front_model.c compiled beside its source and bound here.  The C file walks the graph as oracle/so_rx11n.c does and calls nothing but the
oracle library's exported stage functions; this module loads that library first, with global symbols, so the model links against nothing and never reads the
library under test.  TEST INFRASTRUCTURE: only tests/ use it."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

from oracle import pyoracle

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cxx", "ht40_front_model.c")
E_PLCP_HEADER_FAIL = 0x80000005
OWN_SIGN, OWN_GATE, OWN_EVENTS, JOINT = 1, 2, 4, 8
OWN = OWN_SIGN | OWN_GATE | OWN_EVENTS          # the front end as the library defines it; 0: the reference's 802.11n graph
CAUSES = ("ok", "lsig_bits", "lsig_parity", "lsig_rate", "lsig_length", "ht_crc", "mcs_low", "mcs_high", "cbw20", "len_short", "len_long")
MCS2 = {8: (1, 0), 9: (2, 0), 10: (2, 2), 11: (4, 0), 12: (4, 2), 13: (6, 1), 14: (6, 2)}          # MCS -> (N_BPSC, code rate index)


class Event(ctypes.Structure):
    _fields_ = [("a20", ctypes.c_uint32), ("mcs", ctypes.c_uint32), ("ht_len", ctypes.c_uint32), ("nsym", ctypes.c_uint32), ("cfo", ctypes.c_int32),
                ("end_sample", ctypes.c_uint32), ("error_code", ctypes.c_uint32), ("pad", ctypes.c_uint32), ("S", ctypes.c_int64)]


_lib = None


def _build():
    """-> path of the compiled model (tests/cxx/_build/, or a temporary directory where the tree is read-only)"""
    inc = os.path.join(os.path.dirname(HERE), "oracle")
    for d in (os.path.join(HERE, "cxx", "_build"), os.path.join(tempfile.gettempdir(), "sora_ht40_front_model_%d" % os.getuid())):
        so = os.path.join(d, "libht40_front_model.so")
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
    raise RuntimeError("tests/cxx/ht40_front_model.c could not be built")


def load():
    global _lib
    if _lib is None:
        pyoracle.build()
        o = ctypes.CDLL(pyoracle.ORACLE_SO, mode=ctypes.RTLD_GLOBAL)        # the stage functions the model calls
        o.so_init()
        _lib = ctypes.CDLL(_build())
        _lib.ht40_front_capture.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int, ctypes.POINTER(Event), ctypes.c_int]
    return _lib


def front(iq0, iq1, flags=OWN, max_events=64, counters=None):
    """events of the front end over two int16 [n, 2] captures @40 MHz (n a multiple of 28), ALL the capture raises (the library keeps the first
    max_frames_per_capture of them): [{a20, mcs, ht_len, nsym, cfo, end_sample, error_code, S}].  counters: a dict that receives what the walk counted
    (sig_fields, disagreements, ref_accepts_cbw40, flush0..2, cut_frames, timeouts and the gate's verdicts by cause)."""
    L = load()
    a = np.ascontiguousarray(iq0, np.int16).reshape(-1, 2); b = np.ascontiguousarray(iq1, np.int16).reshape(-1, 2)
    assert len(a) == len(b) and len(a) % 28 == 0
    ev = (Event * max_events)()
    L.ht40_front_reset_counters()
    n = L.ht40_front_capture(a.ctypes.data_as(ctypes.c_void_p), b.ctypes.data_as(ctypes.c_void_p), len(a), int(flags), ev, max_events)
    assert 0 <= n <= max_events, n
    if counters is not None:
        c = (ctypes.c_int * (8 + len(CAUSES)))(); L.ht40_front_counters(c)
        counters.update(dict(zip(("sig_fields", "disagreements", "ref_accepts_cbw40", "flush0", "flush1", "flush2", "cut_frames", "timeouts") + CAUSES, list(c))))
    return [{f: int(getattr(r, f)) for f, _ in Event._fields_ if f != "pad"} for r in ev[:n]]


def noise_var_of(S):
    """noise_var as the front end defines it, exactly: S / 416 (numpy float64 of an int64 below 2^53)"""
    return S / 416.0


# ------------------------------------------------------------------ k_ht40_plan: a record -> the sora_ht40_frame the data field takes
def trunc_half(cfo):
    """cfo / 2 in C: truncation toward zero (-3 -> -1, where an arithmetic shift gives -2)"""
    return -((-cfo) // 2) if cfo < 0 else cfo // 2


def descriptor(cap_offset, rec, noise_var, joint=False, frame_id=0):
    """a recorded frame's record (error_code 0) of a capture at `cap_offset` -> (offset, n_bpsc, code_rate, length0, length1, cfo, noise_var, id): HT-LTF 1 starts
    behind the 160 samples of HT-STF, the CFO per 40 MHz sample is half the estimate per 20 MHz sample, noise_var goes through unchanged, each stream carries a PSDU
    of HT-SIG's LENGTH -- in joint coding the frame carries one"""
    assert rec["error_code"] == 0
    nb, cr = MCS2[rec["mcs"]]
    return (cap_offset + 2 * rec["a20"] + 160, nb, cr, rec["ht_len"], 0 if joint else rec["ht_len"], trunc_half(rec["cfo"]), noise_var, frame_id)
