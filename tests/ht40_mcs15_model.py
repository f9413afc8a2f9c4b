"""ht40_mcs15_model.py -- TEST INFRASTRUCTURE: MCS 15 (two streams, 64-QAM, rate 5/6) and code rate 5/6 at any N_BPSC on the 40 MHz HT 2x2 pair (sora_ht40_set_mcs_max,
SORA_CR_56), from the models that exist.  The reference has no encoder or decoder for the rate, so these are the library's definition:

  * the FORMAT is the existing models' with three definitions extended, for the time a model runs inside `with rate56():` -- oracle/py_ht40.py's ndbps (rate 3: 90 N_BPSC per
    stream), its puncture (rate 3: A1 B1 A2 B3 A4 B5 per five input bits) and its MCS table (15: N_BPSC 6, rate 3).  Everything built on them -- py_ht40.tx / tx_frame,
    tests/ht40_joint_model.py, tests/tx_ht40_model.py, tests/tx_ht40_gi_model.py, tests/ht40_gi_cases.py -- then states an MCS 15 frame, HT-SIG's MCS field included,
    with nothing else changed.  Outside the `with` the modules are what they were;
  * the DATA FIELD is tests/ht40_gi_model.model's soft bytes (they do not depend on the code rate), then tests/viterbi56_model.py, then the oracle's descrambler /
    FCS sink; at rates 0..2 it is tests/ht40_gi_model.model itself;
  * the FRONT END is tests/ht40_front_gi_model.py's walk with the gate as a parameter (tests/cxx/ht40_front_mcs15_model.c).
Nothing here imports the library under test."""
import contextlib
import ctypes
import os
import subprocess
import tempfile

import numpy as np

from oracle import py_ht40 as m
from oracle import pyoracle
import ht40_gi_model as G
import ht40_stage_model as sm
import viterbi56_model as vm

CR_56 = 3
SHORT = 0x100
_NUM, _DEN = (1, 2, 3, 5), (2, 3, 4, 6)


def ndbps(nbpsc, code_rate):
    return 108 * nbpsc * _NUM[code_rate] // _DEN[code_rate]


def puncture(a, b, code_rate):
    if code_rate != CR_56:
        return _puncture0(a, b, code_rate)
    n = len(a) // 5                                              # 5/6: (A0 B0) (A1) (B2) (A3) (B4)
    return np.stack([a[0::5][:n], b[0::5][:n], a[1::5][:n], b[2::5][:n], a[3::5][:n], b[4::5][:n]], 1).reshape(-1)


_puncture0 = m.puncture


@contextlib.contextmanager
def rate56():
    """inside: py_ht40.ndbps / puncture know rate 3 and py_ht40.MCS2 knows MCS 15, so every model built on them states rate 5/6 frames"""
    keep = (m.ndbps, m.puncture, m.MCS2)
    m.ndbps, m.puncture, m.MCS2 = ndbps, puncture, {**keep[2], 15: (6, CR_56)}
    try:
        yield
    finally:
        m.ndbps, m.puncture, m.MCS2 = keep


# ------------------------------------------------------------------ the data field
def model(iq, offset, n_bpsc, code_rate, length, cfo, weights, gi=0, joint=False):
    """tests/ht40_gi_model.model for code_rate 0..3 -> its Result"""
    if code_rate != CR_56:
        return G.model(iq, offset, n_bpsc, code_rate, length, cfo, weights, gi=gi, joint=joint)
    with rate56():
        r = G.model(iq, offset, n_bpsc, code_rate, length, cfo, weights, gi=gi, joint=joint, decode=False)
    jobs = [(r.soft, int(length))] if joint else [(r.soft[s], int(length[s])) for s in range(2)]
    O = sm.oracle()
    for i, (sb, ln) in enumerate(jobs):
        dec = vm.viterbi_frame(sb, CR_56, ln)
        full = np.zeros(ln + 2, np.uint8); full[:len(dec)] = dec
        e, psdu, crc = O.desc_sink(full, ln)
        r.streams[i] = G.Stream(e & 0xFFFFFFFF, crc, psdu.tobytes())
    return r


def descriptor(cap_offset, rec, noise_var, joint=False, frame_id=0):
    """tests/ht40_front_model.descriptor's rule for a recorded frame's record, MCS 15 included: (offset, n_bpsc, code_rate, length0, length1, cfo, noise_var, id)"""
    import ht40_front_model as fm
    if rec["mcs"] != 15:
        return fm.descriptor(cap_offset, rec, noise_var, joint, frame_id)
    d = fm.descriptor(cap_offset, dict(rec, mcs=14), noise_var, joint, frame_id)     # MCS 14's N_BPSC; the rule does not look at the rate otherwise
    assert d[1] == 6 and d[2] == 2
    return d[:2] + (CR_56,) + d[3:]


# ------------------------------------------------------------------ the front end
SRC =os.path.join(os.path.dirname(os.path.abspath(__file__)), "cxx", "ht40_front_mcs15_model.c")
JOINT, GUARD = 8, 16
_lib = None


class Event(ctypes.Structure):
    _fields_ = [("a20", ctypes.c_uint32), ("mcs", ctypes.c_uint32), ("ht_len", ctypes.c_uint32), ("nsym", ctypes.c_uint32), ("cfo", ctypes.c_int32),
                ("end_sample", ctypes.c_uint32), ("error_code", ctypes.c_uint32), ("short_gi", ctypes.c_uint32), ("S", ctypes.c_int64)]


def _build():
    here = os.path.dirname(os.path.abspath(__file__))
    inc = os.path.join(os.path.dirname(here), "oracle")
    for d in (os.path.join(here, "cxx", "_build"), os.path.join(tempfile.gettempdir(), "sora_ht40_front_mcs15_model_%d" % os.getuid())):
        so = os.path.join(d, "libht40_front_mcs15_model.so")
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
    raise RuntimeError("tests/cxx/ht40_front_mcs15_model.c could not be built")


def load():
    global _lib
    if _lib is None:
        pyoracle.build()
        o = ctypes.CDLL(pyoracle.ORACLE_SO, mode=ctypes.RTLD_GLOBAL)        # the stage functions the model calls
        o.so_init()
        _lib = ctypes.CDLL(_build())
        _lib.ht40_front_mcs15_capture.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int, ctypes.c_uint32, ctypes.POINTER(Event), ctypes.c_int]
    return _lib


def front(iq0, iq1, mcs_max=14, guard=False, joint=False, max_events=64):
    """tests/ht40_front_gi_model.front with the gate 8 <= MCS <= mcs_max"""
    L = load()
    a = np.ascontiguousarray(iq0, np.int16).reshape(-1, 2); b = np.ascontiguousarray(iq1, np.int16).reshape(-1, 2)
    assert len(a) == len(b) and len(a) % 28 == 0
    ev = (Event * max_events)()
    n = L.ht40_front_mcs15_capture(a.ctypes.data_as(ctypes.c_void_p), b.ctypes.data_as(ctypes.c_void_p), len(a), (GUARD if guard else 0) | (JOINT if joint else 0),
                                   int(mcs_max), ev, max_events)
    assert 0 <= n <= max_events, n
    return [{f: int(getattr(r, f)) for f, _ in Event._fields_} for r in ev[:n]]
