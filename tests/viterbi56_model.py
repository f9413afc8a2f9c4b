"""The K=7 decoder with the rate 5/6 puncture pattern (include/sora_hip.h, SORA_CR_56): tests/cxx/viterbi56_model.c compiled beside its source and bound here.
The C file links against nothing and reads no library.  TEST INFRASTRUCTURE: only tests/ and tools/ use it."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cxx", "viterbi56_model.c")
CR_56 = 3

_lib = None


def _build():
    """-> path of the compiled model (tests/cxx/_build/, or a temporary directory where the tree is read-only)"""
    for d in (os.path.join(HERE, "cxx", "_build"), os.path.join(tempfile.gettempdir(), "sora_viterbi56_model_%d" % os.getuid())):
        so = os.path.join(d, "libviterbi56_model.so")
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
    raise RuntimeError("tests/cxx/viterbi56_model.c could not be built")


def load():
    global _lib
    if _lib is None:
        _lib = ctypes.CDLL(_build())
        _lib.v56_viterbi_frame.restype = ctypes.c_int
        _lib.v56_viterbi_frame.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32]
        _lib.v56_encode.restype = ctypes.c_int
        _lib.v56_encode.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int, ctypes.c_void_p]
    return _lib


def viterbi_frame(soft, code_rate, frame_length, depth=192, lookahead=36):
    """the decoded bytes (uint8, frame_length + 2 for a whole frame) of one stream of soft values 0..7"""
    a = np.ascontiguousarray(soft, np.uint8)
    out = np.zeros(int(frame_length) + 64, np.uint8)
    n = load().v56_viterbi_frame(a.ctypes.data, len(a), int(code_rate), int(frame_length), out.ctypes.data, depth, lookahead)
    return out[:n]


def encode(bits, code_rate=CR_56):
    """the punctured coded bits (uint8, one per element) of `bits` from the all-zero state; whole puncture groups only"""
    b = np.ascontiguousarray(bits, np.uint8)
    out = np.zeros(2 * len(b) + 8, np.uint8)
    n = load().v56_encode(b.ctypes.data, len(b), int(code_rate), out.ctypes.data)
    return out[:n]


def nsoft_of(frame_length, code_rate=CR_56):
    """soft values of the shortest whole-group stream that holds a frame's last trace-back (tr_end = 8 length + 22 steps)"""
    gs, gb = {0: (1, 2), 1: (2, 3), 2: (3, 4), 3: (5, 6)}[int(code_rate)]
    return (8 * int(frame_length) + 22 + gs - 1) // gs * gb


def clean_stream(payload, code_rate=CR_56, extra_groups=0):
    """soft values (0 / 7) of a frame whose decoder output is `payload` (length + 2 bytes, LSB first), six zero tail bits and zero padding behind it"""
    gs = {0: 1, 1: 2, 2: 3, 3: 5}[int(code_rate)]
    bits = np.unpackbits(np.frombuffer(bytes(payload), np.uint8), bitorder="little")
    steps = (len(bits) + 6 + gs - 1) // gs * gs + extra_groups * gs
    bits = np.concatenate([bits, np.zeros(steps - len(bits), np.uint8)])
    return (encode(bits, code_rate) * 7).astype(np.uint8)
