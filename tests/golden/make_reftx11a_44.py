#!/usr/bin/env python3
"""Generate tests/golden/reftx11a_44.npz from the REFERENCE (run where the reference tree is; the fixture travels, the tree does not).

What the reference's 44 MHz transmit graphs -- CreateModGraph11a_44M + CreatePreamble11a_44M, the 40 MHz graphs with TUpsample40MTo44M
in front of TPackSample16to8 -- send for a list of frames, beside what its 40 MHz graphs send for the same frames.

In a temporary directory: oracle/ref_flatten.py lays the reference's headers out, oracle/ref_graph_shim.cpp is taken as it stands and one
export is appended to the copy -- the body of its ref_tx11a with the two graph names ending in _44M -- and the copy is compiled with
oracle/build_ref.sh's flags and loaded.  Nothing is written under oracle/, nothing compiled is kept.

Per frame i: mpdu_i, tx40_i (int8 [n, 2], ref_tx11a), tx44_i (int8 [11 n / 10, 2]); rate[i], seed[i].  Frames:
  * every rate x (1 byte, seed 0xFF) and (37 bytes, seed 0x5B);
  * the two shortest frames of a seeded search (400 frames, default_rng(3)) whose 40 MHz stream touches an int8 rail AND for which the
    model fed with those bytes (tests/tx11a44_model.py) differs from tx44 outside the indices where the reference read behind its input:
    they pin that the brick runs on the 16-bit samples, in front of the pack.
"""
import ctypes
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from tx11a44_model import compared, frame44_from_tx40, has_rail  # noqa: E402

RATES = (6000, 9000, 12000, 18000, 24000, 36000, 48000, 54000)
CXX = os.environ.get("SORA_REF_CXX", "/opt/rocm/lib/llvm/bin/clang++")
FLAGS = ["-std=c++14", "-O2", "-U__OPTIMIZE__", "-fPIC", "-shared", "-fvisibility=hidden", "-fms-extensions", "-fms-compatibility",
         "-fms-compatibility-version=19.00", "-fdelayed-template-parsing", "-fno-operator-names", "-msse4.1", "-mssse3", "-Wno-everything",
         "-DUSER_MODE", "-D__XSAVEINTRIN_H"]                                       # oracle/build_ref.sh, libsora_refgraph.so


def compile_graphs(tmp):
    oracle = os.path.join(ROOT, "oracle")
    subprocess.check_call([sys.executable, os.path.join(oracle, "ref_flatten.py"), os.path.join(tmp, "flat")])
    with open(os.path.join(oracle, "ref_graph_shim.cpp")) as fh:
        shim = fh.read()
    m = re.search(r"^EXPORT int ref_tx11a\(.*?^}\n", shim, re.S | re.M)
    twin = m.group(0).replace("ref_tx11a(", "ref_tx11a_44(").replace("CreateModGraph11a_40M", "CreateModGraph11a_44M").replace("CreatePreamble11a_40M", "CreatePreamble11a_44M")
    assert twin.count("_44M") == 2
    src = os.path.join(tmp, "shim44.cpp")
    with open(src, "w") as fh:
        fh.write(shim + "\n" + twin)
    so = os.path.join(tmp, "libref44.so")
    subprocess.check_call([CXX] + FLAGS + ["-include", os.path.join(oracle, "ref_compat.h"), "-I" + os.path.join(tmp, "flat"), src, "-o", so])
    return ctypes.CDLL(so)


def main():
    with tempfile.TemporaryDirectory() as tmp:
        L = compile_graphs(tmp)

        def tx(fn, mpdu, rate, seed):
            a = np.frombuffer(bytes(mpdu), np.uint8)
            cap = 11 * (640 + 160 * 1400) // 10
            o = np.zeros((cap, 2), np.int8)
            n = fn(a.ctypes.data_as(ctypes.c_void_p), len(a), rate, seed, o.ctypes.data_as(ctypes.c_void_p), cap)
            assert n > 0
            return o[:n].copy()

        frames = []
        for length, seed in ((1, 0xFF), (37, 0x5B)):
            rng = np.random.default_rng(4400 + length)
            for rate in RATES:
                frames.append((bytes(rng.integers(0, 256, length).astype(np.uint8)), rate, seed))
        rng = np.random.default_rng(3)
        found = []
        for _ in range(400):
            rate = RATES[int(rng.integers(0, 8))]
            mpdu = bytes(rng.integers(0, 256, int(rng.integers(200, 1501))).astype(np.uint8))
            seed = int(rng.integers(1, 128))
            t40 = tx(L.ref_tx11a, mpdu, rate, seed)
            if not has_rail(t40):
                continue
            t44 = tx(L.ref_tx11a_44, mpdu, rate, seed)
            keep = compared(len(t44))
            if not np.array_equal(frame44_from_tx40(t40, allow_rails=True)[keep], t44[keep]):
                found.append((len(t44), mpdu, rate, seed))
        found.sort(key=lambda f: f[0])
        print("rail frames on which the byte-fed model differs: %d of 400; kept:" % len(found), [(f[2], len(f[1]), f[3]) for f in found[:2]])
        frames += [f[1:] for f in found[:2]]
        out = {"rate": np.array([f[1] for f in frames], np.uint32), "seed": np.array([f[2] for f in frames], np.uint32)}
        for i, (mpdu, rate, seed) in enumerate(frames):
            out["mpdu_%d" % i] = np.frombuffer(mpdu, np.uint8)
            out["tx40_%d" % i] = tx(L.ref_tx11a, mpdu, rate, seed)
            out["tx44_%d" % i] = tx(L.ref_tx11a_44, mpdu, rate, seed)
            assert len(out["tx44_%d" % i]) * 10 == len(out["tx40_%d" % i]) * 11
        del L
    path = os.path.join(HERE, "reftx11a_44.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes,", len(frames), "frames")


if __name__ == "__main__":
    main()
