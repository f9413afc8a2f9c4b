#!/usr/bin/env python3
"""Generate tests/golden/ref_vectors_11a_stages.npz from the REFERENCE's own bricks (run where oracle/_ref is built; needs the reference tree).

  ref_vectors_11a_stages.npz  what the compiled reference makes of the recorded subset of tests/stage_edge_cases.py: T11aLTS (every case of the L-LTF family:
                              CFO_est, FreqCoeffs, ChannelCoeffs, and the four phase words it clears), TFreqCompensation -> TFFT64 -> TChannelEqualization (the
                              first 129 symbols), TPhaseCompensate -> TPilotTrack (the tracked symbols of the frames of 1, 2 and 128 symbols, the state record at
                              the end of every frame), the demap primitives behind T11aDemap<N>, T11aDeinterleave*, T11nDemap*, T11nSigDemap, TSisoChannelEst and
                              TMimoChannelEst.  Only outputs and the seeds are stored: the inputs are regenerated from the seeds.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle.pyoracle import Oracle, Reference, ReferenceGraph  # noqa: E402
import stage_edge_cases as sc  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "ref_vectors_11a_stages.npz")


def main():
    o = Oracle(); g = ReferenceGraph(); r = Reference()
    if not (g.has_11a_bricks() and r.available()):
        sys.exit("oracle/_ref is not built (needs the reference tree)")
    v = sc.recorded_vectors(o, sc.Engine(o, g), sc.cpu_functions(o, g, r))
    np.savez_compressed(OUT, **v)
    size = os.path.getsize(OUT)
    print("%s: %d bytes, %s" % (OUT, size, {k: a.shape for k, a in v.items()}))
    assert size <= 512 * 1024


if __name__ == "__main__":
    main()
