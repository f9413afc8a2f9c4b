#!/usr/bin/env python3
"""Generate tests/golden/refmod_11n_mcs11_14.npz from the REFERENCE's own 802.11n modulator (oracle/_ref/libsora_refgraph.so, ReferenceGraph.tx11n):
one frame per MCS 11..14 -- tx<mcs>_0 / tx<mcs>_1, the two TX chains' COMPLEX16 streams @40 MHz, and mpdu<mcs>, the bytes sent (without the FCS the
modulator appends) -- each of two data symbols, and one MCS 9 frame of two data symbols as well (the position rule: an MCS 11..14 event falls where the
compiled graph reports a frame of as many symbols).  Recorded outputs only; tests/test_rx11n_mcs_cpu.py decodes them where oracle/_ref is not built.  Run where the reference tree is."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle.pyoracle import ReferenceGraph  # noqa: E402

LENGTHS = {11: 40, 12: 60, 13: 80, 14: 100, 9: 15}
SEED = 20261017


def main():
    g = ReferenceGraph()
    if not g.available():
        sys.exit("oracle/_ref/libsora_refgraph.so is not built")
    rng = np.random.default_rng(SEED)
    out = {}
    for mcs, ln in LENGTHS.items():
        mp = rng.integers(0, 256, ln).astype(np.uint8)
        s0, s1 = g.tx11n(mp.tobytes(), mcs)
        out["tx%d_0" % mcs] = s0; out["tx%d_1" % mcs] = s1; out["mpdu%d" % mcs] = mp
    np.savez_compressed(os.path.join(os.path.dirname(os.path.abspath(__file__)), "refmod_11n_mcs11_14.npz"), **out)


if __name__ == "__main__":
    main()
