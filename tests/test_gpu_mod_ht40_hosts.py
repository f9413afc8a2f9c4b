"""tests/cxx/mod_ht40_chain.cpp EXECUTED on the GPU box (-m gpu): the joint-coded data graph of the 40 MHz HT 2x2 modulator built sink-first from the BRICK adapters of
include/sora_brick.hpp (scrambler -> encoder -> stream parser -> per stream interleaver -> mapper -> pilots -> IFFT -> guard interval, one symbol per burst), compiled
and linked like a user's program and run as a separate process.  What its two sinks collect is the fused joint transmitter's data field, sample for sample.
MCS 8, 10 and 14 are excluded: their symbol is 13.5, 40.5 and 121.5 bytes of the field, no whole number of the byte-wide bricks' bursts, so a graph that hands on one
symbol per Process() cannot be built from them; MCS 9 (bursts of 1 byte) and MCS 12 (bursts of 3) are taken, one of them with the short guard interval."""
import os

import numpy as np
import pytest

from test_gpu_hosts import ROOT, build, run

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def exe():
    return build("g++", "-std=c++17", os.path.join(ROOT, "tests", "cxx", "mod_ht40_chain.cpp"), "mod_ht40_chain")


@pytest.mark.parametrize("mcs,ln,seed,gi", [(9, 37, 0x5D, 0), (12, 301, 0x5B, 1)])
def test_brick_graph_of_the_ht40_modulator_equals_the_fused_joint_transmitter(tmp_path, exe, mcs, ln, seed, gi):
    import sora_amd
    mpdu = bytes(np.random.default_rng([mcs, ln]).integers(0, 256, ln).astype(np.uint8))
    fin = tmp_path / "mpdu.bin"; fout = tmp_path / "tx.bin"
    fin.write_bytes(mpdu)
    out = run([exe, str(mcs), str(seed), str(gi), str(fin), str(fout)])
    w0, w1, _ = sora_amd.tx_ht40_joint([mpdu], [mcs], [seed], gi=[gi])
    want = np.concatenate([w0.cpu().numpy()[1600:], w1.cpu().numpy()[1600:]])   # the data symbols of chain 0, then those of chain 1
    assert "%d samples per chain" % (len(want) // 2) in out, out
    got = np.frombuffer(fout.read_bytes(), np.int16).reshape(-1, 2)
    assert got.shape == want.shape and np.array_equal(got, want), np.flatnonzero((got != want).any(axis=1))[:8] if got.shape == want.shape else got.shape
