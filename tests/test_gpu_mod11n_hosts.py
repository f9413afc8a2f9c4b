"""tests/cxx/mod11n_chain.cpp EXECUTED on the GPU box (-m gpu): the data graph of the 802.11n 2x2 modulator built sink-first from the BRICK adapters of
include/sora_brick.hpp (scrambler -> encoder -> stream parser -> per stream interleaver -> mapper -> pilots -> TIFFTxOnly -> [TCSD<4>] -> TAddGI, one symbol per
burst), compiled and linked like a user's program and run as a separate process.  What its two sinks collect is the fused transmitter's data field, sample for sample."""
import os

import numpy as np
import pytest

from test_gpu_hosts import ROOT, build, run

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def exe():
    return build("g++", "-std=c++17", os.path.join(ROOT, "tests", "cxx", "mod11n_chain.cpp"), "mod11n_chain")


@pytest.mark.parametrize("mcs,ln,seed", [(9, 37, 0xAB), (11, 150, 0x5B), (12, 301, 0x01), (13, 700, 0xFF)])
def test_brick_graph_of_the_11n_modulator_equals_the_fused_transmitter(tmp_path, exe, mcs, ln, seed):
    import sora_amd
    mpdu = bytes(np.random.default_rng([mcs, ln]).integers(0, 256, ln).astype(np.uint8))
    fin = tmp_path / "mpdu.bin"; fout = tmp_path / "tx.bin"
    fin.write_bytes(mpdu)
    out = run([exe, str(mcs), str(seed), str(fin), str(fout)])
    w0, w1, _ = sora_amd.tx11n([mpdu], [mcs], [seed])
    want = np.concatenate([w0.cpu().numpy()[1600:], w1.cpu().numpy()[1600:]])   # the data symbols of chain 0, then those of chain 1
    assert "%d samples per chain" % (len(want) // 2) in out, out
    got = np.frombuffer(fout.read_bytes(), np.int16).reshape(-1, 2)
    assert got.shape == want.shape and np.array_equal(got, want), np.flatnonzero((got != want).any(axis=1))[:8] if got.shape == want.shape else got.shape
