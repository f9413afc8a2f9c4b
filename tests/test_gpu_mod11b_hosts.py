"""tests/cxx/mod11b_chain.cpp EXECUTED on the GPU box (-m gpu): the 802.11b modulation graph built sink-first from the BRICK adapters of include/sora_brick.hpp
(scrambler -> the host's rate select -> the four spreaders -> pulse shaper -> TPackSample16to8, one byte and then two chips per burst), compiled and linked like a
user's program and run as a separate process.  What its sink collects is the fused transmitter's frame, sample for sample."""
import os

import numpy as np
import pytest

from test_gpu_hosts import ROOT, build, run

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def exe():
    return build("g++", "-std=c++17", os.path.join(ROOT, "tests", "cxx", "mod11b_chain.cpp"), "mod11b_chain")


@pytest.mark.parametrize("rate,kind,ln", [(1000, 0, 37), (2000, 1, 150), (5500, 0, 301), (11000, 1, 700)])
def test_brick_graph_of_the_11b_modulator_equals_the_fused_transmitter(tmp_path, exe, rate, kind, ln):
    import sora_amd
    mpdu = bytes(np.random.default_rng([rate, ln]).integers(0, 256, ln).astype(np.uint8))
    fin = tmp_path / "mpdu.bin"; fout = tmp_path / "tx.bin"
    fin.write_bytes(mpdu)
    out = run([exe, str(rate), str(kind), str(fin), str(fout)])
    want = sora_amd.tx11b([mpdu], [rate], preamble=[kind])[0].cpu().numpy()
    assert "%d samples out" % len(want) in out, out
    got = np.frombuffer(fout.read_bytes(), np.int8).reshape(-1, 2)
    assert got.shape == want.shape and np.array_equal(got, want), np.flatnonzero((got != want).any(axis=1))[:8] if got.shape == want.shape else got.shape
