"""tests/cxx/mod_chain.cpp EXECUTED on the GPU box (-m gpu): the 802.11a modulation graph built sink-first from the BRICK adapters of include/sora_brick.hpp
(scrambler -> encoder -> interleaver -> mapper -> pilots -> IFFT -> [upsampler] -> pack, the SIGNAL branch joining at the pilot brick, one symbol per burst),
compiled and linked like a user's program and run as a separate process.  What its sink collects is the fused transmitter's frame, byte for byte."""
import os

import numpy as np
import pytest

from test_gpu_hosts import ROOT, build, run

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def exe():
    return build("g++", "-std=c++17", os.path.join(ROOT, "tests", "cxx", "mod_chain.cpp"), "mod_chain")


@pytest.mark.parametrize("rate,ln,seed,mhz", [(6000, 37, 0xFF, 40), (18000, 260, 0x5B, 40), (24000, 100, 0x01, 44), (48000, 301, 0xFF, 40), (54000, 700, 0x80, 44)])
def test_brick_graph_of_the_modulator_equals_the_fused_transmitter(tmp_path, exe, rate, ln, seed, mhz):
    import sora_amd
    mpdu = bytes(np.random.default_rng([rate, ln]).integers(0, 256, ln).astype(np.uint8))
    fin = tmp_path / "mpdu.bin"; fout = tmp_path / "tx.bin"
    fin.write_bytes(mpdu)
    out = run([exe, str(rate), str(seed), str(fin), str(fout)] + (["44"] if mhz == 44 else []))
    want, _ = sora_amd.tx11a([mpdu], [rate], [seed], sample_rate_mhz=mhz)
    want = want.cpu().numpy()
    assert "%d samples out" % len(want) in out, out
    got = np.frombuffer(fout.read_bytes(), np.int8).reshape(-1, 2)
    assert got.shape == want.shape and np.array_equal(got, want), np.flatnonzero((got != want).any(axis=1))[:8] if got.shape == want.shape else got.shape
