"""tests/cxx/demod11b_chain.cpp EXECUTED on the GPU box (-m gpu): the byte paths of the 802.11b receive graph built sink-first from the BRICK adapters of
include/sora_brick.hpp (despreader -> DBPSK / DQPSK demapper -> descrambler; CCK 5.5 / 11 decoder -> descrambler, one byte per burst, the context in one shared device
record), compiled and linked like a user's program and run as a separate process on the payload chips of a decoded frame.  What its sink collects is the stage model's
bytes -- and the frame that was sent."""
import os

import numpy as np
import pytest

import rx11b_stage_model as sm
import stage11b_captures as sc
from test_gpu_hosts import ROOT, build, run

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def exe():
    return build("g++", "-std=c++17", os.path.join(ROOT, "tests", "cxx", "demod11b_chain.cpp"), "demod11b_chain")


@pytest.mark.parametrize("name,kind", [("long-1000-33", 1), ("long-2000-33", 2), ("short-5500-120", 5), ("long-11000-120", 11)])
def test_adapter_chain_equals_the_model(tmp_path, exe, name, kind):
    caps = sc.all_captures()
    index = [c.name for c in caps].index(name)
    s = sc.streams(index)
    chips = s["last_despread_chips"] if kind in (1, 2) else s["payload_chips"]
    state = s["payload_state"].copy()
    stage = {1: "dbpsk", 2: "dqpsk", 5: "cck5p5", 11: "cck11"}[kind]
    assert s["payload_kind"] == stage and state[2] == 0
    raw, st = sm.stream_stage(stage, sm.despread(chips) if kind in (1, 2) else chips, state)
    want, _ = sm.stream_stage("desc741", raw, st)
    mp = caps[index].mpdu
    assert len(want) == len(mp) + 3 and want[:len(mp)].tobytes() == mp           # the frame that was sent, and three of its FCS bytes
    fin = tmp_path / "chips.bin"; fout = tmp_path / "bytes.bin"
    fin.write_bytes(np.ascontiguousarray(chips, np.int16).tobytes())
    out = run([exe, str(kind), str(fin), str(int(state[0]) & 0xFFFFFFFF), str(int(state[1]) & 0xFF), str(fout)])
    assert "%d bytes out" % len(want) in out, out
    assert fout.read_bytes() == want.tobytes()
