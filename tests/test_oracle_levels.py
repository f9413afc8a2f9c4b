"""The CPU restatements at full-scale, DC-shifted and near-silent levels: every capture of tests/level_captures.py through so_rx11a_capture at 40 MHz,
the 44 MHz mode behind so_down44to40, so_rx11b_capture and so_rx11n_capture, event for event against what the compiled reference graphs reported for
it (tests/golden/refgraph_levels.npz) -- and against those graphs live where oracle/_ref is built, which also shows the fixture to be current.  The
802.11n extension model (tests/rx11n_ext_model.py), with its gate at the reference's 10, is held to the same events."""
import pytest

import level_captures as lc
from oracle.pyoracle import Oracle, ReferenceGraph


@pytest.fixture(scope="module")
def o():
    return Oracle()


def _differences(caps, got, want, what):
    return ["%s: %s %r, reference %r" % (c.name, what, g, w) for c, g, w in zip(caps, got, want) if g != w]


@pytest.mark.parametrize("chain", lc.CHAINS)
def test_oracle_equals_the_reference_graph_at_every_level(o, chain):
    caps = lc.chain(chain, o)
    want = lc.recorded(chain, caps)
    assert all(len(w) < lc.MAX_EVENTS[chain] for w in want)                         # no recorded list was cut short
    bad = _differences(caps, [lc.run_oracle(o, chain, c) for c in caps], want, "oracle")
    assert not bad, "%d of %d captures differ; first: %s" % (len(bad), len(caps), bad[0])
    g = ReferenceGraph()
    if g.available():
        bad = _differences(caps, [lc.run_reference(g, chain, c) for c in caps], want, "live graph")
        assert not bad, "the recorded events are not what oracle/_ref reports now (%d captures); first: %s" % (len(bad), bad[0])


def test_extension_model_equals_the_reference_graph_at_every_level():
    """tests/rx11n_ext_model.py is the GPU handle's reference once sora_rx11n_set_mcs_max(14) is called (tests/test_gpu_levels.py); with the gate at 10 it is
    the reference's graph and reports the recorded events -- it takes its carrier-offset estimate, dsp_atan32 included, from the oracle's stage functions."""
    import rx11n_ext_model as model
    caps = lc.chain("11n")
    want = lc.recorded("11n", caps)
    got = [lc.row_events("11n", model.rx11n(c.iq[0], c.iq[1], mcs_max=10, max_frames=lc.MAX_EVENTS["11n"])) for c in caps]
    bad = _differences(caps, got, want, "model")
    assert not bad and model.parser_disagreements() == 0, "%d of %d captures differ; first: %s" % (len(bad), len(caps), bad[:1])


@pytest.mark.parametrize("chain", lc.CHAINS)
def test_every_family_holds_work(o, chain):
    """Counted on the recorded reference events alone.  overdriven: decoded frames next to broken ones (for 802.11b: its own failure codes, SYNC_TIMEOUT
    above all); near-silent: at least a quarter of the captures with a frame and a quarter without any event, so the carrier-sense threshold lies inside
    the family; the quietest gain leaves 1-3 LSB."""
    caps = lc.chain(chain, o)
    n = lc.census(caps, lc.recorded(chain, caps))
    assert set(n) == set(lc.FAMILIES) and sum(f["captures"] for f in n.values()) == len(caps) >= 150
    over = n["overdriven"]["codes"]
    if chain == "11b":
        assert over.get(lc.E_OK, 0) >= 5 and over.get(lc.E_CRC, 0) >= 5 and over.get(0x80000009, 0) >= 100 and over.get(0x80000008, 0) >= 1, over
    else:
        assert over.get(lc.E_OK, 0) >= 10 and over.get(lc.E_PLCP, 0) >= 10 and over.get(lc.E_CRC, 0) >= 3, over
    decoded = {e[2] for w in lc.recorded(chain, caps) for e in w if e[0] == lc.E_OK}         # every rate, every MCS of the reference's gate
    assert decoded >= {"11b": {1000, 2000, 5500, 11000}, "11n": {8, 9, 10}}.get(chain, set(lc.RATES_11A)), decoded
    quiet = n["silent"]
    assert 4 * quiet["framed"] >= quiet["captures"] and 4 * quiet["mute"] >= quiet["captures"], quiet
    assert n["offset"]["framed"] * 2 >= n["offset"]["captures"] and n["rails"]["framed"] >= 5 and n["stream"]["framed"] == 1
    lowest = [c for c in caps if c.family == "silent"][-1]                   # the last gain of the list, on a noise floor of +-2
    peak = max(int(abs(x.astype(int)).max()) for x in (lowest.iq if isinstance(lowest.iq, tuple) else (lowest.iq,)))
    assert 1 <= peak <= 6, peak
    rails = [c for c in caps if c.family == "rails"]
    lone = [c for c in rails if "lone" in c.name]
    for c in lone if chain != "11a44" else []:                              # the only extreme value is -32768 (before the interpolation to 44 MHz)
        for x in (c.iq if isinstance(c.iq, tuple) else (c.iq,)):
            assert x.min() == -32768 and x.max() < 32767
