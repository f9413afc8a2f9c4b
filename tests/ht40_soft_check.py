"""What tests/test_gpu_ht40_soft.py, tests/test_gpu_ht40_joint.py and tests/test_gpu_ht40_front.py share: a descriptor call of the 40 MHz HT data field, read back
whole (rows, soft bytes, exported weights), compared with the integer model (oracle/ht40_data_model.py; joint coding: tests/ht40_joint_model.py) -- every soft
byte, every row field, every PSDU byte.  TEST INFRASTRUCTURE."""
import numpy as np

from oracle import ht40_data_model as dm
import ht40_joint_model as J


# ------------------------------------------------------------------ per-stream coding
def soft_capacity(sora, descs):
    return sum(2 * (sora.ht40_symbols(d[3], d[4], d[1], d[2]) * 108 * d[1] + 64) for d in descs)


def models(iq, descs, w):
    return [dm.model(iq, d[0], d[1], d[2], (d[3], d[4]), d[5], w[f]) for f, d in enumerate(descs)]


def assert_is_the_model(got, want, descs, what=""):
    """every soft byte, every row field and every PSDU byte of every frame and stream"""
    assert len(got["rows"]) == 2 * len(descs)
    for f, d in enumerate(descs):
        for s in range(2):
            tag = (what, f, s, d[1:6])
            assert got["soft"][f][s].shape == want[f].soft[s].shape == (want[f].nsym * 108 * d[1],), tag
            if not np.array_equal(got["soft"][f][s], want[f].soft[s]):
                bad = np.nonzero(got["soft"][f][s] != want[f].soft[s])[0]
                raise AssertionError("%r: %d soft bytes differ, the first in symbol %d (position %d: GPU %d, model %d)"
                                     % (tag, len(bad), bad[0] // (108 * d[1]), bad[0], got["soft"][f][s][bad[0]], want[f].soft[s][bad[0]]))
            r = got["rows"][2 * f + s]; ws = want[f].streams[s]
            assert (r["capture_id"], r["stream"]) == (d[7], s), tag
            assert (r["error_code"], r["length"], r["crc32"]) == (ws.error_code, d[3 + s], ws.crc32), (tag, hex(r["error_code"]), hex(ws.error_code))
            assert r["nsym"] == want[f].nsym and r["mpdu"] == ws.psdu, tag


# ------------------------------------------------------------------ joint coding
def joint_soft_capacity(descs):
    """the handle's rule, unchanged by the coding: 2 x nsym x 108 n_bpsc (+ 64) per frame"""
    return sum(2 * (J.nsym_for(d[3], d[1], d[2]) * 108 * d[1] + 64) for d in descs)


def joint_models(iq, descs, w):
    return [J.rx_model(iq, d[0], d[1], d[2], d[3], d[5], w[f]) for f, d in enumerate(descs)]


def assert_is_the_joint_model(got, want, descs, what=""):
    """every merged soft byte, every row field and every PSDU byte of every frame: ONE row per frame"""
    assert len(got["rows"]) == len(descs), (what, len(got["rows"]))
    for f, d in enumerate(descs):
        tag = (what, f, d[1:6])
        assert got["soft"][f].shape == want[f].soft.shape == (want[f].nsym * 216 * d[1],), tag
        if not np.array_equal(got["soft"][f], want[f].soft):
            bad = np.nonzero(got["soft"][f] != want[f].soft)[0]
            raise AssertionError("%r: %d merged soft bytes differ, the first in symbol %d (position %d: GPU %d, model %d)"
                                 % (tag, len(bad), bad[0] // (216 * d[1]), bad[0], got["soft"][f][bad[0]], want[f].soft[bad[0]]))
        r = got["rows"][f]; wf = want[f]
        assert (r["capture_id"], r["start_sample"], r["stream"]) == (d[7], 0, 0), tag
        assert (r["error_code"], r["length"], r["crc32"]) == (wf.error_code, d[3], wf.crc32), (tag, hex(r["error_code"]), hex(wf.error_code))
        assert r["nsym"] == wf.nsym and r["rate_kbps"] == 10 * d[1] + d[2] and r["mpdu"] == wf.psdu, tag
