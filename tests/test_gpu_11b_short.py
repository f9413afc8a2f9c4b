"""The 802.11b receive handle with the short preamble (sora_rx11b_set_preamble): rows, flags and MPDU bytes equal tests/rx11b_ext_model.py at
mode 1 exactly -- the model tests/test_11b_short_cpu.py pins to the reference's graph at mode 0 and shows to decode short-preamble frames at
mode 1 -- and mode 0 on the same input equals the oracle (and the compiled reference graph where it is built), as before.  Under every pass
plan, through deliver_async, in stream mode, and switching the mode between calls."""
import numpy as np
import pytest

import rx11b_ext_model as rxm
import tx11b_model as txm
from gpu_util import same_as_reference_11b

pytestmark = pytest.mark.gpu
MAXF = 64                             # per capture: the long-only graph raises up to 37 events (SYNC_TIMEOUT by the dozen) on a CCK frame behind a short preamble
E_OK = 0x1


@pytest.fixture(scope="module")
def sora():
    import sora_amd
    if sora_amd.device_count() <= 0:
        pytest.skip("no HIP device")
    return sora_amd


def _frame(rng, rate, ln, kind):
    mp = rng.integers(0, 256, ln).astype(np.uint8).tobytes()
    return txm.tx11b(mp, rate, phase_in=int(rng.integers(0, 4)), preamble=kind)[0]


def _one(rng, spec, cut=None):
    """spec [(rate, length, kind)] -> a capture: the first frame behind 1500..4000 samples, the others at gaps of 300..3000, noise of sigma <= 20;
    cut: samples kept behind the first frame's start"""
    waves = [_frame(rng, *s) for s in spec]
    leads = [int(rng.integers(1500, 4001))] + [int(rng.integers(300, 3001)) for _ in spec[1:]]
    c = rxm.capture(rng, waves, leads, float(rng.uniform(0, 20)))
    return c if cut is None else np.ascontiguousarray(c[:(leads[0] + cut) // 28 * 28])


def make_captures(seed):
    rng = np.random.default_rng(seed)
    caps = []
    for rate in (2000, 5500, 11000):                                    # short only
        for ln in (1, 5, 14, int(rng.integers(100, 301)), int(rng.integers(100, 301))):
            caps.append(_one(rng, [(rate, ln, 1)]))
    for rate in (1000, 2000, 5500, 11000):                              # long only
        for ln in (1, 5, 14, int(rng.integers(100, 301))):
            caps.append(_one(rng, [(rate, ln, 0)]))
    for i in range(36):                                                 # both kinds in one capture
        spec = []
        for j in range(2 + i % 3):
            kind = int(rng.integers(0, 2)) if j else i % 2
            spec.append((int(rng.choice([1000, 2000, 5500, 11000] if kind == 0 else [2000, 5500, 11000])), int(rng.choice([1, 5, 14, 60, 150])), kind))
        caps.append(_one(rng, spec))
    caps.append(_one(rng, [(11000, 100, 1)], cut=72 * 44 + 10 * 44))    # cut inside the short header (its third byte)
    caps.append(_one(rng, [(5500, 100, 1)], cut=60 * 44))               # cut inside the short SFD
    caps.append(_one(rng, [(2000, 50, 1), (2000, 50, 0)], cut=96 * 44 + 54 * 176 + 24 + 400 + 130 * 44))      # ... and inside a long SYNC behind a short frame
    for _ in range(5):                                                  # nothing but noise
        caps.append(np.rint(rng.normal(0, float(rng.choice([10, 300])), (28 * int(rng.integers(50, 400)), 2))).astype(np.int16))
    assert 64 <= len(caps) <= 128
    return caps


class Batch:
    def __init__(self, seed):
        from oracle.pyoracle import Oracle
        o = Oracle()
        self.caps = make_captures(seed)
        self.iq = np.ascontiguousarray(np.concatenate(self.caps)); self.descs = []; off = 0
        for k, c in enumerate(self.caps):
            self.descs.append((off, len(c), k)); off += len(c)
        self.model1 = [rxm.rx11b(c, 1, max_frames=MAXF) for c in self.caps]
        self.oracle0 = [o.rx11b_capture(c, max_frames=MAXF) for c in self.caps]
        assert all(len(r) < MAXF for r in self.model1 + self.oracle0)                           # no list was cut short
        ok = [r for rows in self.model1 for r in rows if r["error_code"] == E_OK]
        assert sum(r["flags"] == 2 for r in ok) >= 50 and sum(r["flags"] == 0 for r in ok) >= 40, len(ok)    # the model decodes both kinds here
        assert not any(r["flags"] for rows in self.oracle0 for r in rows if "flags" in r)

    def want(self, mode):
        rows = self.model1 if mode else self.oracle0
        return [(k,) + rxm.key(dict(r, flags=r.get("flags", 0))) for k, cap in enumerate(rows) for r in cap]


def gpu_key(r):
    return (r["capture_id"],) + rxm.key(r)


@pytest.fixture(scope="module")
def batch():
    return Batch(1130)


@pytest.fixture(scope="module")
def d_iq(batch):
    import torch
    return torch.from_numpy(batch.iq).cuda()


@pytest.mark.parametrize("plan", [0, 1, 2])
def test_rows_equal_the_model_under_every_pass_plan(sora, batch, d_iq, plan):
    rx = sora.Rx11b(len(batch.caps), len(batch.iq), max_frames_per_capture=MAXF)
    rx.set_single_pass(plan)
    assert rx.set_preamble(1) == 0 and rx.set_preamble(-1) == 1
    buf = sora.HostResults(len(batch.caps) * MAXF, 1 << 20)
    for rep in range(3):                                                # (plan 2 measures on its first call and may take the single pass afterwards)
        t = rx.process_dev(d_iq, batch.descs)
        rx.deliver_async(t, buf)
        rx.wait(t)
        got = [gpu_key(r) for r in buf.results()]
        assert got == batch.want(1), (plan, rep)
        assert [gpu_key(r) for r in rx.results(ticket=t)] == got, (plan, rep)
    assert rx.set_preamble(0) == 1
    t = rx.process_dev(d_iq, batch.descs)
    rx.deliver_async(t, buf)
    rx.wait(t)
    got = [gpu_key(r) for r in buf.results()]
    assert got == batch.want(0) and [gpu_key(r) for r in rx.results(ticket=t)] == got, plan
    buf.close(); rx.close()


def test_mode_0_equals_the_compiled_reference_graph(sora, batch, d_iq):
    from oracle.pyoracle import ReferenceGraph
    g = ReferenceGraph()
    if not g.available():
        pytest.skip("oracle/_ref/libsora_refgraph.so not present")
    rx = sora.Rx11b(len(batch.caps), len(batch.iq), max_frames_per_capture=MAXF)
    assert rx.set_preamble(-1) == 0                                     # the default
    rx.process_dev(d_iq, batch.descs)
    rows = rx.results(); rx.close()
    for k, c in enumerate(batch.caps):
        ok, why = same_as_reference_11b([r for r in rows if r["capture_id"] == k], g.rx11b(c, max_frames=MAXF))
        assert ok, (k, why)


def test_each_call_runs_in_its_own_mode(sora, batch, d_iq):
    """0 -> 1 -> 0 -> 1 on one handle, calls issued back to back (the switch waits for the calls in flight); a bad mode is refused and changes nothing"""
    rx = sora.Rx11b(len(batch.caps), len(batch.iq), max_frames_per_capture=MAXF)
    tickets = []
    for mode in (0, 1, 0, 1):
        rx.set_preamble(mode)
        tickets.append((rx.process_dev(d_iq, batch.descs), mode))
        if len(tickets) >= 2:
            t, m = tickets[-2]
            assert [gpu_key(r) for r in rx.results(ticket=t)] == batch.want(m), (t, m)
    with pytest.raises(sora.SoraError):
        rx.set_preamble(2)
    assert rx.set_preamble(-1) == 1
    t, m = tickets[-1]
    assert [gpu_key(r) for r in rx.results(ticket=t)] == batch.want(m)
    rx.close()


@pytest.mark.parametrize("plan", [0, 2])
def test_stream_mode_pieces_equal_the_model_on_the_uncut_stream(sora, plan):
    """Short and long frames in one stream, handed over in pieces cut at random source calls (tests/test_gpu_stream11b.py's pattern): the rows of
    all pieces together are the model's rows on the uncut stream."""
    import torch
    rng = np.random.default_rng(1140 + plan)
    spec = [(int(rng.choice([2000, 5500, 11000])), int(rng.choice([1, 14, 60, 200])), 1) if j % 2 == 0 else
            (int(rng.choice([1000, 2000, 5500, 11000])), int(rng.choice([5, 40, 120])), 0) for j in range(12)]
    waves = [_frame(rng, *s) for s in spec]
    stream = rxm.capture(rng, waves, [2000] + [int(rng.integers(300, 3001)) for _ in spec[1:]], 10.0, tail=28 * 150)
    want = rxm.rx11b(stream, 1, max_frames=256)
    assert sum(r["error_code"] == E_OK for r in want) == len(spec) and sum(r["flags"] == 2 for r in want) == 6
    rx = sora.Rx11b(1, len(stream) + 28, max_frames_per_capture=MAXF)
    rx.set_single_pass(plan)
    assert rx.set_preamble(1) == 0 and rx.set_stream_mode(1) == 0
    base = arrived = calls = 0
    got = []
    while True:
        arrived = min(len(stream), max(arrived, base) + 28 * int(rng.integers(1, 600)))
        n = (arrived - base) // 28 * 28
        last = base + n + 28 > len(stream)
        seg = np.ascontiguousarray(stream[base:base + n]) if n else np.zeros((28, 2), np.int16)
        t = rx.process_dev(torch.from_numpy(seg).cuda(), [(0, n, 0)])
        rows = rx.results(ticket=t)
        used = int(rx.stream_consumed(t, 1)[0])
        assert all(r["end_sample"] <= used for r in rows)
        got += [dict(r, end_sample=r["end_sample"] + base) for r in rows]
        base += used; calls += 1
        if last and (used == 0 or len(stream) - base < 28):
            break
        assert calls < 1000
    rx.close()
    assert calls >= 10
    assert [rxm.key(r) for r in got] == [rxm.key(r) for r in want]
