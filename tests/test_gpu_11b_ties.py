"""The 802.11b receive handle where CCK metrics and AdjustTiming's energies tie (tests/ties11b_captures.py): strict comparisons decide bits there, and the
handle takes them from the shared pieces of sora_amd/csrc/dev_11b.h -- the code-word tree in cck11_decode and bulk_pass, the 5.5 Mbps half byte, the early-late
decision -- while its parity tests run on random captures, where ties are rare.  CPU part: the planted chips are what reaches the model's CCK decoder, and
tests/rx11b_ext_model.py at mode 0 equals oracle/so_rx11b.c (and the compiled reference graph where it is built) on these captures.  GPU part: rows and MPDU bytes
of the handle equal the model's under the two-pass plan, the single-pass plan and in stream mode."""
import numpy as np
import pytest

import rx11b_ext_model as rxm
import ties11b_captures as tc
from gpu_util import same_as_reference_11b

MAXF = 64
E_CRC32_FAIL = 0x80000006


@pytest.fixture(scope="module")
def caps():
    return tc.captures()


@pytest.fixture(scope="module")
def want(caps):
    """per capture, the model's events at the capture's preamble mode"""
    rows = [rxm.rx11b(c.iq, c.mode, max_frames=MAXF) for c in caps]
    assert all(len(r) < MAXF for r in rows)
    return rows


def test_the_planted_chips_are_what_the_models_decoder_is_given(caps, want):
    assert [c.name for c in caps] == list(tc.NAMES)
    for c, rows in zip(caps, want):
        got = tc.reaching_the_decoder(c)
        assert len(got) == len(c.planted) and np.array_equal(got, c.planted), c.name
        # the frame is delivered whole with a failing FCS: every MPDU byte and the FCS word
        first = rows[0]
        assert first["error_code"] == E_CRC32_FAIL and first["rate_kbps"] == int(c.name.split("-")[1]) and first["length"] == int(c.name.split("-")[2]) + 4, (c.name, first)
        assert len(first["mpdu"]) == first["length"] and first["flags"] == (2 if c.mode else 0), c.name


def test_the_model_at_mode_0_equals_the_oracle_and_the_reference_graph(caps):
    from oracle.pyoracle import Oracle, ReferenceGraph
    o = Oracle(); g = ReferenceGraph()
    for c in caps:
        m0 = rxm.rx11b(c.iq, 0, max_frames=MAXF)
        assert len(m0) < MAXF
        assert [rxm.key(r) for r in m0] == [rxm.key(dict(r, flags=0)) for r in o.rx11b_capture(c.iq, max_frames=MAXF)], c.name
        if g.available():
            ok, why = same_as_reference_11b(m0, g.rx11b(c.iq, max_frames=MAXF))
            assert ok, (c.name, why)


@pytest.fixture(scope="module")
def sora():
    import sora_amd
    if sora_amd.device_count() <= 0:
        pytest.skip("no HIP device")
    return sora_amd


def _rows(rx, t, base=None):
    out = {}
    for r in rx.results(ticket=t):
        k = r["capture_id"]
        out.setdefault(k, []).append(rxm.key(r if base is None else dict(r, end_sample=r["end_sample"] + base[k])))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("plan", [0, 1])
def test_rows_equal_the_model_under_the_two_pass_and_the_single_pass_plan(sora, caps, want, plan):
    import torch
    iq = np.ascontiguousarray(np.concatenate([c.iq for c in caps])); descs = []; off = 0
    for k, c in enumerate(caps):
        descs.append((off, len(c.iq), k)); off += len(c.iq)
    d_iq = torch.from_numpy(iq).cuda()
    rx = sora.Rx11b(len(caps), len(iq), max_frames_per_capture=MAXF)
    rx.set_single_pass(plan)
    for mode in (0, 1):                                                 # a call runs wholly in one mode: each capture is compared in the call of its own
        rx.set_preamble(mode)
        got = _rows(rx, rx.process_dev(d_iq, descs))
        for k, c in enumerate(caps):
            if c.mode == mode:
                assert got.get(k, []) == [rxm.key(r) for r in want[k]], (plan, c.name)
    rx.close()


@pytest.mark.gpu
def test_stream_mode_pieces_equal_the_model(sora, caps):
    """every capture in two pieces, cut at a multiple of 28 samples inside the silence in front of its frame; preamble mode 1 throughout"""
    import torch
    want1 = [[rxm.key(r) for r in rxm.rx11b(c.iq, 1, max_frames=MAXF)] for c in caps]
    cuts = [(c.frame_at // 2) // 28 * 28 for c in caps]
    assert all(28 <= cut < c.frame_at - 28 for cut, c in zip(cuts, caps))
    rx = sora.Rx11b(len(caps), sum(len(c.iq) for c in caps), max_frames_per_capture=MAXF)
    assert rx.set_preamble(1) == 0 and rx.set_stream_mode(1) == 0
    base = [0] * len(caps); ends = cuts
    got = {}
    for piece in range(2):
        segs = [np.ascontiguousarray(c.iq[b:e]) for c, b, e in zip(caps, base, ends)]
        descs = []; off = 0
        for k, s in enumerate(segs):
            assert len(s) % 28 == 0
            descs.append((off, len(s), k)); off += len(s)
        t = rx.process_dev(torch.from_numpy(np.ascontiguousarray(np.concatenate(segs))).cuda(), descs)
        for k, rows in _rows(rx, t, base).items():
            got.setdefault(k, []).extend(rows)
        used = rx.stream_consumed(t, len(caps))
        base = [b + int(u) for b, u in zip(base, used)]
        ends = [len(c.iq) for c in caps]
    rx.close()
    for k, c in enumerate(caps):
        assert got.get(k, []) == want1[k], c.name
