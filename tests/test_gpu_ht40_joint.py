"""The 40 MHz HT receive handle in JOINT coding (sora_ht40_set_coding(rx, SORA_HT40_CODING_JOINT)), descriptor form, held BIT FOR BIT to
the integer model tests/ht40_joint_model.py::rx_model from the detection weights on, as tests/test_gpu_ht40_soft.py holds the per-stream coding to
oracle/ht40_data_model.py: every MERGED soft byte (sora_ht40_soft_of, stream 0), every row field (capture_id, start_sample, error_code, length, crc32, nsym, rate_kbps)
and every PSDU byte, of frames that pass and of frames that FAIL their FCS.  No tolerance; no frame, byte or field left out.  The model takes the GPU's exported
weights (their own arithmetic is held in tests/test_gpu_ht40.py); its per-stream soft bytes are the pinned ones, de-parsed by the stream parser's rule."""
import numpy as np
import pytest

from oracle import ht40_data_model as dm
from oracle import py_ht40 as m
import ht40_joint_model as J
from ht40_soft_check import assert_is_the_joint_model as assert_is_the_model, joint_models as models, joint_soft_capacity as soft_capacity
from test_gpu_ht40_soft import GRID_RATES, H0, adversarial_inputs, place
from test_gpu_ht40_soft import lengths_for as per_stream_lengths_for, real_frame as per_stream_frame

pytestmark = pytest.mark.gpu

FRAME_OK, CRC32_FAIL = 1, 0x80000006


@pytest.fixture(scope="module")
def env():
    import torch
    import sora_amd
    if sora_amd.device_count() <= 0:
        pytest.skip("no HIP device")
    return torch, sora_amd


# ------------------------------------------------------------------ inputs
def length_for(nb, cr, nsym, rng):
    """a PSDU length (>= 5) that needs exactly nsym symbols in joint coding"""
    nd = J.ndbps(nb, cr)
    top = (nsym * nd - 22) // 8
    low = max(5, ((nsym - 1) * nd - 22) // 8 + 1)
    assert top >= low, (nb, cr, nsym)
    ln = int(rng.integers(low, top + 1))
    assert J.nsym_for(ln, nb, cr) == nsym
    return ln


def real_frame(rng, nb, cr, length, sigma, cfo_step=0.0):
    """a joint-coded frame of the float model through the 2x2 channel -> int16 [2, (2 + nsym) * 160, 2], psdu"""
    psdu = m.add_fcs(rng.integers(0, 256, length - 4, dtype=np.uint8).tobytes())
    x, nsym = J.tx_joint(psdu, nb, cr, seed=int(rng.integers(1, 128)))
    return m.channel(x, H0, sigma, rng, cfo_step=cfo_step), psdu


# ------------------------------------------------------------------ one call, read back whole
def gpu_call(env, iq, descs, want_w=True, trellis=None):
    """-> dict: rows (results), soft[frame] (the merged bytes), w int16 [nframes, 4, 128, 2] or None"""
    torch, sora = env
    rx = sora.RxHt40(len(descs), soft_capacity(descs))
    assert rx.set_coding(sora.HT40_CODING_JOINT) == sora.HT40_CODING_PER_STREAM and rx.set_coding() == sora.HT40_CODING_JOINT
    if trellis is not None:
        rx.set_trellis(trellis)
    w = torch.zeros((len(descs), 4, 128, 2), dtype=torch.int16, device="cuda") if want_w else None
    t = rx.process_dev(torch.from_numpy(iq[0].copy()).cuda(), torch.from_numpy(iq[1].copy()).cuda(), descs, w)
    rows = rx.results(ticket=t)
    soft = [rx.soft(f, 0, ticket=t) for f in range(len(descs))]
    rx.close()
    return {"rows": rows, "soft": soft, "w": w.cpu().numpy() if want_w else None}


# ------------------------------------------------------------------ the shape grid
@pytest.fixture(scope="module")
def grid():
    """n_bpsc 1, 2, 4, 6 (s = 1, 1, 2, 3) x nsym 1, 2, 3, 12, code rates as GRID_RATES; ordered so that every workgroup of four frames holds all four n_bpsc.
    -> [(segment, descriptor tail (nb, cr, length, 0), psdu)]"""
    rng = np.random.default_rng(5001)
    out = []
    for col, nsym in enumerate((1, 2, 3, 12)):
        for nb in (1, 2, 4, 6):
            cr = GRID_RATES[nb][col]
            ln = length_for(nb, cr, nsym, rng)
            seg, psdu = real_frame(rng, nb, cr, ln, 6.0)
            assert seg.shape[1] == (2 + nsym) * 160
            out.append((seg, (nb, cr, ln, 0), psdu))
    return out


def describe(bank, offs):
    """descriptors of frames of the grid: cfo 0, the noise variance of sigma 6 in the FFT<128> output's units (MMSE mode), frame ids 100..."""
    return [(offs[i],) + b[1] + (0, 2 * 6.0 * 6.0 / 128.0, 100 + i) for i, b in enumerate(bank)]


def test_shape_grid_every_soft_byte_row_and_psdu(env, grid):
    iq, offs = place([g[0] for g in grid])
    descs = describe(grid, offs)
    got = gpu_call(env, iq, descs)
    want = models(iq, descs, got["w"])
    assert_is_the_model(got, want, descs, "grid")
    for f, g in enumerate(grid):                                          # these are clean frames: the model (and so the GPU) decodes them
        assert (want[f].error_code, want[f].psdu) == (FRAME_OK, g[2]), f


@pytest.mark.parametrize("nframes", [1, 3, 4, 5])
def test_batch_layouts_partial_full_and_a_lone_trellis_job(env, grid, nframes):
    """a partial workgroup, a full one and one frame more; one job per frame, so a code-rate list of an odd count ends in a wave with one job"""
    pick = [grid[(5 * i + nframes) % 16] for i in range(nframes)]
    per_rate = [sum(1 for p in pick if p[1][1] == r) for r in range(3)]
    assert any(c % 2 for c in per_rate), per_rate
    iq, offs = place([g[0] for g in pick])
    descs = describe(pick, offs)
    got = gpu_call(env, iq, descs)
    assert_is_the_model(got, models(iq, descs, got["w"]), descs, "batch of %d" % nframes)


def test_frame_offsets_off_every_alignment_and_the_last_frame_ends_the_buffer(env, grid):
    mods = [0, 1, 2, 3, 5, 63]
    pick = [grid[i] for i in (12, 1, 6, 11, 0, 13)]
    iq, offs = place([g[0] for g in pick], mods)
    assert [o % 64 for o in offs] == mods and offs[0] == 0 and any(o % 4 for o in offs)
    assert offs[-1] + pick[-1][0].shape[1] == iq.shape[1]                  # the kernel reads up to, and not past, the last sample
    descs = describe(pick, offs)
    got = gpu_call(env, iq, descs)
    assert_is_the_model(got, models(iq, descs, got["w"]), descs, "offsets")


# ------------------------------------------------------------------ real frames: noise, carrier offsets, both detectors
def test_real_frames_that_pass_and_that_fail_cfo_and_both_detectors(env):
    """64-QAM 3/4 at sigma 6 (they pass) and at sigma 150 (1200 .. 1500 bytes: dozens of byte errors in the zero-forcing model, so they fail under either
    detector), zero forcing and MMSE, cfo 0, 37, -511, 4096"""
    rng = np.random.default_rng(5002)
    segs, tails, nvs, cfos, sig = [], [], [], [], []
    for cfo in (0, 37, -511, 4096):
        for sigma, nv in ((6.0, 0.0), (6.0, 3000.0), (150.0, 0.0), (150.0, 3000.0)):
            ln = int(rng.integers(120, 400)) if sigma < 100 else int(rng.integers(1200, 1500))
            seg, _ = real_frame(rng, 6, 2, ln, sigma, cfo_step=-float(cfo))
            segs.append(seg); tails.append((6, 2, ln, 0)); nvs.append(nv); cfos.append(cfo); sig.append(sigma)
    iq, offs = place(segs, [int(v) for v in rng.integers(0, 64, len(segs))])
    descs = [(offs[i],) + tails[i] + (cfos[i], nvs[i], i) for i in range(len(segs))]
    got = gpu_call(env, iq, descs)
    want = models(iq, descs, got["w"])
    # the model first: the loud frames fail, the quiet ones pass
    assert [w.error_code for w, s in zip(want, sig) if s < 100] == [FRAME_OK] * 8, [hex(w.error_code) for w in want]
    assert [w.error_code for w, s in zip(want, sig) if s > 100] == [CRC32_FAIL] * 8, [hex(w.error_code) for w in want]
    assert_is_the_model(got, want, descs, "real frames")                   # rows and bytes of FAILED frames are compared too
    assert [r["error_code"] for r in got["rows"]].count(CRC32_FAIL) >= 4


# ------------------------------------------------------------------ no frame at all: the saturating paths
def test_adversarial_input_saturating_paths_both_detectors(env):
    """tests/test_gpu_ht40_soft.py's inputs (noise, rails, constants, quiet HT-LTFs in front of full-scale data): a described frame that is not there"""
    inputs = adversarial_inputs()
    rng = np.random.default_rng(5004)
    singular = inputs[2][1].copy(); singular[1] = singular[0]
    segs, tails = [], []
    for i, (name, seg) in enumerate(inputs):
        for nv in (0.0, 3000.0):
            nb = (1, 2, 4, 6)[(i + (nv > 0)) % 4]; cr = (0, 2, 0, 1)[(i + (nv > 0)) % 4]
            segs.append(seg); tails.append((nb, cr, length_for(nb, cr, 3, rng), 0, int(rng.choice([0, 37, -511, 4096])), nv))
    segs.append(singular); tails.append((4, 0, length_for(4, 0, 3, rng), 0, 0, 0.0))
    iq, offs = place(segs, [int(v) for v in rng.integers(0, 64, len(segs))])
    descs = [(offs[i],) + tails[i] + (i,) for i in range(len(segs))]
    got = gpu_call(env, iq, descs)
    want = models(iq, descs, got["w"])
    assert_is_the_model(got, want, descs, "adversarial")
    occ = dm.OCCUPIED_BINS
    for zf in (True, False):                                               # the saturating paths were really reached, under both detectors
        fr = [f for f, d in enumerate(descs) if (d[6] == 0.0) == zf]
        xsat = sum(int(np.sum((want[f].xs[:, :, occ] == 32767) | (want[f].xs[:, :, occ] == -32768))) for f in fr)
        assert xsat > 0, ("zero forcing" if zf else "MMSE", xsat)


# ------------------------------------------------------------------ variants of the same call
def test_without_weight_export_and_with_either_trellis_nothing_changes(env, grid):
    rng = np.random.default_rng(5005)
    pick = [grid[i] for i in (15, 2, 9, 4, 14)]
    seg, _ = real_frame(rng, 6, 2, 1300, 150.0)                           # ... and a frame too noisy to decode
    pick.append((seg, (6, 2, 1300, 0), None))
    iq, offs = place([g[0] for g in pick], [int(v) for v in rng.integers(0, 64, len(pick))])
    descs = describe(pick, offs)
    base = gpu_call(env, iq, descs)
    want = models(iq, descs, base["w"])
    assert_is_the_model(base, want, descs, "with d_weights")
    assert any(r["error_code"] == CRC32_FAIL for r in base["rows"])
    for trellis, want_w in ((None, False), (16, False), (64, False), (64, True)):
        assert_is_the_model(gpu_call(env, iq, descs, want_w=want_w, trellis=trellis), want, descs, "trellis %s, d_weights %s" % (trellis, want_w))


@pytest.mark.parametrize("mcs", [8, 11, 13, 14])
def test_the_longest_frames(env, mcs):
    """LENGTH 4000: MCS 8 (297 symbols, 64152 soft bytes), MCS 11 (64800 soft bytes: the largest decoder job), MCS 13 (32832 field bits: the largest bit field,
    4104 decoded bytes), MCS 14"""
    nb, cr = m.MCS2[mcs]
    rng = np.random.default_rng(5100 + mcs)
    seg, psdu = real_frame(rng, nb, cr, 4000, 6.0)
    for trellis in (16, 64):
        iq, offs = place([seg], [5])
        descs = [(offs[0], nb, cr, 4000, 0, 0, 0.0, 9)]
        got = gpu_call(env, iq, descs, trellis=trellis)
        want = models(iq, descs, got["w"])
        assert_is_the_model(got, want, descs, "LENGTH 4000, MCS %d, trellis %d" % (mcs, trellis))
        assert (want[0].error_code, want[0].psdu) == (FRAME_OK, psdu)
    if mcs == 8:
        assert want[0].nsym == 297 and len(want[0].soft) == 64152
    if mcs == 11:
        assert len(want[0].soft) == 64800


def test_refusals_and_switching_the_coding_back(env, grid):
    torch, sora = env
    pick = [grid[i] for i in (5, 10, 3)]
    iq, offs = place([g[0] for g in pick])
    descs = describe(pick, offs)
    d0, d1 = torch.from_numpy(iq[0].copy()).cuda(), torch.from_numpy(iq[1].copy()).cuda()
    rx = sora.RxHt40(4, 1 << 16)
    assert rx.set_coding() == 0 and rx.set_coding(1) == 0
    with pytest.raises(sora.SoraError) as e:                              # no such coding
        rx.set_coding(2)
    assert e.value.code == -1 and rx.set_coding() == 1
    bad = [descs[0], descs[1][:4] + (7,) + descs[1][5:], descs[2]]
    with pytest.raises(sora.SoraError) as e:                              # a second PSDU length in joint coding: refused before anything is launched
        rx.process_dev(d0, d1, bad)
    assert e.value.code == -1 and "length[1] must be 0" in str(e.value)
    w = torch.zeros((3, 4, 128, 2), dtype=torch.int16, device="cuda")
    t = rx.process_dev(d0, d1, descs, w)
    want = models(iq, descs, w.cpu().numpy())
    assert [(r["error_code"], r["mpdu"]) for r in rx.results(ticket=t)] == [(x.error_code, x.psdu) for x in want]
    assert np.array_equal(rx.soft(2, 0, ticket=t), want[2].soft)
    for frame, stream in ((0, 1), (2, 1), (3, 0)):                        # joint coding has one stream of soft bytes per frame
        with pytest.raises(sora.SoraError) as e:
            rx.soft(frame, stream, ticket=t)
        assert e.value.code == -1
    # back to the per-stream coding: the handle is the per-stream handle again, held to the per-stream model
    assert rx.set_coding(0) == 1 and rx.set_coding() == 0
    rng = np.random.default_rng(5006)
    lens = per_stream_lengths_for(4, 2, 3, 1, rng)
    seg, ps = per_stream_frame(rng, 4, 2, lens, 6.0)
    pd = [(0, 4, 2, lens[0], lens[1], 0, 0.0, 77)]
    w1 = torch.zeros((1, 4, 128, 2), dtype=torch.int16, device="cuda")
    t = rx.process_dev(torch.from_numpy(seg[0].copy()).cuda(), torch.from_numpy(seg[1].copy()).cuda(), pd, w1)
    rows = rx.results(ticket=t)
    ref = dm.model(seg, 0, 4, 2, lens, 0, w1.cpu().numpy()[0])
    assert len(rows) == 2
    for s in range(2):
        assert np.array_equal(rx.soft(0, s, ticket=t), ref.soft[s]), s
        assert (rows[s]["stream"], rows[s]["error_code"], rows[s]["length"], rows[s]["crc32"], rows[s]["mpdu"]) == \
               (s, ref.streams[s].error_code, lens[s], ref.streams[s].crc32, ref.streams[s].psdu) and rows[s]["mpdu"] == ps[s]
    rx.synchronize(); rx.close()


def test_per_stream_psdus_beyond_one_crc_pass(env):
    """The finisher both codings share checks the FCS with a 64-lane CRC that covers 2560 bytes a pass; PSDUs of up to 4000 bytes take a second pass.  The
    per-stream coding, lengths on both sides of the step (2564 = 2560 + FCS) and the longest: rows, soft bytes and PSDUs are oracle/ht40_data_model.py's"""
    torch, sora = env
    rng = np.random.default_rng(5007)
    for lens in ((2564, 2565), (4000, 2700)):
        seg, ps = per_stream_frame(rng, 6, 2, lens, 6.0)
        pd = [(0, 6, 2, lens[0], lens[1], 0, 0.0, 5)]
        rx = sora.RxHt40(1, 2 * (m.nsym_for(list(lens), 6, 2) * 648 + 64))
        w = torch.zeros((1, 4, 128, 2), dtype=torch.int16, device="cuda")
        t = rx.process_dev(torch.from_numpy(seg[0].copy()).cuda(), torch.from_numpy(seg[1].copy()).cuda(), pd, w)
        rows = rx.results(ticket=t)
        ref = dm.model(seg, 0, 6, 2, lens, 0, w.cpu().numpy()[0])
        for s in range(2):
            assert np.array_equal(rx.soft(0, s, ticket=t), ref.soft[s]), (lens, s)
            assert (rows[s]["error_code"], rows[s]["crc32"], rows[s]["mpdu"]) == (ref.streams[s].error_code, ref.streams[s].crc32, ref.streams[s].psdu), (lens, s)
            assert (ref.streams[s].error_code, ref.streams[s].psdu) == (FRAME_OK, ps[s]), (lens, s)
        rx.close()
