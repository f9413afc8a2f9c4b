"""The 40 MHz HT data field on the GPU (k_ht40_frame and what follows it) held BIT FOR BIT to the integer model oracle/ht40_data_model.py, from the detection
weights on: every de-interleaved soft byte of both streams (sora_ht40_soft_of), every row field (error_code, length, crc32) and every PSDU byte, of frames that
pass and of frames that FAIL their FCS.  No tolerance, no frame, carrier or byte left out.  The model's weight input is the GPU's exported d_weights (their own
arithmetic is held in tests/test_gpu_ht40.py: +-1 LSB in MMSE mode, bit for bit in zero-forcing mode -- which is extended here to adversarial input); the model
itself is held to the independent numpy model of the format in tests/test_ht40_data_model.py.  All calls are descriptor calls (sora_ht40_process_dev).

What the existing loop-back tests cannot see and these do: a pilot read from the wrong carrier, a tracker with another gain or one stream's pilots only, theta
wrapping wrongly at +-32768, a saturation at the wrong place, a frequency-compensation index that is off -- each changes soft bytes long before it loses a frame."""
import numpy as np
import pytest

from oracle import ht40_data_model as dm
from oracle import py_ht40 as m
from ht40_soft_check import assert_is_the_model, models, soft_capacity

pytestmark = pytest.mark.gpu

H0 = np.array([[1.0 * np.exp(0.3j), 0.35 * np.exp(-1.1j)], [0.3 * np.exp(2.0j), 0.9 * np.exp(-0.4j)]])


@pytest.fixture(scope="module")
def env():
    import torch
    import sora_amd
    if sora_amd.device_count() <= 0:
        pytest.skip("no HIP device")
    return torch, sora_amd


# ------------------------------------------------------------------ inputs
def lengths_for(nb, cr, nsym, longer, rng):
    """two different PSDU lengths (>= 4) whose LONGER one, in stream `longer`, needs exactly nsym symbols"""
    nd = m.ndbps(nb, cr)
    top = (nsym * nd - 22) // 8
    low = max(4, ((nsym - 1) * nd - 22) // 8 + 1)
    assert top >= 5 and top >= low, (nb, cr, nsym)
    big = int(rng.integers(max(low, 5), top + 1)); small = int(rng.integers(4, big))
    lens = (small, big) if longer else (big, small)
    assert m.nsym_for(list(lens), nb, cr) == nsym and lens[0] != lens[1]
    return lens


def real_frame(rng, nb, cr, lens, sigma, cfo_step=0.0):
    """a py_ht40 frame through the 2x2 channel -> int16 [2, (2 + nsym) * 160, 2], psdus"""
    ps = [m.add_fcs(rng.integers(0, 256, ln - 4, dtype=np.uint8).tobytes()) for ln in lens]
    x, nsym = m.tx(ps, nb, cr, seeds=(int(rng.integers(1, 128)), int(rng.integers(1, 128))))
    return m.channel(x, H0, sigma, rng, cfo_step=cfo_step), ps


def place(segments, mods=None):
    """segments: [int16 [2, n, 2]] -> (iq [2, N, 2], offsets).  mods[i] (optional): the residue mod 64 frame i's offset must have; zeros fill the gaps; nothing
    follows the last frame: it ends on the buffer's last sample."""
    parts, offs, pos = [], [], 0
    for i, seg in enumerate(segments):
        gap = 0 if mods is None else (mods[i] - pos) % 64
        if gap:
            parts.append(np.zeros((2, gap, 2), np.int16)); pos += gap
        offs.append(pos); parts.append(seg); pos += seg.shape[1]
    return np.concatenate(parts, axis=1), offs


# ------------------------------------------------------------------ one call, read back whole
def gpu_call(env, iq, descs, want_w=True, trellis=None):
    """-> dict: rows (results), soft[frame][stream], w int16 [nframes, 4, 128, 2] or None"""
    torch, sora = env
    rx = sora.RxHt40(len(descs), soft_capacity(sora, descs))
    if trellis is not None:
        rx.set_trellis(trellis)
    w = torch.zeros((len(descs), 4, 128, 2), dtype=torch.int16, device="cuda") if want_w else None
    t = rx.process_dev(torch.from_numpy(iq[0].copy()).cuda(), torch.from_numpy(iq[1].copy()).cuda(), descs, w)
    rows = rx.results(ticket=t)
    soft = [[rx.soft(f, s, ticket=t) for s in range(2)] for f in range(len(descs))]
    rx.close()
    return {"rows": rows, "soft": soft, "w": w.cpu().numpy() if want_w else None}


def saturated_symbols(want):
    """components of detected symbols at the rails of TMimoChannelComp's saturating pack, over the 114 occupied carriers"""
    return sum(int(np.sum((r.xs[:, :, dm.OCCUPIED_BINS] == 32767) | (r.xs[:, :, dm.OCCUPIED_BINS] == -32768))) for r in want)


# ------------------------------------------------------------------ the shape grid
GRID_RATES = {1: (2, 0, 2, 0), 2: (0, 2, 0, 2), 4: (2, 0, 2, 0), 6: (1, 2, 1, 2)}        # code rate per (n_bpsc, grid column)


@pytest.fixture(scope="module")
def grid():
    """n_bpsc 1, 2, 4, 6 x nsym 1, 2, 3, 12, the two streams' lengths different, the longer one alternating between the streams; ordered so that every workgroup
    of four frames holds all four n_bpsc.  -> [(segment, descriptor tail (nb, cr, l0, l1), psdus)]"""
    rng = np.random.default_rng(4001)
    out = []
    for col, nsym in enumerate((1, 2, 3, 12)):
        for nb in (1, 2, 4, 6):
            cr = GRID_RATES[nb][col]
            lens = lengths_for(nb, cr, nsym, (col + nb) & 1, rng)
            seg, ps = real_frame(rng, nb, cr, lens, 6.0)
            out.append((seg, (nb, cr, lens[0], lens[1]), ps))
    per = {(nb, (seg.shape[1] // 160 - 2)): (seg.shape[1] // 160 - 2) * 108 * nb for seg, (nb, _, _, _), _ in out}
    assert per[(4, 2)] % 32 == 0 and per[(1, 1)] == 108 and per[(1, 1)] % 32 != 0      # stream 1 behind a count that is a multiple of 32, and behind one that is padded (108 -> 128)
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
        assert [want[f].streams[s].psdu for s in range(2)] == g[2], f


@pytest.mark.parametrize("nframes", [1, 3, 4, 5])
def test_batch_layouts_partial_full_and_one_more_than_a_workgroup(env, grid, nframes):
    pick = [grid[(5 * i + nframes) % 16] for i in range(nframes)]
    iq, offs = place([g[0] for g in pick])
    descs = describe(pick, offs)
    got = gpu_call(env, iq, descs)
    assert_is_the_model(got, models(iq, descs, got["w"]), descs, "batch of %d" % nframes)


def test_frame_offsets_off_every_alignment_and_the_last_frame_ends_the_buffer(env, grid):
    mods = [0, 1, 2, 3, 5, 63, 65 % 64]
    pick = [grid[i] for i in (12, 1, 6, 11, 0, 13, 10)]
    iq, offs = place([g[0] for g in pick], mods)
    offs65 = offs[6]
    assert [o % 64 for o in offs] == mods and offs[0] == 0 and offs65 >= 65 and any(o % 4 for o in offs)
    assert offs[-1] + pick[-1][0].shape[1] == iq.shape[1]                  # the kernel reads up to, and not past, the last sample
    descs = describe(pick, offs)
    got = gpu_call(env, iq, descs)
    assert_is_the_model(got, models(iq, descs, got["w"]), descs, "offsets")
    for lead in (1, 2, 3, 5, 63, 65):                                      # ... and the same offsets taken literally: one short frame behind `lead` samples
        iq, offs = place([np.zeros((2, lead, 2), np.int16), grid[0][0]])
        descs = describe([grid[0]], offs[1:])
        assert descs[0][0] == lead and lead + grid[0][0].shape[1] == iq.shape[1]
        got = gpu_call(env, iq, descs)
        assert_is_the_model(got, models(iq, descs, got["w"]), descs, "offset %d" % lead)


# ------------------------------------------------------------------ real frames: noise, carrier offsets, both detectors
def test_real_frames_that_pass_and_that_fail_cfo_and_both_detectors(env):
    rng = np.random.default_rng(4002)
    segs, tails, nvs, cfos = [], [], [], []
    for cfo in (0, 37, -511, 4096):
        for sigma, nv in ((6.0, 0.0), (6.0, 3000.0), (150.0, 0.0), (150.0, 3000.0)):
            lo, hi = (60, 200) if sigma < 100 else (150, 300)
            lens = (int(rng.integers(lo, hi)), int(rng.integers(lo, hi)))
            seg, _ = real_frame(rng, 6, 2, lens, sigma, cfo_step=-float(cfo))
            segs.append(seg); tails.append((6, 2) + lens); nvs.append(nv); cfos.append(cfo)
    # the mistuned descriptor of tests/test_ht40_data_model.py: sent with cfo_step 37, described as 0 -- theta ramps by 5920 a symbol and wraps inside 12 symbols
    seg, ps_mistuned = real_frame(rng, 1, 0, (75, 60), 2.0, cfo_step=37.0)
    for nv in (0.0, 3000.0):
        segs.append(seg); tails.append((1, 0, 75, 60)); nvs.append(nv); cfos.append(0)
    iq, offs = place(segs, [int(v) for v in rng.integers(0, 64, len(segs))])
    descs = [(offs[i],) + tails[i] + (cfos[i], nvs[i], i) for i in range(len(segs))]
    got = gpu_call(env, iq, descs)
    want = models(iq, descs, got["w"])
    assert_is_the_model(got, want, descs, "real frames")
    codes = [r["error_code"] for r in got["rows"]]
    loud = [c for f in range(16) if f % 4 >= 2 for c in codes[2 * f:2 * f + 2]]
    assert all(c == 1 for f in range(16) if f % 4 < 2 for c in codes[2 * f:2 * f + 2]), [hex(c) for c in codes]
    assert loud.count(0x80000006) >= 4, [hex(c) for c in loud]             # 64-QAM 3/4 at sigma 150 fails: rows and bytes of FAILED frames were compared too
    for f in (16, 17):
        th = want[f].theta.astype(int)
        assert np.any(np.diff(th) < -30000) and th.max() > 26000 and th.min() < -26000, th           # theta wrapped
        assert [r["mpdu"] for r in got["rows"][2 * f:2 * f + 2]] == ps_mistuned, f


# ------------------------------------------------------------------ no frame at all: the saturating paths
def adversarial_inputs():
    """-> [(name, int16 [2, 800, 2])]: 800 samples hold the two HT-LTF symbols and three data symbols of a described frame that is not there"""
    rng = np.random.default_rng(4003)
    out = []
    for amp in (30, 400, 3000, 32767):
        out.append(("uniform %d" % amp, rng.integers(-amp, amp + 1, (2, 800, 2)).astype(np.int16)))
    out.append(("rails", np.where(rng.integers(0, 2, (2, 800, 2)) == 1, 32767, -32768).astype(np.int16)))
    out.append(("all +32767", np.full((2, 800, 2), 32767, np.int16)))
    out.append(("all -32768", np.full((2, 800, 2), -32768, np.int16)))
    # quiet HT-LTF symbols (the weights saturate) in front of full-scale data symbols: the products reach the 32-bit sum's and the >> 9 pack's rails with every
    # value in between, not only with the constants of the two inputs above
    for name, data in (("quiet LTF, full-scale noise", out[3][1]), ("quiet LTF, rails", out[4][1])):
        x = out[0][1].copy(); x[:, 320:] = data[:, 320:]
        out.append((name, x))
    return out


def test_adversarial_input_saturating_paths_both_detectors_and_the_zero_forcing_weights(env):
    """Both chains noise, rails or a constant, HT-LTF symbols included: the channel matrix is ill-conditioned, the weights saturate, so do the detected symbols.
    Plus one frame whose chain 1 equals chain 0 (a singular channel matrix on every carrier).  In zero-forcing mode the GPU's weights on the 114 occupied carriers
    must be TMimoChannelEst's arithmetic in the model, bit for bit (test_zero_forcing_weights_are_the_reference_bricks on three benign frames, extended to these levels)."""
    inputs = adversarial_inputs()
    rng = np.random.default_rng(4004)
    singular = inputs[2][1].copy(); singular[1] = singular[0]
    segs, descs_tail = [], []
    for i, (name, seg) in enumerate(inputs):
        for nv in (0.0, 3000.0):
            nb = (1, 2, 4, 6)[(i + (nv > 0)) % 4]; cr = (0, 2, 0, 1)[(i + (nv > 0)) % 4]
            lens = lengths_for(nb, cr, 3, i & 1, rng)
            segs.append(seg); descs_tail.append((nb, cr) + lens + (int(rng.choice([0, 37, -511, 4096])), nv))
    segs.append(singular); descs_tail.append((4, 0) + lengths_for(4, 0, 3, 0, rng) + (0, 0.0))
    iq, offs = place(segs, [int(v) for v in rng.integers(0, 64, len(segs))])
    descs = [(offs[i],) + descs_tail[i] + (i,) for i in range(len(segs))]
    got = gpu_call(env, iq, descs)
    want = models(iq, descs, got["w"])
    assert_is_the_model(got, want, descs, "adversarial")
    occ = dm.OCCUPIED_BINS
    zf_sat = 0
    for f, d in enumerate(descs):
        if d[6] == 0.0:
            own = dm.zf_weights(iq, d[0], d[5])
            assert np.array_equal(got["w"][f][:, occ], own[:, occ]), ("zero-forcing weights", f, d[1:6])
            zf_sat += int(np.sum((own[:, occ] == 32767) | (own[:, occ] == -32768)))
    # the saturating paths were really reached, under both detectors: detected symbols at the rails of the >> 9 pack, weights at the rails of their own pack
    for zf in (True, False):
        fr = [f for f, d in enumerate(descs) if (d[6] == 0.0) == zf]
        xsat = saturated_symbols([want[f] for f in fr])
        wsat = int(np.sum((got["w"][fr][:, :, occ] == 32767) | (got["w"][fr][:, :, occ] == -32768)))
        assert xsat > 0 and wsat > 0, ("zero forcing" if zf else "MMSE", xsat, wsat)
    assert zf_sat > 0
    sing = got["w"][len(segs) - 1][:, occ]
    assert np.all((sing == 32767) | (sing == -32768) | (sing == 0)), "a singular channel matrix has no finite inverse"


# ------------------------------------------------------------------ variants of the same call
def test_without_weight_export_and_with_either_trellis_nothing_changes(env, grid):
    rng = np.random.default_rng(4005)
    pick = [grid[i] for i in (15, 2, 9, 4, 14)]
    seg, _ = real_frame(rng, 6, 2, (150, 90), 150.0)                      # ... and a frame too noisy to decode
    pick.append((seg, (6, 2, 150, 90), None))
    iq, offs = place([g[0] for g in pick], [int(v) for v in rng.integers(0, 64, len(pick))])
    descs = describe(pick, offs)
    base = gpu_call(env, iq, descs)
    want = models(iq, descs, base["w"])
    assert_is_the_model(base, want, descs, "with d_weights")
    assert any(r["error_code"] == 0x80000006 for r in base["rows"])
    for trellis, want_w in ((None, False), (16, False), (64, False), (64, True)):
        assert_is_the_model(gpu_call(env, iq, descs, want_w=want_w, trellis=trellis), want, descs, "trellis %s, d_weights %s" % (trellis, want_w))


def test_soft_of_belongs_to_its_ticket_and_refuses_what_it_cannot_answer(env, grid):
    """Nine calls over the handle's eight slots: the soft bytes of the OLDEST call still in flight, read while newer ones run, are its own; a ticket whose slot was
    reused, a raw-capture call, a frame or stream that is not there and a buffer that is too small are refused."""
    import ctypes
    torch, sora = env
    batches = []
    for b in range(3):
        pick = [grid[(3 * b + 5 * i) % 16] for i in range(3 + b)]
        iq, offs = place([g[0] for g in pick])
        descs = describe(pick, offs)
        want = models(iq, descs, gpu_call(env, iq, descs)["w"])
        batches.append((torch.from_numpy(iq[0].copy()).cuda(), torch.from_numpy(iq[1].copy()).cuda(), descs, want))
    rx = sora.RxHt40(8, max(soft_capacity(sora, b[2]) for b in batches))
    depth = rx.calls_in_flight()
    assert depth == 8

    def check(t, b):
        f0, f1, descs, want = batches[b]
        for f in range(len(descs)):
            for s in range(2):
                assert np.array_equal(rx.soft(f, s, ticket=t), want[f].soft[s]), (t, b, f, s)

    tickets = [(rx.process_dev(batches[k % 3][0], batches[k % 3][1], batches[k % 3][2]), k % 3) for k in range(9)]
    check(*tickets[1])                                                     # the oldest call still addressable, while the newer ones run
    for t, b in tickets[2:]:
        check(t, b)
    assert np.array_equal(rx.soft(0, 1), batches[tickets[-1][1]][3][0].soft[1])         # ticket None: the most recent call
    with pytest.raises(sora.SoraError) as e:
        rx.soft(0, 0, ticket=tickets[0][0])                                # its slot was reused by the ninth call
    assert e.value.code == -1 and "stale ticket" in str(e.value)
    t, b = tickets[-1]
    n = len(batches[b][2])
    for frame, stream in ((n, 0), (0, 2), (2 ** 32 - 1, 0)):
        with pytest.raises(sora.SoraError) as e:
            rx.soft(frame, stream, ticket=t)
        assert e.value.code == -1
    L = sora.load(); buf = np.zeros(16, np.uint8); ns = ctypes.c_size_t(0)
    assert L.sora_ht40_soft_of(rx._h, t, 0, 0, buf.ctypes.data, buf.size, ctypes.byref(ns)) == -6          # SORA_ERR_CAPACITY: the count is reported, nothing is copied
    assert ns.value == len(batches[b][3][0].soft[0]) and not buf.any()
    # a raw-capture call plans its frames on the device: refused
    noise = torch.from_numpy(np.random.default_rng(1).integers(-30, 31, (2800, 2)).astype(np.int16)).cuda()
    tc = rx.process_captures_dev(noise, noise, [(0, 2800, 7)], max_frames_per_capture=1)
    with pytest.raises(sora.SoraError) as e:
        rx.soft(0, 0, ticket=tc)
    assert e.value.code == -1 and "descriptor calls" in str(e.value)
    rx.synchronize(); rx.close()
