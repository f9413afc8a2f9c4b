"""The 802.11a handle's soft stream as one pre-scaled byte per value (v << 1: sora_amd/csrc/rx_types.h) between the symbol chain
(k_frame, k_sym_back, k_pipe's back role) and every form of the trellis (k_viterbi, k_viterbi16, k_viterbi16w + k_win_redo, k_pipe's trellis role), against the
oracle's rows and MPDUs (oracle.pyoracle), never against the library itself.

What the format changed and what each test is after:
  * a trellis lane stores the byte it fetched into the high byte of its 16-bit operand slot and relies on the low byte being zero -- in the sixteen-lane layout the
    operand tables share their bytes with the trace-back's register dump, so they are cleared again behind every trace-back: frames of many windows, and frames that
    are noise behind an intact SIGNAL symbol (every metric byte in use, the window-parallel form decoding them a second time);
  * k_viterbi16's fast loop fetches without a clamp, so the lane of a frame that has ended reads on past its stream for as long as the longest frame of its wave
    runs: a 1-byte frame beside a 1500-byte one, and the same with the short frame in the LAST symbol slots of the handle (its fetches land in the pad behind the
    array -- an ordinary call, correct by construction);
  * sora_hip_viterbi11a* keeps the three-bit streams it packs into the caller's workspace (the *_p3 instantiations; tests/test_gpu_trellis_stage.py,
    test_gpu_ring_wrap.py and test_gpu_parity.py cover them), so the noise test runs on the handle path, and the workspace sizes are pinned as they were."""
import numpy as np
import pytest

from gpu_util import batch, make_capture, oracle_results, same_results
from oracle.pyoracle import RATES

gpu = pytest.mark.gpu
WINDOWED = 1
LENGTHS = (1, 2, 37, 100, 257, 1500)
_MADE = {}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def mixed_captures(o):
    """24 captures at 20 MHz, one frame each: every rate three times, with a very short, a middling and a 1500-byte MPDU.  The code-rate lists (1/2: 6, 12, 24 Mbps;
    3/4: 9, 18, 36, 54; 2/3: 48) hold 9, 12 and 3 frames, so every k_viterbi16 wave has frames of different modulations and of lengths 1 or 2 up to 1500, in
    whatever order k_scan queues them; neighbours in the call are as unlike as the set allows."""
    if "mixed" not in _MADE:
        keyed = []
        for i, rate in enumerate(RATES):
            for j, ln in enumerate((LENGTHS[i % 2], LENGTHS[2 + i % 3], 1500)):
                keyed.append((((i + j) % 3, i), make_capture(o, rate, ln, seed=7300 + 10 * i + j, rate_mhz=20, sigma=25 + 5 * (i % 4), tail=160)[0]))
        caps = [c for _, c in sorted(keyed, key=lambda t: t[0])]
        want = oracle_results(o, caps, 20)
        assert len(want) == 24 and all(r["error_code"] == 1 for r in want)
        assert {r["rate_kbps"] for r in want} == set(RATES) and {r["length"] - 4 for r in want} == set(LENGTHS)
        _MADE["mixed"] = (caps, want)
    return _MADE["mixed"]


def noise_captures(o):
    """one frame per code rate (24, 48, 54 Mbps), 1200-odd bytes -- dozens of windows -- whose SIGNAL symbol is intact and whose data field is noise"""
    if "noise" not in _MADE:
        rng = np.random.default_rng(913)
        caps = []
        for i, rate in enumerate((24000, 48000, 54000)):
            cap = make_capture(o, rate, 1200 + 37 * i, seed=940 + i, rate_mhz=20, sigma=30, tail=160)[0].astype(np.int32)
            d0 = 320 + 80                                                          # preamble + SIGNAL at 20 MHz
            cap[d0:len(cap) - 160] = np.rint(rng.normal(0, 2500, (len(cap) - 160 - d0, 2)))
            caps.append(np.clip(cap, -32768, 32767).astype(np.int16))
        want = oracle_results(o, caps, 20)
        assert len(want) == 3 and all(r["error_code"] != 1 for r in want)
        _MADE["noise"] = (caps, want)
    return _MADE["noise"]


def last_slot_captures(o):
    """four frames of the 3/4 list -- one k_viterbi16 wave -- the 1500-byte one first and, LAST in the buffer, a two-symbol frame that ends on the buffer's last
    sample: its stream sits in the last symbol slots the call has, and its lane reads 200-odd symbols past it"""
    if "last" not in _MADE:
        def ending_with_its_frame(rate, length):
            mp = np.random.default_rng(length).integers(0, 256, length).astype(np.uint8).tobytes()
            x = o.tx_capture(mp, rate, seed=1 + length % 127, lead=0, tail=0)
            lead20 = (-(len(x) // 2)) % 14 + 28
            return np.concatenate([np.zeros((2 * lead20, 2), np.int16), x])[::2].copy()
        caps = [make_capture(o, 36000, 1500, seed=7501, rate_mhz=20, sigma=30, tail=160)[0], make_capture(o, 9000, 100, seed=7502, rate_mhz=20, sigma=30, tail=160)[0],
                make_capture(o, 18000, 257, seed=7503, rate_mhz=20, sigma=30, tail=160)[0], ending_with_its_frame(54000, 30)]
        want = oracle_results(o, caps, 20)
        assert [r["length"] for r in want] == [1504, 104, 261, 34] and all(r["error_code"] == 1 for r in want)
        assert want[3]["end_sample"] == len(caps[3]) and want[3]["nsym"] == 2
        _MADE["last"] = (caps, want)
    return _MADE["last"]


def run(torch, caps, trellis=None, front=None, exact=False):
    import sora_amd
    iq, descs = batch(caps)
    if exact:
        iq = iq[:descs[-1][0] + descs[-1][1]]                                      # the last capture's last sample is the buffer's last
    rx = sora_amd.Rx(max_captures=len(caps), max_total_samples=len(iq), sample_rate_mhz=20, max_frames_per_capture=2)
    if trellis is not None:
        rx.set_trellis(trellis); assert rx.trellis() == trellis
    if front is not None:
        rx.set_front(front)
    rx.process_dev(torch.from_numpy(iq).cuda(), descs)
    got = rx.results()
    rx.process_dev(torch.from_numpy(iq).cuda(), descs)                            # ... and once more over the streams the first call left behind
    again = rx.results()
    st = rx.window_stats() if trellis == WINDOWED else None
    rx.close()
    return got, again, st


@gpu
@pytest.mark.parametrize("trellis,front", [(64, None), (16, None), (WINDOWED, None), (16, 1), (16, 3), (WINDOWED, 3), (WINDOWED, 4)])
def test_every_rate_and_unlike_lengths_in_one_wave(oracle, torch_cuda, trellis, front):
    caps, want = mixed_captures(oracle)
    got, again, st = run(torch_cuda, caps, trellis, front)
    for g in (got, again):
        ok, why = same_results(g, want)
        assert ok, (trellis, front, why)
    if st is not None:
        assert st["boundaries_failed"] == 0 and st["frames_decoded_again"] == 0, st


@gpu
@pytest.mark.parametrize("trellis", [16, 64, WINDOWED])
def test_short_frame_in_the_last_slots(oracle, torch_cuda, trellis):
    caps, want = last_slot_captures(oracle)
    got, again, _ = run(torch_cuda, caps, trellis, None, exact=True)
    for g in (got, again):
        ok, why = same_results(g, want)
        assert ok, (trellis, why)


@gpu
@pytest.mark.parametrize("trellis", [16, 64, WINDOWED])
def test_noise_behind_a_good_header(oracle, torch_cuda, trellis):
    """(in place of a noise stream through sora_hip_viterbi11a, which keeps its three-bit path)"""
    caps, want = noise_captures(oracle)
    for group, w in ((caps, want), (caps[2:], [dict(want[2], capture_id=0)])):
        got, again, st = run(torch_cuda, group, trellis)
        for g in (got, again):
            ok, why = same_results(g, w)
            assert ok, (trellis, len(group), why)
        if st is not None:
            assert st["boundaries_failed"] > 0 and st["frames_decoded_again"] > 0, st


def test_stage_workspace_sizes_are_what_they_were():
    """sora_hip_viterbi11a_workspace_bytes / 11n: the contract of the caller-owned workspace, pinned to the values of the commit before the byte-wide stream"""
    import sora_amd
    sizes = ((24, 1), (48, 1), (1001, 3), (65568, 1), (192000, 8), (1 << 20, 300), (50000000, 4096), (123456789, 20000))
    assert [sora_amd.viterbi11a_workspace_bytes(s, n) for s, n in sizes] == [23552, 23552, 65536, 56320, 264704, 4807680, 30376448, 72610816]
    assert [sora_amd.viterbi11n_workspace_bytes(s, n) for s, n in sizes] == [23552, 23552, 66048, 89088, 360704, 5331968, 55376384, 134339328]
