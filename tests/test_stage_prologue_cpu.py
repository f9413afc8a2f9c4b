"""The shared prologue of the stage entry points (sora_amd/csrc/host_stage.h) on the 802.11a symbol chain and the older 802.11n stages, the parts that need no GPU:
each refuses a null pointer by name, accepts a count of 0, computes nothing without a device and refuses a count of 2^31 (SORA_ERR_CAPACITY: the device check comes
first, so without a device that call reports the missing device).  The newer stage blocks assert the same in their own files (tests/test_11b_stages_cpu.py and its kin)."""
import ctypes

import pytest

SORA_OK, SORA_ERR_INVALID_PARAM, SORA_ERR_NO_DEVICE, SORA_ERR_CAPACITY = 0, -1, -5, -6
P = ctypes.c_void_p(4096)                                                        # a 16-byte-aligned pointer that is not null and is never followed: every check below comes first

# name -> (arguments with every pointer set and counts of 1, the indices of the pointers that must not be null, the index of the count); a tuple among the indices:
# pointers of which one must be set
STAGES = {
    "sora_hip_fft64":            ([P, P, 1, None], (0, 1), 2),
    "sora_hip_fft128":           ([P, P, 1, None], (0, 1), 2),
    "sora_hip_lts11a":           ([P, P, 1, None], (0, 1), 2),
    "sora_hip_symfront11a":      ([P, P, P, P, 1, None], (0, 1, 3), 4),
    "sora_hip_freq_comp11a":     ([P, P, P, P, 1, None], (0, 1, 3), 4),
    "sora_hip_equalize11a":      ([P, P, P, P, 1, None], (0, 1, 3), 4),
    "sora_hip_phase_comp11a":    ([P, P, P, P, 1, None], (0, 1, 3), 4),
    "sora_hip_pilot_track11a":   ([P, P, P, P, P, 1, None], (0, 1, 2, 3, 4), 5),
    "sora_hip_pilot11a":         ([P, P, P, P, P, 1, None], (0, 1, 2, 3, 4), 5),
    "sora_hip_demap11a":         ([P, P, 1, 1, None], (0, 1), 3),
    "sora_hip_deinterleave11a":  ([P, P, 1, 1, None], (0, 1), 3),
    "sora_hip_demap11n":         ([P, P, 1, 1, None], (0, 1), 3),
    "sora_hip_deinterleave11n":  ([P, P, 1, 0, 1, None], (0, 1), 4),
    "sora_hip_cfo_est11n":       ([P, P, P, 1, None], (0, 1, 2), 3),
    "sora_hip_freq_comp11n":     ([P, P, P, P, P, P, P, 1, 1, None], (0, 1, 2, 3, 4, 5, 6), 7),
    "sora_hip_pilot_track11n":   ([P, P, P, P, P, P, 1, None], (0, 1, 2, 3, 4), 6),
    "sora_hip_mimo_est11n":      ([P, P, P, P, 1, None], (0, 1, 2, 3), 4),
    "sora_hip_mimo_comp11n":     ([P, P, P, P, P, P, 1, None], (0, 2, 3, 4, 5), 6),
    "sora_hip_siso_est11n":      ([P, P, P, 1, None], (0, 1, 2), 3),
    "sora_hip_siso_comp11n":     ([P, P, P, P, P, P, P, 1, None], (0, 2, 3, (4, 5, 6)), 7),
    "sora_hip_sig_demap11n":     ([P, P, 1, None], (0, 1), 2),
    "sora_hip_sig_decode11n":    ([P, P, 1, None], (0, 1), 2),
}


@pytest.fixture(scope="module")
def lib():
    import sora_amd
    return sora_amd.load()


def test_the_entries_are_bound_and_typed(lib):
    assert len(STAGES) == 22
    for name, (args, _, _) in STAGES.items():
        assert getattr(lib, name).argtypes is not None and len(getattr(lib, name).argtypes) == len(args), name


@pytest.mark.parametrize("name", sorted(STAGES))
def test_a_null_pointer_is_refused_by_name(lib, name):
    args, ptrs, _ = STAGES[name]
    for i in ptrs:
        a = list(args)
        for k in (i if isinstance(i, tuple) else (i,)):
            a[k] = None
        assert getattr(lib, name)(*a) == SORA_ERR_INVALID_PARAM, (name, i)
        msg = lib.sora_hip_last_error()
        assert name.encode() in msg and b"null pointer" in msg, (name, i, msg)


@pytest.mark.parametrize("name", sorted(STAGES))
def test_a_count_of_zero_is_accepted_and_nothing_computes_without_a_device(lib, name):
    import sora_amd
    args, _, ncount = STAGES[name]
    a = list(args); a[ncount] = 0
    assert getattr(lib, name)(*a) == SORA_OK, name
    if sora_amd.device_count() <= 0:                                             # (with a device these addresses would be launched on)
        assert getattr(lib, name)(*args) == SORA_ERR_NO_DEVICE, name
        assert b"no HIP device" in lib.sora_hip_last_error()


@pytest.mark.parametrize("name", sorted(STAGES))
def test_a_count_of_two_to_the_31_is_refused(lib, name):
    import sora_amd
    args, _, ncount = STAGES[name]
    a = list(args); a[ncount] = 1 << 31
    if sora_amd.device_count() <= 0:                                             # the device check precedes the capacity check
        assert getattr(lib, name)(*a) == SORA_ERR_NO_DEVICE, name
        return
    assert getattr(lib, name)(*a) == SORA_ERR_CAPACITY, name                     # (refused in the prologue: nothing is launched on these addresses)
    msg = lib.sora_hip_last_error()
    assert name.encode() in msg and b"too many for one call" in msg, (name, msg)
