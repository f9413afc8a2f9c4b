"""The seven stage entry points of the 802.11a receive graph's front end, the parts that need no GPU: declared in include/sora_hip.h, exported, bound and typed; each
refuses a null pointer by name and accepts a count of 0; the record sizes match the ctypes mirrors.  (This file fails without the feature: the names do not exist.)"""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SORA_OK, SORA_ERR_INVALID_PARAM, SORA_ERR_NO_DEVICE = 0, -1, -5
P = ctypes.c_void_p(4096)                                                        # a pointer that is not null and is never followed: every check below comes first

# name -> (arguments with every pointer set and counts of 1, the indices of the pointers, the index of the count)
STAGES = {
    "sora_hip_dc_remove11a":     ([P, P, P, P, P, P, 1, 1, None], (0, 1, 2, 3, 4, 5), 6),
    "sora_hip_dc_estimate11a":   ([P, P, P, P, 1, 1, None], (0, 1, 2, 3), 4),
    "sora_hip_cca11a":           ([P, P, P, P, P, P, P, P, 1, 1, 0, None], (0, 1, 2, 3, 4, 5, 6, 7), 8),
    "sora_hip_carrier_sense11a": ([P, P, P, P, P, 1, 1, 0, None], (0, 1, 2, 3, 4), 5),
    "sora_hip_data_symbol11a":   ([P, P, P, P, P, 1, 1, None], (0, 1, 2, 3, 4), 5),
    "sora_hip_viterbi_sig11a":   ([P, P, 1, None], (0, 1), 2),
    "sora_hip_plcp_parse11a":    ([P, P, 1, None], (0, 1), 2),
}


class Complex16(ctypes.Structure):
    _fields_ = [("re", ctypes.c_int16), ("im", ctypes.c_int16)]


class DcEst11aState(ctypes.Structure):
    _fields_ = [("update_cnt", ctypes.c_uint32), ("sum_dc", Complex16), ("dc", Complex16), ("reserved", ctypes.c_uint32)]


class Cca11aState(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint32) for n in ("cca_state", "error_code", "cca_pwr_threshold", "cca_pwr_reading", "cca_peak_index", "sync_state", "auto_count", "sense_count",
                                               "high_count")] + [("peak_corr", ctypes.c_int32), ("peak_index", ctypes.c_uint32), ("reserved0", ctypes.c_uint32),
               ("sample_his", Complex16 * 16), ("ac_re", ctypes.c_int32 * 4), ("ac_im", ctypes.c_int32 * 4), ("energy", ctypes.c_int32 * 4), ("ac_re_sum", ctypes.c_int32),
               ("ac_im_sum", ctypes.c_int32), ("energy_sum", ctypes.c_int32), ("reserved1", ctypes.c_uint32)]


class Cs11aState(ctypes.Structure):
    _fields_ = [("cca", Cca11aState), ("dc", DcEst11aState)]


@pytest.fixture(scope="module")
def lib():
    import sora_amd
    return sora_amd.load()


def test_the_seven_are_declared_exported_bound_and_typed(lib):
    from sora_amd import capi
    assert len(STAGES) == 7
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sora_hip.h")).read(), flags=re.S)
    for name, (args, _, _) in STAGES.items():
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in capi.EXPORTS and hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None and len(getattr(lib, name).argtypes) == len(args), name
    assert lib.sora_hip_abi_version() == 4
    assert "#define SORA_CCA11A_STOP_ON_TIMEOUT 1u" in header


def test_the_records_are_the_ctypes_mirrors_and_the_documented_words():
    from sora_amd import capi
    header = open(os.path.join(ROOT, "include", "sora_hip.h")).read()
    assert ctypes.sizeof(Cca11aState) == 4 * capi.CCA11A_WORDS == 176
    assert ctypes.sizeof(DcEst11aState) == 4 * capi.DCEST11A_WORDS == 16
    assert ctypes.sizeof(Cs11aState) == 4 * capi.CS11A_WORDS == 192
    for field, word in (("cca_pwr_threshold", 2), ("sync_state", 5), ("sense_count", 7), ("peak_corr", 9), ("sample_his", 12), ("ac_re", 28), ("energy", 36), ("ac_re_sum", 40)):
        assert getattr(Cca11aState, field).offset == 4 * word, field
    for struct in (Cca11aState, DcEst11aState):                                   # the header declares the same field names in the same order
        names = [n for n, _ in struct._fields_]
        tag = "sora_cca11a_state" if struct is Cca11aState else "sora_dcest11a_state"
        body = re.search(r"typedef struct \{([^}]*)\} %s;" % tag, header).group(1)
        found = [m for m in re.findall(r"\b([a-z_0-9]+)(?:\[\d+\])?\s*[,;]", body)]
        assert found == names, (tag, found)


def test_the_six_adapters_instantiate():
    """tests/cxx/rx11a_front_chain.cpp uses all six; it compiles against include/sora_brick.hpp without a GPU"""
    import subprocess
    src = os.path.join(ROOT, "tests", "cxx", "rx11a_front_chain.cpp")
    text = open(src).read()
    for name in ("THip11aDCRemoveEx", "THip11aDCEstimator", "THip11aCCA", "THip11aDataSymbol", "THip11aViterbiSig", "THip11aPLCPParser"):
        assert name + "<" in text or name + " " in text, name
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_python_surface():
    import sora_amd
    for name in ("dc_remove11a", "dc_estimate11a", "cca11a", "carrier_sense11a", "data_symbol11a", "viterbi_sig11a", "plcp_parse11a", "cca11a_states", "dcest11a_states",
                 "cs11a_states", "cca11a_reset", "cs11a_record_words", "rx11a_stages", "rx11a_by_stages"):
        assert callable(getattr(sora_amd, name)), name
    assert "not a fast path" in sora_amd.rx11a_by_stages.__doc__ and "44 MHz" in sora_amd.rx11a_by_stages.__doc__
    assert sora_amd.CCA11A_STOP_ON_TIMEOUT == 1 and sora_amd.CS11A_WORDS == 48


@pytest.mark.parametrize("name", sorted(STAGES))
def test_a_null_pointer_is_refused_by_name(lib, name):
    args, ptrs, _ = STAGES[name]
    for i in ptrs:
        a = list(args); a[i] = None
        assert getattr(lib, name)(*a) == SORA_ERR_INVALID_PARAM, (name, i)
        assert name.encode() in lib.sora_hip_last_error(), (name, i, lib.sora_hip_last_error())


@pytest.mark.parametrize("name", sorted(STAGES))
def test_a_count_of_zero_is_accepted_and_nothing_computes_without_a_device(lib, name):
    import sora_amd
    args, _, ncount = STAGES[name]
    a = list(args); a[ncount] = 0
    assert getattr(lib, name)(*a) == SORA_OK, name
    if sora_amd.device_count() <= 0:
        assert getattr(lib, name)(*args) == SORA_ERR_NO_DEVICE, name
        assert b"no HIP device" in lib.sora_hip_last_error()
