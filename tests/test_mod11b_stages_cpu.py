"""The seven stage entry points of the 802.11b modulation graph (include/sora_hip.h, sora_amd/csrc/k_mod11b.hip), the parts that need no GPU: declared, exported, bound
and typed; each refuses a null pointer by name and accepts a count of 0; the composition refuses what tx11b refuses; the six brick adapters and the C++ graph built from
them compile as a user's would.  (This file fails without the feature: the names do not exist.)"""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SORA_OK, SORA_ERR_INVALID_PARAM, SORA_ERR_NO_DEVICE = 0, -1, -5
P = ctypes.c_void_p(4096)                                                        # a pointer that is not null and is never followed: every check below comes first

# name -> (arguments with every pointer set and counts of 1, the indices of the pointers that must not be null, the index of the count)
STAGES = {
    "sora_hip_ppdu11b":         ([P, P, P, P, P, P, P, 1, None], (0, 1, 2, 3, 4, 5, 6), 7),
    "sora_hip_sc741_11b":       ([P, P, P, P, P, P, 1, 1, None], (0, 1, 2, 3, 4, 5), 6),
    "sora_hip_dbpsk_spread11b": ([P, P, P, P, P, P, 1, 1, None], (0, 1, 2, 3, 4, 5), 6),
    "sora_hip_dqpsk_spread11b": ([P, P, P, P, P, P, 1, 1, None], (0, 1, 2, 3, 4, 5), 6),
    "sora_hip_cck5_encode11b":  ([P, P, P, P, P, P, 1, 1, None], (0, 1, 2, 3, 4, 5), 6),
    "sora_hip_cck11_encode11b": ([P, P, P, P, P, P, 1, 1, None], (0, 1, 2, 3, 4, 5), 6),
    "sora_hip_pulse_shape11b":  ([P, P, P, P, P, P, P, 1, 1, None], (0, 1, 2, 3, 5, 6), 7),      # (d_flush, argument 4, may be null)
}
WRAPPERS = ("ppdu11b", "sc741_11b", "dbpsk_spread11b", "dqpsk_spread11b", "cck5_encode11b", "cck11_encode11b", "pulse_shape11b", "mod11b_by_stages")


@pytest.fixture(scope="module")
def lib():
    import sora_amd
    return sora_amd.load()


def test_the_seven_are_declared_exported_bound_and_typed(lib):
    from sora_amd import capi
    from sora_amd.build import SOURCES
    assert len(STAGES) == 7
    text = open(os.path.join(ROOT, "include", "sora_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, (args, _, _) in STAGES.items():
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in capi.EXPORTS and hasattr(lib, name), name
        f = getattr(lib, name)
        assert f.argtypes is not None and len(f.argtypes) == len(args) and f.argtypes[-1] is ctypes.c_void_p, name
    assert header.index("sora_hip_tx11b_pre(") < min(header.index(n + "(") for n in STAGES)          # a block of their own behind sora_hip_tx11b_pre
    assert re.search(r"typedef struct \{ uint32_t last_phase, is_even, reserved\[2\]; \} sora_mod11b_state;", header)
    assert "_pulse_shape11b" in text[text.index("Additive since"):text.index("#define SORA_HIP_ABI_VERSION")]
    assert lib.sora_hip_abi_version() == 4
    assert "k_mod11b.hip" in SOURCES


def test_python_surface():
    import sora_amd
    for name in WRAPPERS:
        assert callable(getattr(sora_amd, name)), name
    assert "not a fast path" in sora_amd.mod11b_by_stages.__doc__ and "demonstration" in sora_amd.mod11b_by_stages.__doc__


@pytest.mark.parametrize("name", sorted(STAGES))
def test_a_null_pointer_is_refused_by_name(lib, name):
    args, ptrs, _ = STAGES[name]
    for i in ptrs:
        a = list(args); a[i] = None
        assert getattr(lib, name)(*a) == SORA_ERR_INVALID_PARAM, (name, i)
        assert name.encode() in lib.sora_hip_last_error() and b"null pointer" in lib.sora_hip_last_error(), (name, i, lib.sora_hip_last_error())


@pytest.mark.parametrize("name", sorted(STAGES))
def test_a_count_of_zero_is_accepted_and_nothing_computes_without_a_device(lib, name):
    import sora_amd
    args, _, ncount = STAGES[name]
    a = list(args); a[ncount] = 0
    assert getattr(lib, name)(*a) == SORA_OK, name
    if sora_amd.device_count() <= 0:
        assert getattr(lib, name)(*args) == SORA_ERR_NO_DEVICE, name
        assert b"no HIP device" in lib.sora_hip_last_error()
        if name == "sora_hip_pulse_shape11b":                                    # with no flush table either
            a = list(args); a[4] = None
            assert getattr(lib, name)(*a) == SORA_ERR_NO_DEVICE


def test_by_stages_refuses_what_tx11b_refuses():
    import sora_amd
    cases = [([b"\x01\x02\x03"], [3000], None, None), ([b""], [1000], None, None), ([bytes(4093)], [11000], None, None), ([b"\x01", b"\x02"], [2000, 7], None, None),
             ([b"\x01"], [1000], None, 1), ([b"\x01"], [2000], None, 2), ([b"\x01", b"\x02"], [2000, 2000], None, [0]), ([b"\x01"], [2000], 4, None),
             ([b"\x01", b"\x02"], [2000, 2000], [0], None), ([b"\x01", b"\x02"], [2000], None, None)]
    for mpdus, rates, phase_in, preamble in cases:
        with pytest.raises(sora_amd.SoraError) as e:
            sora_amd.mod11b_by_stages(mpdus, rates, phase_in=phase_in, preamble=preamble)
        with pytest.raises(sora_amd.SoraError) as t:
            sora_amd.tx11b(mpdus, rates, phase_in=phase_in, preamble=preamble)
        assert e.value.code == t.value.code == SORA_ERR_INVALID_PARAM and str(e.value) == str(t.value), (rates, phase_in, preamble)


@pytest.mark.parametrize("what", ["sora_brick.hpp", "mod11b_chain.cpp"])
def test_adapters_and_the_cxx_graph_compile_clean(tmp_path, what):
    if what == "sora_brick.hpp":                                                 # (a header is checked as a user includes it)
        src = tmp_path / "include_brick.cpp"; src.write_text('#include "sora_brick.hpp"\n')
    else:
        src = os.path.join(ROOT, "tests", "cxx", "mod11b_chain.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_the_six_adapters_exist_and_instantiate(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "sora_brick.hpp")).read()
    for cls in ["THip11bSc741", "THip11bDBPSKSpread", "THip11bDQPSKSpread", "THip11bCCK5Encode", "THip11bCCK11Encode", "THip11bQuickPulseShaper"]:
        assert re.search(r"\b(class|struct|using) %s\b" % cls, hdr), cls
    src = tmp_path / "graph11b_mod.cpp"
    src.write_text("""
#include "sora_brick.hpp"
using namespace sora_brick;
int build_graph(uint8_t* d_bytes, sora_complex8* d_chips, sora_complex16* d_wide, void* d_tab, uint32_t* d_reg, sora_mod11b_state* d_ctx, sora_shaper11b_state* d_temps) {
    CF_Error ctx; TDrop<CF_Error> drop(ctx);
    uint8_t* t = static_cast<uint8_t*>(d_tab);
    THip11bQuickPulseShaper<88, CF_Error, TDrop<CF_Error>> s88(ctx, &drop, d_wide, t, d_temps);
    THip11bQuickPulseShaper<44, CF_Error, TDrop<CF_Error>> s44(ctx, &drop, d_wide, t + 16, d_temps);
    THip11bQuickPulseShaper<16, CF_Error, TDrop<CF_Error>> s16(ctx, &drop, d_wide, t + 32, d_temps);
    THip11bQuickPulseShaper<8, CF_Error, TDrop<CF_Error>> s8(ctx, &drop, d_wide, t + 48, d_temps);
    static_assert(decltype(s88)::oport_traits::burst == 4 * 88 && decltype(s8)::kFlushBursts == 1 && THip11bQuickPulseShaper<1, CF_Error, TDrop<CF_Error>>::kFlushBursts == 5, "1 -> 4");
    THip11bDBPSKSpread<1, CF_Error, decltype(s88)> dbpsk(ctx, &s88, d_chips, t + 64, d_ctx);
    THip11bDQPSKSpread<1, CF_Error, decltype(s44)> dqpsk(ctx, &s44, d_chips, t + 80, d_ctx);
    THip11bCCK5Encode<1, CF_Error, decltype(s16)> cck5(ctx, &s16, d_chips, t + 96, d_ctx);
    THip11bCCK11Encode<1, CF_Error, decltype(s8)> cck11(ctx, &s8, d_chips, t + 112, d_ctx);
    static_assert(decltype(dbpsk)::oport_traits::burst == 88 && decltype(dqpsk)::oport_traits::burst == 44 && decltype(cck5)::oport_traits::burst == 16 &&
                  decltype(cck11)::oport_traits::burst == 8 && decltype(dbpsk)::iport_traits::burst == 1, "the bricks' burst ratios");
    THip11bSc741<1, CF_Error, decltype(dbpsk)> sc(ctx, &dbpsk, d_bytes + 16, t + 128, d_reg, 0x1B);
    DevicePin<uint8_t, 1> src(d_bytes); src.append();
    bool ok = sc.Process(src);
    src.append(); ok = ok && dqpsk.Process(src); src.append(); ok = ok && cck5.Process(src); src.append(); ok = ok && cck11.Process(src);
    sc.SetSeed(0x6C); sc.Reset(); cck11.Reset(); sc.Flush(); cck11.Flush();
    return ok ? 0 : (int)ctx.error_code;
}
""")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
