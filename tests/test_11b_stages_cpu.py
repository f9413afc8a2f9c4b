"""The thirteen 802.11b stage entry points, the parts that need no GPU: declared in include/sora_hip.h, exported, bound and typed; each refuses a null pointer by name
and accepts a count of 0; the seven brick adapters instantiate into a graph.  (This file fails without the feature: the names do not exist.)"""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SORA_OK, SORA_ERR_INVALID_PARAM, SORA_ERR_NO_DEVICE = 0, -1, -5
P = ctypes.c_void_p(4096)                                                        # a pointer that is not null and is never followed: every check below comes first

# name -> (arguments with every pointer set and counts of 1, the indices of the pointers, the index of nstreams)
STAGES = {
    "sora_hip_dc_remove11b":      ([P, P, P, P, P, P, 1, 1, None], (0, 1, 2, 3, 4, 5), 6),
    "sora_hip_energy_detect11b":  ([P, P, P, P, P, 1, 1, None], (0, 1, 2, 3, 4), 5),
    "sora_hip_symtiming11b":      ([P, P, P, P, P, P, P, 1, 1, None], (0, 1, 2, 3, 4, 5, 6), 7),
    "sora_hip_barker_sync11b":    ([P, P, P, P, P, 1, 1, None], (0, 1, 2, 3, 4), 5),
    "sora_hip_despread11b":       ([P, P, P, P, P, 1, 1, None], (0, 1, 2, 3, 4), 5),
    "sora_hip_sfd_sync11b":       ([P, P, P, P, P, 1, 1, 0, None], (0, 1, 2, 3, 4), 5),
    "sora_hip_dbpsk_demap11b":    ([P, P, P, P, P, P, 1, 1, None], (0, 1, 2, 3, 4, 5), 6),
    "sora_hip_dqpsk_demap11b":    ([P, P, P, P, P, P, 1, 1, None], (0, 1, 2, 3, 4, 5), 6),
    "sora_hip_cck5p5_decode11b":  ([P, P, P, P, P, P, 1, 1, None], (0, 1, 2, 3, 4, 5), 6),
    "sora_hip_cck11_decode11b":   ([P, P, P, P, P, P, 1, 1, None], (0, 1, 2, 3, 4, 5), 6),
    "sora_hip_desc741_11b":       ([P, P, P, P, P, P, 1, 1, None], (0, 1, 2, 3, 4, 5), 6),
    "sora_hip_plcp_parse11b":     ([P, P, 1, None], (0, 1), 2),
    "sora_hip_frame_sink11b":     ([P, P, P, P, 1, None], (0, 1, 2, 3), 4),
}


@pytest.fixture(scope="module")
def lib():
    import sora_amd
    return sora_amd.load()


def test_the_thirteen_are_declared_exported_bound_and_typed(lib):
    from sora_amd import capi
    assert len(STAGES) == 13
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sora_hip.h")).read(), flags=re.S)
    for name, (args, _, _) in STAGES.items():
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in capi.EXPORTS and hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None and len(getattr(lib, name).argtypes) == len(args), name
    assert lib.sora_hip_abi_version() == 4


def test_python_surface():
    import sora_amd
    for name in ("dc_remove11b", "energy_detect11b", "symtiming11b", "barker_sync11b", "despread11b", "sfd_sync11b", "dbpsk_demap11b", "dqpsk_demap11b", "cck5p5_decode11b",
                 "cck11_decode11b", "desc741_11b", "plcp_parse11b", "frame_sink11b", "rx11b_by_stages"):
        assert callable(getattr(sora_amd, name)), name
    assert "not a fast path" in sora_amd.rx11b_by_stages.__doc__


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


def test_the_seven_adapters_instantiate(tmp_path):
    src = tmp_path / "graph11b.cpp"
    src.write_text("""
#include "sora_brick.hpp"
using namespace sora_brick;
int build_graph(sora_complex16* d_chips, sora_complex16* d_sym, uint8_t* d_raw, uint8_t* d_out, void* d_tab, sora_stream11b_state* d_ctx) {
    CF_Error ctx; TDrop<CF_Error> drop(ctx);
    uint8_t* t = static_cast<uint8_t*>(d_tab);
    THip11bDesc741<6, CF_Error, TDrop<CF_Error>> desc(ctx, &drop, d_out, t, d_ctx);
    THip11bDBPSKDemap<6, CF_Error, decltype(desc)> dbpsk(ctx, &desc, d_raw, t + 16, d_ctx);
    THip11bDQPSKDemap<6, CF_Error, decltype(desc)> dqpsk(ctx, &desc, d_raw, t + 32, d_ctx);
    THip11bDespread<48, CF_Error, decltype(dbpsk)> despread(ctx, &dbpsk, d_sym, t + 48);
    THip11bCCK5P5Decoder<4, CF_Error, decltype(desc)> cck5(ctx, &desc, d_raw, t + 64, d_ctx);
    THip11bCCK11Decoder<4, CF_Error, decltype(desc)> cck11(ctx, &desc, d_raw, t + 80, d_ctx);
    THip11bDCRemove<7, CF_Error, TDrop<CF_Error>> dc(ctx, &drop, d_sym, t + 96);
    dc.SetDC(sora_complex16{3, -3});
    DevicePin<sora_complex16, 11 * 48> chips(d_chips); chips.append();
    bool ok = despread.Process(chips);
    DevicePin<sora_complex16, 24> sym(d_sym); sym.append(); ok = ok && dqpsk.Process(sym);
    DevicePin<sora_complex16, 64> c5(d_chips); c5.append(); ok = ok && cck5.Process(c5);
    DevicePin<sora_complex16, 32> c11(d_chips); c11.append(); ok = ok && cck11.Process(c11);
    DevicePin<sora_complex16, 28> raw(d_chips); raw.append(); ok = ok && dc.Process(raw);
    cck11.Reset(); cck11.Flush(); despread.Reset(); despread.Flush();
    return ok ? 0 : (int)ctx.error_code;
}
""")
    for s in (str(src), os.path.join(ROOT, "tests", "cxx", "demod11b_chain.cpp")):
        r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), s], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
