"""Stream continuation of the 802.11n receive handle (sora_rx11n_set_stream_mode), checked without a GPU: the two exports are in the library,
declared in the header and bound with argument types; a null handle is refused before any device work; and the stream form of the scan
kernel ships as a kernel of its own that, like the default front ends and the data field's kernels behind them, keeps every register in registers (code-object metadata)."""
import ctypes
import os
import re
import subprocess

import pytest

from test_capi_cpu import declared_functions
from test_isa_dpp_guard import LLVM, ROOT, code_objects

NEW = ("sora_rx11n_set_stream_mode", "sora_rx11n_stream_consumed")
SORA_ERR_INVALID_PARAM = -1                                             # include/sora_hip.h


@pytest.fixture(scope="module")
def lib():
    import sora_amd
    return sora_amd.load(build_if_missing=False)


def test_exports_are_declared_bound_and_typed(lib):
    from sora_amd import capi
    for n in NEW:
        assert hasattr(lib, n), n
        assert n in declared_functions() and n in capi.EXPORTS, n
        assert getattr(lib, n).argtypes is not None, n


# every receive handle's calls-in-flight and stream-mode entry points, and those whose message names them for a null handle
PREFIXES = ("sora_rx", "sora_rx11b", "sora_rx11n", "sora_ht40")
NAMED = {"sora_rx": {"wait_any", "stream_consumed"}, "sora_rx11b": {"wait_any", "set_stream_mode", "stream_consumed"},
         "sora_rx11n": {"wait", "wait_any", "results_of", "deliver_async", "set_stream_mode", "stream_consumed"}, "sora_ht40": {"wait_any"}}


@pytest.mark.parametrize("pre", PREFIXES)
def test_null_handle_is_an_invalid_parameter(lib, pre):
    from sora_amd import capi
    out = (ctypes.c_uint32 * 4)(); rows = (capi.FrameResult * 4)(); n = ctypes.c_size_t(0); t = ctypes.c_int(0)
    calls = [("wait", (None, 1)), ("wait_any", (None, ctypes.byref(t))), ("results_of", (None, 1, rows, 4, ctypes.byref(n), None, 0)),
             ("deliver_async", (None, 1, None, 0, None, None, 0)), ("set_stream_mode", (None, 1)), ("set_stream_mode", (None, -1)),
             ("stream_consumed", (None, 1, ctypes.cast(out, ctypes.c_void_p), 4))]
    for fn, args in calls:
        name = pre + "_" + fn
        if name not in capi.EXPORTS:
            continue
        lib.sora_hip_table_digest(None, None)                           # leaves a message that names no receive handle
        assert getattr(lib, name)(*args) == SORA_ERR_INVALID_PARAM, name
        if fn in NAMED[pre]:
            assert name.encode() in lib.sora_hip_last_error(), (name, lib.sora_hip_last_error())
    assert getattr(lib, pre + "_ticket")(None) == 0
    if pre + "_stream_of" in capi.EXPORTS:
        assert getattr(lib, pre + "_stream_of")(None, 1) is None


def kernel_metadata(tmp_path):
    """{kernel symbol: {field: value}} of every gfx950 code object that holds a k_scan11n kernel"""
    lib = os.path.join(ROOT, "sora_amd", "lib", "libsora_hip.so")
    assert os.path.exists(lib), "libsora_hip.so is not built (__graft_entry__.build() / python -m sora_amd.build)"
    if not os.path.exists(os.path.join(LLVM, "llvm-readobj")):
        pytest.fail("llvm-readobj not found under " + LLVM)
    fat = tmp_path / "fatbin"
    subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", lib, str(fat)])
    out = {}
    for k, co in enumerate(code_objects(fat.read_bytes())):
        if b"k_scan11n" not in co:
            continue
        p = tmp_path / ("co%d.o" % k)
        p.write_bytes(co)
        notes = subprocess.run([os.path.join(LLVM, "llvm-readobj"), "--notes", str(p)], capture_output=True, text=True, check=True).stdout
        for blk in re.split(r"\n\s*- \.agpr_count:", notes)[1:]:
            name = re.search(r"\.name:\s+(\S+)", blk)
            if name:
                out[name.group(1)] = {f: int(v) for f, v in re.findall(r"\.(vgpr_count|private_segment_fixed_size|vgpr_spill_count):\s+(\d+)", blk)}
    return out


def test_stream_scan_kernel_exists_and_nothing_spills(tmp_path):
    md = kernel_metadata(tmp_path)
    names = {re.sub(r"^_ZN4sora\d+(\w+?)ENS_\d+(?:Scan|Frame)11nArgsE.*$", r"\1", k): v for k, v in md.items()}
    for k in ("k_scan11n", "k_scan_ht40", "k_scan11n_stream", "k_frame11n", "k_finish11n"):
        assert k in names, "kernel %s missing from libsora_hip.so (found %s)" % (k, sorted(names))
        assert names[k]["private_segment_fixed_size"] == 0 and names[k].get("vgpr_spill_count", 0) == 0, (k, names[k])
    waves = lambda v: 512 // ((v + 7) // 8 * 8)                          # waves per SIMD the VGPR budget allows (gfx950: 512 per lane)
    assert waves(names["k_scan11n_stream"]["vgpr_count"]) >= waves(names["k_scan11n"]["vgpr_count"]), names
