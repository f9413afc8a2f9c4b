"""The stage entry points of the 802.11a modulation graph (include/sora_hip.h, sora_amd/csrc/k_mod.hip), the parts that need no GPU: the exports exist, are
declared, bound and typed; their argument checks; the BRICK adapters and the C++ graph built from them compile as a user's would."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAGES = ["sora_hip_scramble11a", "sora_hip_conv_encode11a", "sora_hip_interleave11a", "sora_hip_map11a", "sora_hip_add_pilot11a", "sora_hip_ifftx11a",
          "sora_hip_upsample40to44", "sora_hip_pack16to8", "sora_hip_preamble11a"]
WRAPPERS = ["scramble11a", "conv_encode11a", "interleave11a", "map11a", "add_pilot11a", "ifftx11a", "upsample40to44", "pack16to8", "preamble11a", "mod11a_by_stages"]
P = 0x7f0000001000                                                               # a 16-byte aligned address that is never dereferenced: no call below gets to a launch
Q = P + 0x100000


@pytest.fixture(scope="module")
def sora():
    import sora_amd
    sora_amd.load()
    return sora_amd


def calls(L, p=P, q=Q):
    """name -> (function, arguments with every pointer non-null, indices of the pointers that must not be null)"""
    return {
        "sora_hip_scramble11a": (L.sora_hip_scramble11a, [p, q, p, p, p, p, 1, 16, None], [0, 1, 2, 3, 5]),          # (d_tail may be null)
        "sora_hip_conv_encode11a": (L.sora_hip_conv_encode11a, [p, p, p, 0, q, p, 1, 16, None], [0, 1, 2, 4, 5]),
        "sora_hip_interleave11a": (L.sora_hip_interleave11a, [p, q, 1, 1, None], [0, 1]),
        "sora_hip_map11a": (L.sora_hip_map11a, [p, q, 1, 0, 1, None], [0, 1]),
        "sora_hip_add_pilot11a": (L.sora_hip_add_pilot11a, [p, q, p, p, 1, 0, None], [0, 1, 2, 3]),
        "sora_hip_add_pilot11a_from": (L.sora_hip_add_pilot11a_from, [p, q, p, p, p, 1, 0, None], [0, 1, 2, 3]),  # (d_pos0 may be null)
        "sora_hip_ifftx11a": (L.sora_hip_ifftx11a, [p, q, 1, None], [0, 1]),
        "sora_hip_upsample40to44": (L.sora_hip_upsample40to44, [p, q, p, 1, None], [0, 1]),                       # (d_sees_next may be null)
        "sora_hip_pack16to8": (L.sora_hip_pack16to8, [p, q, 8, None], [0, 1]),
        "sora_hip_preamble11a": (L.sora_hip_preamble11a, [q, 1, None], [0]),
    }


def test_the_nine_stages_are_exported_declared_bound_and_typed(sora):
    from sora_amd import capi
    L = sora.load()
    header = open(os.path.join(ROOT, "include", "sora_hip.h")).read()
    for name in STAGES + ["sora_hip_add_pilot11a_from"]:
        assert name in capi.EXPORTS, name
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        f = getattr(L, name)
        assert f.argtypes is not None and f.argtypes[-1] is ctypes.c_void_p, name
        assert len(f.argtypes) == len(calls(L)[name][1]), name
    for w in WRAPPERS:
        assert callable(getattr(sora, w)), w
    assert L.sora_hip_abi_version() == 4
    assert "k_mod.hip" in __import__("sora_amd.build", fromlist=["SOURCES"]).SOURCES


def test_a_null_pointer_is_refused_and_without_a_device_so_is_everything_else(sora):
    L = sora.load()
    have_gpu = sora.device_count() > 0
    for name, (f, args, ptrs) in calls(L).items():
        for i in ptrs:
            a = list(args); a[i] = None
            assert f(*a) == -1, (name, i)                                        # SORA_ERR_INVALID_PARAM, with or without a device
            assert b"null pointer" in L.sora_hip_last_error()
        if not have_gpu:                                                         # (with a device these addresses would be launched on)
            assert f(*args) == -5, name                                          # SORA_ERR_NO_DEVICE


def test_argument_checks_that_come_before_any_launch(sora):
    """On a machine with a device these are refused for the argument; without one the missing device is reported first for some -- refused either way, never 0."""
    L = sora.load()
    have_gpu = sora.device_count() > 0
    bad = [L.sora_hip_interleave11a(P, Q, 3, 1, None), L.sora_hip_map11a(P, Q, 5, 0, 1, None), L.sora_hip_map11a(P, Q, 2, 40000, 1, None),
           L.sora_hip_conv_encode11a(P, P, P, 3, Q, P, 1, 16, None), L.sora_hip_pack16to8(P, Q, 12, None), L.sora_hip_ifftx11a(P + 4, Q, 1, None),
           L.sora_hip_ifftx11a(P, Q + 8, 1, None), L.sora_hip_interleave11a(P + 2, Q, 1, 1, None), L.sora_hip_preamble11a(Q + 4, 1, None),
           L.sora_hip_upsample40to44(P, Q + 4, None, 1, None), L.sora_hip_add_pilot11a(P + 8, Q, P, P, 1, 0, None)]
    assert all(rc == (-1 if have_gpu else -5) for rc in bad), bad
    if have_gpu:                                                                 # a count of 0 launches nothing
        for name, (f, args, ptrs) in calls(L).items():
            a = list(args); a[{"sora_hip_scramble11a": 6, "sora_hip_conv_encode11a": 6, "sora_hip_interleave11a": 3, "sora_hip_map11a": 4, "sora_hip_add_pilot11a": 4,
                               "sora_hip_add_pilot11a_from": 5, "sora_hip_ifftx11a": 2, "sora_hip_upsample40to44": 3, "sora_hip_pack16to8": 2,
                               "sora_hip_preamble11a": 1}[name]] = 0
            assert f(*a) == 0, name


def test_by_stages_refuses_what_tx11a_refuses(sora):
    with pytest.raises(ValueError):
        sora.mod11a_by_stages([b"x" * 10], [6000], sample_rate_mhz=20)


def test_fields_of_the_binding_are_the_models():
    import numpy as np
    import mod11a_model as M
    from sora_amd.capi import mod11a_fields
    for rate in M.RATES:
        for ln in (1, 2, 37, 260, 1496):
            mp = bytes(np.random.default_rng(ln).integers(0, 256, ln).astype(np.uint8))
            a, b = mod11a_fields(mp, rate), M.fields(mp, rate)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]


@pytest.mark.parametrize("what", ["sora_brick.hpp", "mod_chain.cpp"])
def test_adapters_and_the_cxx_graph_compile_clean(tmp_path, what):
    if what == "sora_brick.hpp":                                                 # (a header is checked as a user includes it)
        src = tmp_path / "include_brick.cpp"; src.write_text('#include "sora_brick.hpp"\n')
    else:
        src = os.path.join(ROOT, "tests", "cxx", "mod_chain.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    hdr = open(os.path.join(ROOT, "include", "sora_brick.hpp")).read()
    for cls in ["THip11aSc", "THipConvEncode", "THip11aInterleave", "THipMap11a", "THip11aAddPilot", "THipIFFTx", "THipUpsample40MTo44M", "THipPackSample16to8"]:
        assert re.search(r"\b(class|struct) %s\b" % cls, hdr), cls
