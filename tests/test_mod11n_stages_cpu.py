"""The stage entry points of the 802.11n modulation graphs (include/sora_hip.h, sora_amd/csrc/k_mod11n.hip), the parts that need no GPU: the exports exist, are
declared, bound and typed; their argument checks; the host's share of the composition; the BRICK adapters and the C++ graph built from them compile as a user's would."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAGES = ["sora_hip_stream_parse11n", "sora_hip_interleave11n", "sora_hip_map11n", "sora_hip_sig_map11n", "sora_hip_add_pilot11n", "sora_hip_ifft_only11n",
          "sora_hip_csd11n", "sora_hip_add_gi11n", "sora_hip_preamble11n"]
WRAPPERS = ["stream_parse11n", "interleave11n", "map11n", "sig_map11n", "add_pilot11n", "ifft_only11n", "csd11n", "add_gi11n", "preamble11n", "mod11n_fields",
            "mod11n_by_stages", "Mod11nStages"]
P = 0x7f0000001000                                                               # 16-byte aligned addresses that are never dereferenced: no call below gets to a launch
Q = P + 0x100000
R = Q + 0x100000


@pytest.fixture(scope="module")
def sora():
    import sora_amd
    sora_amd.load()
    return sora_amd


def calls(L, p=P, q=Q, r=R):
    """name -> (function, arguments with every pointer non-null, indices of the pointers that must not be null, index of the count)"""
    return {
        "sora_hip_stream_parse11n": (L.sora_hip_stream_parse11n, [p, q, r, 1, 1, None], [0, 1, 2], 4),
        "sora_hip_interleave11n": (L.sora_hip_interleave11n, [p, q, 1, 0, 1, None], [0, 1], 4),
        "sora_hip_map11n": (L.sora_hip_map11n, [p, q, 1, 0, 1, None], [0, 1], 4),
        "sora_hip_sig_map11n": (L.sora_hip_sig_map11n, [p, q, 1, None], [0, 1], 2),
        "sora_hip_add_pilot11n": (L.sora_hip_add_pilot11n, [p, q, p, p, p, 1, 0, None], [0, 1, 2, 3], 5),           # (d_pos0 may be null)
        "sora_hip_ifft_only11n": (L.sora_hip_ifft_only11n, [p, q, 1, None], [0, 1], 2),
        "sora_hip_csd11n": (L.sora_hip_csd11n, [p, q, 2, 1, None], [0, 1], 3),
        "sora_hip_add_gi11n": (L.sora_hip_add_gi11n, [p, q, 1, None], [0, 1], 2),
        "sora_hip_preamble11n": (L.sora_hip_preamble11n, [q, r, 0, 1, None], [0, 1], 3),
    }


def test_the_nine_stages_are_exported_declared_bound_and_typed(sora):
    from sora_amd import capi
    L = sora.load()
    header = open(os.path.join(ROOT, "include", "sora_hip.h")).read()
    for name in STAGES:
        assert name in capi.EXPORTS, name
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        f = getattr(L, name)
        assert f.argtypes is not None and f.argtypes[-1] is ctypes.c_void_p, name
        assert len(f.argtypes) == len(calls(L)[name][1]), name
    assert header.index("sora_hip_preamble11a(") < header.index("sora_hip_stream_parse11n(") < header.index("sora_hip_tx11n(")   # behind the 802.11a modulation stages
    for w in WRAPPERS:
        assert callable(getattr(sora, w, None) or getattr(capi, w)), w
    assert L.sora_hip_abi_version() == 4
    assert "k_mod11n.hip" in __import__("sora_amd.build", fromlist=["SOURCES"]).SOURCES


def test_a_null_pointer_is_refused_and_without_a_device_so_is_everything_else(sora):
    L = sora.load()
    have_gpu = sora.device_count() > 0
    for name, (f, args, ptrs, _) in calls(L).items():
        for i in ptrs:
            a = list(args); a[i] = None
            assert f(*a) == -1, (name, i)                                        # SORA_ERR_INVALID_PARAM, with or without a device
            assert b"null pointer" in L.sora_hip_last_error()
        if not have_gpu:                                                         # (with a device these addresses would be launched on)
            assert f(*args) == -5, name                                          # SORA_ERR_NO_DEVICE


def test_argument_checks_that_come_before_any_launch(sora):
    """On a machine with a device these are refused for the argument; without one the missing device is reported first -- refused either way, never 0."""
    L = sora.load()
    have_gpu = sora.device_count() > 0
    bad = {"parse n_bpsc 3": L.sora_hip_stream_parse11n(P, Q, R, 3, 1, None), "parse n_bpsc 5": L.sora_hip_stream_parse11n(P, Q, R, 5, 1, None),
           "interleave n_bpsc 3": L.sora_hip_interleave11n(P, Q, 3, 0, 1, None), "interleave n_bpsc 5": L.sora_hip_interleave11n(P, Q, 5, 0, 1, None),
           "map n_bpsc 3": L.sora_hip_map11n(P, Q, 3, 0, 1, None), "map n_bpsc 5": L.sora_hip_map11n(P, Q, 5, 0, 1, None), "map mod": L.sora_hip_map11n(P, Q, 2, 40000, 1, None),
           "interleave stream -1": L.sora_hip_interleave11n(P, Q, 1, -1, 1, None), "interleave stream 2": L.sora_hip_interleave11n(P, Q, 1, 2, 1, None),
           "pilot stream -1": L.sora_hip_add_pilot11n(P, Q, P, P, None, 1, -1, None), "pilot stream 2": L.sora_hip_add_pilot11n(P, Q, P, P, None, 1, 2, None),
           "csd 0": L.sora_hip_csd11n(P, Q, 0, 1, None), "csd 32": L.sora_hip_csd11n(P, Q, 32, 1, None), "csd in place": L.sora_hip_csd11n(P, P, 2, 1, None),
           "field 2": L.sora_hip_preamble11n(Q, R, 2, 1, None),
           "parse in": L.sora_hip_stream_parse11n(P + 4, Q, R, 1, 1, None), "parse out1": L.sora_hip_stream_parse11n(P, Q, R + 8, 1, 1, None),
           "interleave in": L.sora_hip_interleave11n(P + 2, Q, 1, 0, 1, None), "map out": L.sora_hip_map11n(P, Q + 4, 1, 0, 1, None),
           "sig_map in": L.sora_hip_sig_map11n(P + 1, Q, 1, None), "pilot in": L.sora_hip_add_pilot11n(P + 8, Q, P, P, None, 1, 0, None),
           "ifft out": L.sora_hip_ifft_only11n(P, Q + 8, 1, None), "csd in": L.sora_hip_csd11n(P + 4, Q, 2, 1, None), "gi out": L.sora_hip_add_gi11n(P, Q + 4, 1, None),
           "preamble out1": L.sora_hip_preamble11n(Q, R + 4, 0, 1, None)}
    assert all(rc == (-1 if have_gpu else -5) for rc in bad.values()), bad
    if have_gpu:                                                                 # a count of 0 launches nothing
        for name, (f, args, ptrs, cnt) in calls(L).items():
            a = list(args); a[cnt] = 0
            assert f(*a) == 0, name


@pytest.mark.parametrize("mcs", range(8, 15))
def test_fields_of_the_binding_are_the_models(mcs):
    import mod11n_model as M
    from sora_amd.capi import mod11n_fields
    for ln in (1, 2, 37, 151, 1496):
        mp = bytes(np.random.default_rng([mcs, ln]).integers(0, 256, ln).astype(np.uint8))
        a, b = mod11n_fields(mp, mcs, 0x5B), M.fields(mp, mcs)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2] and a[3] == b[3], (mcs, ln)
        assert a[4] == 0x5B


def test_fields_count_the_symbols_the_transmitter_emits(sora):
    from sora_amd.capi import mod11n_fields
    for mcs, ln in [(10, 150), (8, 7), (14, 1), (12, 30), (9, 4092), (13, 1)]:   # the reference's extra symbol among them
        assert 1600 + 160 * mod11n_fields(bytes(ln), mcs)[3] == sora.tx11n_samples(ln, mcs), (mcs, ln)


def test_by_stages_refuses_what_tx11n_refuses(sora):
    for mpdus, mcs in ([[b"\x01\x02\x03"], [7]], [[b"\x01\x02\x03"], [15]], [[b""], [9]], [[b"\x01", b"\x02"], [9, 7]], [[bytes(4093)], [8]]):
        with pytest.raises(sora.SoraError):
            sora.mod11n_by_stages(mpdus, mcs)


@pytest.mark.parametrize("what", ["sora_brick.hpp", "mod11n_chain.cpp"])
def test_adapters_and_the_cxx_graph_compile_clean(tmp_path, what):
    if what == "sora_brick.hpp":                                                 # (a header is checked as a user includes it)
        src = tmp_path / "include_brick.cpp"; src.write_text('#include "sora_brick.hpp"\n')
    else:
        src = os.path.join(ROOT, "tests", "cxx", "mod11n_chain.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    hdr = open(os.path.join(ROOT, "include", "sora_brick.hpp")).read()
    for cls in ["THipStreamParser", "THip11nInterleave", "THipMap11n", "THipSigMap11n", "THip11nAddPilot", "THipIFFTxOnly", "THipCSD", "THipAddGI"]:
        assert re.search(r"\b(class|struct) %s\b" % cls, hdr), cls
