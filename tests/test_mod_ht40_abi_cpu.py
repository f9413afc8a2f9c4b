"""The stage entry points of the 40 MHz HT modulation graph (include/sora_hip.h, sora_amd/csrc/k_mod_ht40.hip), the parts that need no GPU: the exports exist, are
declared, bound and typed; their argument checks; the host's share of the composition against the model; the BRICK adapters and the C++ graph built from them compile
as a user's would."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAGES = ["sora_hip_stream_parse_ht40", "sora_hip_interleave_ht40", "sora_hip_interleave_ht40_stream", "sora_hip_map_ht40", "sora_hip_sig_map_ht40",
          "sora_hip_add_pilot_ht40", "sora_hip_ifft_ht40", "sora_hip_add_gi_ht40", "sora_hip_preamble_ht40"]
WRAPPERS = ["stream_parse_ht40", "interleave_ht40", "interleave_ht40_stream", "map_ht40", "sig_map_ht40", "add_pilot_ht40", "ifft_ht40", "add_gi_ht40", "preamble_ht40",
            "mod_ht40_fields", "mod_ht40_by_stages", "ModHt40Stages"]
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
        "sora_hip_stream_parse_ht40": (L.sora_hip_stream_parse_ht40, [p, q, r, 1, 1, None], [0, 1, 2], 4),
        "sora_hip_interleave_ht40": (L.sora_hip_interleave_ht40, [p, q, 1, 0, 1, None], [0, 1], 4),
        "sora_hip_interleave_ht40_stream": (L.sora_hip_interleave_ht40_stream, [p, p, p, p, q, 1, 0, 1, None], [0, 1, 2, 3, 4], 7),
        "sora_hip_map_ht40": (L.sora_hip_map_ht40, [p, q, 1, 1, None], [0, 1], 3),
        "sora_hip_sig_map_ht40": (L.sora_hip_sig_map_ht40, [p, q, 1, None], [0, 1], 2),
        "sora_hip_add_pilot_ht40": (L.sora_hip_add_pilot_ht40, [p, q, p, p, 1, None], [0, 1, 2, 3], 4),
        "sora_hip_ifft_ht40": (L.sora_hip_ifft_ht40, [p, q, 1, None], [0, 1], 2),
        "sora_hip_add_gi_ht40": (L.sora_hip_add_gi_ht40, [p, q, 0, 1, None], [0, 1], 3),
        "sora_hip_preamble_ht40": (L.sora_hip_preamble_ht40, [q, r, 0, 1, None], [0, 1], 3),
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
        decl = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, header).group(1)   # the binding's argument types are the declaration's, one by one
        for ct, arg in zip(f.argtypes, decl.split(",")):
            want = ctypes.c_void_p if "*" in arg else ctypes.c_size_t if "size_t" in arg else ctypes.c_int
            assert ct is want, (name, arg.strip(), ct)
    assert header.index("sora_hip_tx_ht40_joint_gi(") < header.index("sora_hip_stream_parse_ht40(") < header.index("sora_hip_tx11b_samples(")
    for w in WRAPPERS:
        assert callable(getattr(sora, w, None)), w
    assert L.sora_hip_abi_version() == 4                                         # additive: the ABI version is the parent's
    assert re.search(r"#define\s+SORA_HIP_ABI_VERSION\s+4\b", header)
    assert "k_mod_ht40.hip" in __import__("sora_amd.build", fromlist=["SOURCES"]).SOURCES


def test_a_null_pointer_is_refused_by_name_and_without_a_device_so_is_everything_else(sora):
    L = sora.load()
    have_gpu = sora.device_count() > 0
    for name, (f, args, ptrs, _) in calls(L).items():
        for i in ptrs:
            a = list(args); a[i] = None
            assert f(*a) == -1, (name, i)                                        # SORA_ERR_INVALID_PARAM, with or without a device
            assert (name + ": null pointer").encode() in L.sora_hip_last_error(), (name, L.sora_hip_last_error())
        if not have_gpu:                                                         # (with a device these addresses would be launched on)
            assert f(*args) == -5, name                                          # SORA_ERR_NO_DEVICE


def test_a_count_of_zero_is_ok_with_or_without_a_device(sora):
    L = sora.load()
    for name, (f, args, ptrs, cnt) in calls(L).items():
        a = list(args); a[cnt] = 0
        assert f(*a) == 0, name


def test_a_bad_kind_is_refused_before_the_count_is_looked_at(sora):
    """n_bpsc, spatial_stream, gi and field are refused with or without a device, and even for a count of 0, as by the receive stages of this graph"""
    L = sora.load()
    for cnt in (1, 0):
        bad = {"parse n_bpsc 3": L.sora_hip_stream_parse_ht40(P, Q, R, 3, cnt, None), "parse n_bpsc 0": L.sora_hip_stream_parse_ht40(P, Q, R, 0, cnt, None),
               "interleave n_bpsc 3": L.sora_hip_interleave_ht40(P, Q, 3, 0, cnt, None), "interleave n_bpsc 5": L.sora_hip_interleave_ht40(P, Q, 5, 0, cnt, None),
               "interleave stream 2": L.sora_hip_interleave_ht40(P, Q, 1, 2, cnt, None), "interleave stream -1": L.sora_hip_interleave_ht40(P, Q, 1, -1, cnt, None),
               "stream n_bpsc 3": L.sora_hip_interleave_ht40_stream(P, P, P, P, Q, 3, 0, cnt, None),
               "stream stream 2": L.sora_hip_interleave_ht40_stream(P, P, P, P, Q, 6, 2, cnt, None),
               "map n_bpsc 3": L.sora_hip_map_ht40(P, Q, 3, cnt, None), "map n_bpsc 8": L.sora_hip_map_ht40(P, Q, 8, cnt, None),
               "gi 2": L.sora_hip_add_gi_ht40(P, Q, 2, cnt, None), "gi -1": L.sora_hip_add_gi_ht40(P, Q, -1, cnt, None),
               "field 2": L.sora_hip_preamble_ht40(Q, R, 2, cnt, None)}
        assert all(rc == -1 for rc in bad.values()), (cnt, bad)                  # SORA_ERR_INVALID_PARAM
    assert L.sora_hip_add_gi_ht40(P, Q, 2, 1, None) == -1 and b"gi must be 0" in L.sora_hip_last_error()
    assert L.sora_hip_map_ht40(P, Q, 3, 1, None) == -1 and b"n_bpsc must be 1, 2, 4 or 6" in L.sora_hip_last_error()


def test_a_misaligned_symbol_buffer_is_refused(sora):
    """On a machine with a device these are refused for the argument; without one the missing device is reported first -- refused either way, never 0."""
    L = sora.load()
    have_gpu = sora.device_count() > 0
    bad = {"parse in": L.sora_hip_stream_parse_ht40(P + 4, Q, R, 1, 1, None), "parse out1": L.sora_hip_stream_parse_ht40(P, Q, R + 8, 1, 1, None),
           "interleave in": L.sora_hip_interleave_ht40(P + 2, Q, 1, 0, 1, None), "stream out": L.sora_hip_interleave_ht40_stream(P, P, P, P, Q + 1, 1, 0, 1, None),
           "map out": L.sora_hip_map_ht40(P, Q + 4, 1, 1, None), "sig_map in": L.sora_hip_sig_map_ht40(P + 1, Q, 1, None),
           "pilot in": L.sora_hip_add_pilot_ht40(P + 8, Q, P, P, 1, None), "ifft out": L.sora_hip_ifft_ht40(P, Q + 8, 1, None),
           "gi out": L.sora_hip_add_gi_ht40(P, Q + 4, 1, 1, None), "preamble out1": L.sora_hip_preamble_ht40(Q, R + 4, 0, 1, None)}
    assert all(rc == (-1 if have_gpu else -5) for rc in bad.values()), bad


@pytest.mark.parametrize("mcs", range(8, 15))
def test_fields_of_the_binding_are_the_models(mcs):
    import mod_ht40_model as M
    from sora_amd.capi import mod_ht40_fields
    for ln in (1, 2, 37, 151, 1496):
        a, b = (bytes(np.random.default_rng([mcs, ln, s]).integers(0, 256, ln).astype(np.uint8)) for s in (0, 1))
        for coding, mp, seeds in ((0, (a, b), (0x5B, 0x01)), (1, a, 0x5B), (0, (a, b), None), (1, a, None)):
            for gi in (0, 1):
                x, y = mod_ht40_fields(mp, mcs, coding, gi, seeds), M.fields(mp, mcs, coding, gi, seeds)
                assert np.array_equal(x[0], y[0]), (mcs, ln, coding, gi)
                assert len(x[1]) == len(y[1]) and all(np.array_equal(p, q) for p, q in zip(x[1], y[1])), (mcs, ln, coding, gi)
                assert x[2:] == y[2:], (mcs, ln, coding, gi, x[2:], y[2:])
                assert all(len(d) % (1, 2, 3)[M.m.MCS2[mcs][1]] == 0 for d in x[1])   # whole bursts of the encoder stage


def test_fields_count_the_symbols_the_transmitters_emit(sora):
    from sora_amd.capi import mod_ht40_fields
    for mcs, ln in [(10, 150), (8, 7), (14, 1), (12, 30), (9, 3996), (13, 1)]:
        for gi in (0, 1):
            assert 1600 + (144 if gi else 160) * mod_ht40_fields((bytes(ln), bytes(ln)), mcs, 0, gi)[5] == sora.tx_ht40_gi_samples(ln, mcs, gi), (mcs, ln, gi)
            assert 1600 + (144 if gi else 160) * mod_ht40_fields(bytes(ln), mcs, 1, gi)[5] == sora.tx_ht40_joint_gi_samples(ln, mcs, gi), (mcs, ln, gi)


def test_by_stages_refuses_what_the_transmitters_refuse(sora):
    one = [b"\x01\x02\x03"]
    for a, b, mcs, kw in ((one, one, [7], {}), (one, None, [15], {}), ([b""], None, [9], {}), ([b"\x01", b"\x02"], None, [9, 7], {}), ([bytes(3997)], None, [8], {}),
                          (one, [b"\x01\x02"], [9], {}), (one, None, [9], {"gi": [2]}), (one, one, [9], {"seeds": [0x5D]}), (one, None, [9], {"seeds": [(1, 2)]})):
        with pytest.raises(sora.SoraError):
            sora.mod_ht40_by_stages(a, b, mcs, **kw)


@pytest.mark.parametrize("what", ["sora_brick.hpp", "mod_ht40_chain.cpp"])
def test_adapters_and_the_cxx_graph_compile_clean(tmp_path, what):
    if what == "sora_brick.hpp":                                                 # (a header is checked as a user includes it)
        src = tmp_path / "include_brick.cpp"; src.write_text('#include "sora_brick.hpp"\n')
    else:
        src = os.path.join(ROOT, "tests", "cxx", "mod_ht40_chain.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    hdr = open(os.path.join(ROOT, "include", "sora_brick.hpp")).read()
    for cls in ["THipHt40StreamParser", "THipHt40Interleave", "THipHt40Map", "THipHt40SigMap", "THipHt40AddPilot", "THipHt40IFFT", "THipHt40AddGI"]:
        assert re.search(r"\b(class|struct) %s\b" % cls, hdr), cls
