"""The bricks that complete the 802.11n receive graph as stages, the parts that need no GPU.
1. The per-brick model (tests/rx11n_stage_model.py) is pinned: TCCA11n against Oracle.cca11n burst for burst, with the branches its built streams reach counted (the GPU
   test runs the same streams); T11nDataSymbol, the de-parser and the tail against the oracle's restatement; the model composition against the oracle's whole-capture
   receiver, and against the compiled reference graph where oracle/_ref is built.
2. The surface: declared, exported, bound and typed; a null pointer refused by name before any device work; the adapters and the C++ host compile; no new kernel uses scratch.
(This file fails without the feature: the names do not exist.)

A note on the "full-scale" streams.  At +-32767 nothing wraps inside MimoAutoCorr: a term is 2 x 32767^2 >> 5 = 67104768 and 32 of them add to 2147352576, 131071 short of
2^31 -- a moving sum of 32 terms >> 5 of an int32 cannot leave int32.  What does wrap is the squared norm of a -32768 sample (2^31), and with it acorr (2^63 on a stream of
nothing else).  The cases hold streams at +-32767 AND streams at the int16 rails, and the wrap branch counts the latter."""
import ctypes
import os
import re
import subprocess
import zlib

import numpy as np
import pytest

import rx11n_stage_cases as cases
import rx11n_stage_model as model
from oracle.pyoracle import Oracle, ReferenceGraph
from sora_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SORA_OK, SORA_ERR_INVALID_PARAM, SORA_ERR_NO_DEVICE = 0, -1, -5
E_FRAME_OK, E_CRC32_FAIL, E_CS_TIMEOUT = 0x1, 0x80000006, 0x80000007
P = ctypes.c_void_p(4096)                                                        # a pointer that is not null and is never followed: every check below comes first
STAGES = {
    "sora_hip_cca11n":         ([P, P, P, P, P, P, 1, 1, 0, None], (0, 1, 2, 3, 4, 5), 6),
    "sora_hip_data_symbol11n": ([P, P, P, P, P, P, P, 1, 1, None], (0, 1, 2, 3, 4, 5, 6), 7),
    "sora_hip_stream_join11n": ([P, P, P, 2, 1, None], (0, 1, 2), 4),
    "sora_hip_desc11a":        ([P, P, P, P, P, 1, None], (0, 1, 2, 3, 4), 5),
    "sora_hip_frame_sink11a":  ([P, P, P, P, 1, None], (0, 1, 2, 3), 4),
}
NEW_KERNELS = ("k_cca11n", "k_data_symbol11n", "k_stream_join11n", "k_desc11a", "k_frame_sink11a")


@pytest.fixture(scope="module")
def o():
    return Oracle()


@pytest.fixture(scope="module")
def streams():
    return cases.built_streams()


def detections(x0, x1, skip, branches=None):
    """what so_cca11n reports, through the model's brick: REARM, and after a detection `skip` bursts withheld and the brick Reset"""
    st = capi.cca11n_states(1)[0]; pos = 0; nb = len(x0) // 4; det = []
    while pos < nb:
        st, used = model.cca(x0[4 * pos:], x1[4 * pos:], st, capi.CCA11N_REARM, branches)
        pos += used
        if st[0] == 1:
            det.append(pos - 1); pos += skip
            st = st.copy(); st[0] = 0; st[3:6] = 0
    return det


def test_cca_model_equals_the_oracle_and_the_built_streams_reach_every_branch(o, streams):
    total = np.zeros(16, np.uint32)
    for name, x0, x1 in streams:
        for skip in (0, cases.FRAME_BURSTS):
            assert detections(x0, x1, skip, total) == o.cca11n(x0, x1, skip), (name, skip)
        st, used = model.cca(x0, x1, capi.cca11n_states(1)[0], 0, total)         # without REARM: the first time-out stands
        assert (st[0] == 1) != ((int(st[1]) & 0xFFFFFFFF) == E_CS_TIMEOUT) or used == len(x0) // 4, name
    reached = dict(zip(model.BRANCHES, total.tolist()))
    print("branches reached:", reached)
    assert all(v > 0 for v in reached.values()), reached
    two = np.zeros(16, np.uint32)                                                # two or more time-outs inside ONE call
    st, _ = model.cca(streams[0][1], streams[0][2], capi.cca11n_states(1)[0], capi.CCA11N_REARM, two)
    assert st[7] >= 2 and two[6] == st[7]
    assert any(np.abs(x0).max() <= 3 and np.abs(x1).max() <= 3 for _, x0, x1 in streams) and any(np.abs(x0.astype(np.int32)).min() == 32767 for _, x0, _ in streams)


def test_cca_model_on_random_streams_equals_the_oracle(o):
    rng = np.random.default_rng(77)
    for x0, x1 in cases.lengths_streams(rng):
        for skip in (0, 30):
            assert detections(x0, x1, skip) == o.cca11n(x0, x1, skip)


@pytest.mark.parametrize("flags", [0, capi.CCA11N_REARM])
def test_a_cca_stream_cut_into_two_calls_equals_one_call(streams, flags):
    for name, x0, x1 in streams:
        nb = len(x0) // 4
        one, used = model.cca(x0, x1, capi.cca11n_states(1)[0], flags)
        for cut in sorted({1, max(used - 1, 1), used, min(used + 1, nb), nb - 1}):
            a, ua = model.cca(x0[:4 * cut], x1[:4 * cut], capi.cca11n_states(1)[0], flags)
            b, ub = model.cca(x0[4 * ua:], x1[4 * ua:], a, flags)
            assert ua + ub == used and np.array_equal(b, one), (name, cut)


def test_a_cca_stream_that_enters_decided_consumes_nothing(streams):
    _, x0, x1 = streams[0]
    for word, value in ((0, 1), (1, E_CS_TIMEOUT)):
        st = capi.cca11n_states(1)[0]; st[word] = np.uint32(value).astype(np.int32)
        after, used = model.cca(x0, x1, st, capi.CCA11N_REARM)
        assert used == 0 and np.array_equal(after, st)


def test_model_composition_equals_the_whole_capture_receivers(o):
    """the first event of the composed stages = the first event of Oracle.rx11n_capture (and of the compiled reference graph where it is built)"""
    from gpu_util import capture_11n
    z = np.load(cases.GOLD)
    g = ReferenceGraph()
    key = lambda r: None if r is None else (r["error_code"], r["rate_kbps"], r["length"], r["crc32"], r["mpdu"])
    kinds = set()
    for i in range(4):
        for seed in range(4):
            a, b = capture_11n(np.random.default_rng(50 * i + seed), [(z["tx%d_0" % i], z["tx%d_1" % i])], sigma=[20.0, 90.0][seed & 1])
            ev = model.first_events(a, b, [(0, len(a))])[0]
            want = o.rx11n_capture(a, b)
            assert key(ev) == key(want[0] if want else None), (i, seed)
            if g.available():
                ref = g.rx11n(a, b)                                              # (behind a failed header the compiled graph reports stale rate and length fields)
                r0 = key(ref[0]) if ref else None
                assert (ev is None) == (r0 is None) and (ev is None or key(ev)[:1 if ev["error_code"] == 0x80000005 else 4] == r0[:1 if ev["error_code"] == 0x80000005 else 4]), (i, seed)
            kinds.add(ev["error_code"] if ev else None)
    assert {E_FRAME_OK, 0x80000005} <= kinds
    rng = np.random.default_rng(5)
    n = 28 * 200
    noise = [np.rint(rng.normal(0, 30, (n, 2))).astype(np.int16) for _ in range(2)]
    assert model.first_events(noise[0], noise[1], [(0, n)]) == [None] and o.rx11n_capture(noise[0], noise[1]) == []


def test_data_symbol_and_stream_join_equal_the_restatement():
    rng = np.random.default_rng(3)
    x = rng.integers(-32768, 32768, (80 * 7 + 5, 2)).astype(np.int16)
    for first in range(4):
        for nsym in (0, 1, 2, 7):
            got = model.data_symbol(x[first:], nsym)
            want = [x[first + 80 * k + 16 + i] for k in range(nsym) for i in range(64)]
            assert np.array_equal(got, np.array(want, np.int16).reshape(-1, 2))
    for nb in (1, 2, 4, 6):
        s = max(nb // 2, 1)
        d0 = rng.integers(0, 256, (3, 52 * nb)).astype(np.uint8); d1 = rng.integers(0, 256, (3, 52 * nb)).astype(np.uint8)
        got = model.stream_join(d0, d1, nb)
        for g in range(104 * nb):                                                # so_rx11n.c:194 generalised: position g takes element (g / 2s) s + g % s of stream (g / s) & 1
            src = (d1 if (g // s) & 1 else d0)[:, (g // (2 * s)) * s + g % s]
            assert np.array_equal(got[:, g], src), (nb, g)


def tail_cases(o, rng):
    """-> [(decoded bytes, length, good FCS?)]: lengths 4, 5, 14, 1500 and 4095, each with a good FCS and a corrupted one, behind random seeds"""
    out = []
    for length in (4, 5, 14, 1500, 4095):
        for good in (True, False):
            body = rng.integers(0, 256, length - 4, dtype=np.uint8).tobytes()
            fcs = zlib.crc32(body) & 0xFFFFFFFF
            mpdu = np.frombuffer(body + int(fcs).to_bytes(4, "little"), np.uint8).copy()
            if not good:
                mpdu[int(rng.integers(0, length))] ^= 1 << int(rng.integers(0, 8))
            dec = np.zeros(length + 2, np.uint8); dec[0] = rng.integers(0, 256); dec[1] = rng.integers(0, 256)
            seq = o.desc_sink(dec, length)[1]                                    # the scrambler's bytes behind this seed
            dec[2:] = mpdu ^ seq
            out.append((dec, length, good))
    return out


def test_the_tail_equals_the_oracle(o):
    rng = np.random.default_rng(11)
    for dec, length, good in tail_cases(o, rng):
        e, mpdu, crc = o.desc_sink(dec, length)
        by = model.desc(dec, length)
        rec = model.frame_sink(by, length)
        assert np.array_equal(by, mpdu) and (int(rec[0]), int(rec[1])) == (e & 0xFFFFFFFF, crc), (length, good)
        assert (e & 0xFFFFFFFF) == (E_FRAME_OK if good else E_CRC32_FAIL), (length, good)
    for length in (0, 1, 2, 3):                                                  # (ulong)(frame_length - 4) has wrapped: the brick never decides
        assert model.frame_sink(rng.integers(0, 256, 8, dtype=np.uint8), length).tolist() == [0, 0]


# ---- the surface
@pytest.fixture(scope="module")
def lib():
    import sora_amd
    return sora_amd.load()


def test_the_five_are_declared_exported_bound_and_typed(lib):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sora_hip.h")).read(), flags=re.S)
    for name, (args, _, _) in STAGES.items():
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in capi.EXPORTS and hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None and len(getattr(lib, name).argtypes) == len(args), name
    assert lib.sora_hip_abi_version() == 4
    assert "sora_cca11n_state" in header and "sora_sink11a_rec" in header and "SORA_CCA11N_REARM" in header


def test_python_surface():
    import sora_amd
    for name in ("cca11n", "data_symbol11n", "stream_join11n", "desc11a", "frame_sink11a", "cca11n_states", "rx11n_by_stages", "rx11n_stages"):
        assert callable(getattr(sora_amd, name)), name
    assert "not a fast path" in sora_amd.rx11n_by_stages.__doc__
    st = sora_amd.cca11n_states(3)
    assert st.shape == (3, 264) and (st[:, :8] == 0).all() and (st[:, 136:] == 0).all()
    assert (st[:, 8:136].view(np.int64) == np.iinfo(np.int64).max).all()        # the ring starts at LLONG_MAX


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


def test_stream_join_refuses_three_bits_per_carrier(lib):
    assert lib.sora_hip_stream_join11n(P, P, P, 3, 1, None) == SORA_ERR_INVALID_PARAM
    assert b"sora_hip_stream_join11n" in lib.sora_hip_last_error()


def test_the_adapters_and_the_host_compile(tmp_path):
    src = tmp_path / "graph11n.cpp"
    src.write_text("""
#include "sora_brick.hpp"
using namespace sora_brick;
int build_graph(sora_complex16* d_a, sora_complex16* d_b, uint8_t* d_s, uint8_t* d_out, void* d_tab, sora_cca11n_state* d_cca, sora_sink11a_rec* d_rec) {
    CF_Error ctx; TDrop<CF_Error> drop(ctx);
    uint32_t* t = static_cast<uint32_t*>(d_tab);
    THip11nDataSymbol<3, CF_Error, TDrop<CF_Error>> ds(ctx, &drop, d_b, t);
    DevicePin<sora_complex16, 2 * 240> in(d_a); in.append();
    bool ok = ds.Process(in);
    THip11nStreamJoin<4, 5, CF_Error, TDrop<CF_Error>> join(ctx, &drop, d_out);
    DevicePin<uint8_t, 104 * 4 * 5> soft(d_s); soft.append();
    ok = ok && join.Process(soft);
    CF_11aSink sink; THip11aFrameSink fsink(sink, d_rec, t + 4);
    THip11aDesc<CF_Error, THip11aFrameSink> desc(ctx, &fsink, d_out, t + 8);
    desc.SetFrame(100); fsink.SetFrame(100);
    DevicePin<uint8_t, 102> dec(d_s); dec.append();
    const bool undecided = desc.Process(dec);
    CF_11nCCA cca; THip11nCCA<16> sense(cca, d_cca, t + 12, SORA_CCA11N_REARM);
    DevicePin<sora_complex16, 2 * 64> bursts(d_a); bursts.append();
    ok = ok && sense.Process(bursts) && sense.Reset();
    ds.Reset(); ds.Flush(); sense.Flush(); desc.Reset();
    return ok && !undecided ? (int)(cca.cca_state + sink.error_code + sense.used()) : (int)ctx.error_code;
}
""")
    for s in (str(src), os.path.join(ROOT, "tests", "cxx", "rx11n_tail_chain.cpp")):
        r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), s], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr


def test_no_new_kernel_uses_scratch(tmp_path):
    from test_isa_dpp_guard import LLVM, code_objects
    so = os.path.join(ROOT, "sora_amd", "lib", "libsora_hip.so")
    assert os.path.exists(so), "libsora_hip.so is not built (__graft_entry__.build() / python -m sora_amd.build)"
    if not os.path.exists(os.path.join(LLVM, "llvm-readobj")):
        pytest.fail("llvm-readobj not found under " + LLVM)
    fat = tmp_path / "fatbin"
    subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", so, str(fat)])
    found = {}
    for k, co in enumerate(code_objects(fat.read_bytes())):
        if b"k_cca11n" not in co:
            continue
        p = tmp_path / ("co%d.o" % k)
        p.write_bytes(co)
        notes = subprocess.run([os.path.join(LLVM, "llvm-readobj"), "--notes", str(p)], capture_output=True, text=True, check=True).stdout
        for blk in re.split(r"\n\s*- \.agpr_count:", notes)[1:]:
            name = re.search(r"\.name:\s+(\S+)", blk)
            if name and any(kn in name.group(1) for kn in NEW_KERNELS):
                found[name.group(1)] = {f: int(v) for f, v in re.findall(r"\.(vgpr_count|private_segment_fixed_size|vgpr_spill_count):\s+(\d+)", blk)}
    for kn in NEW_KERNELS:
        assert any(kn in name for name in found), "kernel %s missing from libsora_hip.so (found %s)" % (kn, sorted(found))
    assert len(found) == 7, sorted(found)                                       # the join has one instance per group size
    for name, md in found.items():
        assert md["private_segment_fixed_size"] == 0 and md.get("vgpr_spill_count", 0) == 0, (name, md)
        assert not any(s in name for s in ("k_scan11n", "k_frame11n", "k_finish11n")), name
