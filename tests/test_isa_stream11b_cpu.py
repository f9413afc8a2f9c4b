"""The stream form of the 802.11b receive graph ships as kernels of its own (sora_rx11b_set_stream_mode), and the default ones keep their
register budget: read from the code-object metadata of libsora_hip.so, without a GPU."""
import os
import re
import subprocess

import pytest

from test_isa_dpp_guard import LLVM, ROOT, code_objects


def kernel_metadata(tmp_path, holds=b"k_rx11b"):
    """{kernel symbol: {field: value}} of every gfx950 code object that holds a kernel whose symbol contains `holds`"""
    lib = os.path.join(ROOT, "sora_amd", "lib", "libsora_hip.so")
    assert os.path.exists(lib), "libsora_hip.so is not built (__graft_entry__.build() / python -m sora_amd.build)"
    if not os.path.exists(os.path.join(LLVM, "llvm-readobj")):
        pytest.fail("llvm-readobj not found under " + LLVM)
    fat = tmp_path / "fatbin"
    subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", lib, str(fat)])
    out = {}
    for k, co in enumerate(code_objects(fat.read_bytes())):
        if holds not in co:
            continue
        p = tmp_path / ("co%d.o" % k)
        p.write_bytes(co)
        notes = subprocess.run([os.path.join(LLVM, "llvm-readobj"), "--notes", str(p)], capture_output=True, text=True, check=True).stdout
        for blk in re.split(r"\n\s*- \.agpr_count:", notes)[1:]:
            name = re.search(r"\.name:\s+(\S+)", blk)
            if name:
                out[name.group(1)] = {f: int(v) for f, v in re.findall(r"\.(vgpr_count|sgpr_count|private_segment_fixed_size|group_segment_fixed_size|vgpr_spill_count):\s+(\d+)", blk)}
    return out


def test_stream_kernels_exist_and_fit_the_default_budget(tmp_path):
    md = kernel_metadata(tmp_path)
    names = {re.sub(r"^_ZN4sora\d+(\w+?)ENS_9Rx11bArgsE$", r"\1", k): v for k, v in md.items()}
    for k in ("k_rx11b", "k_rx11b_cck", "k_rx11b_stream", "k_rx11b_cck_stream"):
        assert k in names, "kernel %s missing from libsora_hip.so (found %s)" % (k, sorted(names))
    waves = lambda v: 512 // ((v + 7) // 8 * 8)                          # waves per SIMD the VGPR budget allows (gfx950: 512 per lane)
    # the Barker-rate pass: the stream form runs as many waves per SIMD as the default one, and neither spills to memory
    assert waves(names["k_rx11b_stream"]["vgpr_count"]) >= waves(names["k_rx11b"]["vgpr_count"]), names
    assert names["k_rx11b"]["private_segment_fixed_size"] == 0 and names["k_rx11b_stream"]["private_segment_fixed_size"] == 0, names
    assert names["k_rx11b_cck_stream"]["vgpr_count"] <= 128, names
