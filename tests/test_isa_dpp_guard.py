"""A guard against the folded-DPP miscompile: hipcc once folded a v_mov_b32_dpp into the REVERSED form of the instruction
that consumed it (v_subrev_u32_dpp), and on gfx950 that computed the negated difference.  The trellis kernels are the heaviest DPP users, so every
gfx950 code object that libsora_hip.so ships is disassembled here and no reversed non-commutative VOP2 opcode may carry a DPP modifier.  Runs
without a GPU: the code objects are read out of the library's .hip_fatbin section."""
import os
import re
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/llvm/bin"
REVERSED_DPP = re.compile(r"\b(v_\w*rev\w*_dpp)\b")          # v_subrev_u32_dpp, v_lshlrev_b32_dpp, v_subrev_f32_e64_dpp, ...
LABEL = re.compile(r"^[0-9a-f]+ <(.+)>:$")


def code_objects(fatbin):
    """the device ELF images inside a fat binary section (one offload bundle per translation unit)"""
    out, i = [], 0
    while True:
        i = fatbin.find(b"\x7fELF", i)
        if i < 0:
            return out
        if fatbin[i + 4] == 2 and struct.unpack_from("<H", fatbin, i + 0x12)[0] == 224:      # ELFCLASS64, EM_AMDGPU
            shoff, = struct.unpack_from("<Q", fatbin, i + 0x28)
            shentsize, shnum = struct.unpack_from("<HH", fatbin, i + 0x3A)
            end = i + shoff + shentsize * shnum
            out.append(fatbin[i:end])
            i = end
        else:
            i += 4


def reversed_dpp(disassembly):
    """[(kernel, instruction line)] for every reversed opcode with a DPP modifier"""
    hits, fn = [], "?"
    for line in disassembly.splitlines():
        m = LABEL.match(line.strip())
        if m:
            fn = m.group(1)
        elif REVERSED_DPP.search(line):
            hits.append((fn, line.strip()))
    return hits


def test_the_pattern_is_recognised():
    dis = "0000000000001000 <k_viterbi16>:\n\tv_sub_u32_dpp v1, v2, v3 row_shr:1\n\tv_subrev_u32_dpp v4, v5, v6 quad_perm:[1,0,3,2] row_mask:0xf\n"
    assert reversed_dpp(dis) == [("k_viterbi16", "v_subrev_u32_dpp v4, v5, v6 quad_perm:[1,0,3,2] row_mask:0xf")]
    assert reversed_dpp("<f>:\n\tv_subrev_u32_e32 v1, v2, v3\n\tv_mov_b32_dpp v1, v2 row_shr:1\n") == []


def test_no_reversed_dpp_opcode_in_the_shipped_code_objects(tmp_path):
    lib = os.path.join(ROOT, "sora_amd", "lib", "libsora_hip.so")
    assert os.path.exists(lib), "libsora_hip.so is not built (__graft_entry__.build() / python -m sora_amd.build)"
    if not os.path.exists(os.path.join(LLVM, "llvm-objdump")):
        pytest.fail("llvm-objdump not found under " + LLVM)
    fat = tmp_path / "fatbin"
    subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", lib, str(fat)])
    objs = code_objects(fat.read_bytes())
    assert len(objs) >= 10, "expected one gfx950 code object per source, found %d" % len(objs)
    hits, dpp = [], 0
    for k, co in enumerate(objs):
        p = tmp_path / ("co%d.o" % k)
        p.write_bytes(co)
        dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "-C", "--mcpu=gfx950", str(p)], capture_output=True, text=True, check=True).stdout
        dpp += dis.count("_dpp ")
        hits += reversed_dpp(dis)
    assert dpp > 1000, "the disassembly holds too few DPP instructions (%d): is this the trellis library?" % dpp
    assert not hits, "reversed opcode with a DPP modifier (the folded-DPP miscompile, DESIGN.md 3.11):\n" + "\n".join(
        "  %s: %s" % h for h in hits[:40])
