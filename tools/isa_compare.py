#!/usr/bin/env python3
"""Compare the gfx950 code of two source trees kernel by kernel, without a GPU (a refactor's "same code generation" check).

    python tools/isa_compare.py compile <tree> <outdir> k_mod.hip k_mod11n.hip ...   # sora_amd.build's FLAGS plus --cuda-device-only -S, one .s per source
    python tools/isa_compare.py table <parent_dir> <branch_dir> [--json out.json]    # the per-kernel table

Per kernel: the instruction lines between its label and its .Lfunc_end (comments dropped, basic-block labels renumbered), how many of them lie inside a loop (a natural loop of the
control-flow graph: block layout alone can branch backwards), and vgpr_count / sgpr_count / group_segment_fixed_size / private_segment_fixed_size / the spill counts from the code-object
metadata the assembly ends with."""
import json
import os
import re
import subprocess
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def compile_tree(tree, outdir, sources):
    from sora_amd.build import FLAGS, hipcc
    os.makedirs(outdir, exist_ok=True)
    procs = [subprocess.Popen([hipcc()] + FLAGS + ["--cuda-device-only", "-S", os.path.join(tree, "sora_amd", "csrc", s), "-o",
                                                   os.path.join(outdir, os.path.splitext(s)[0] + ".s")], stderr=subprocess.DEVNULL) for s in sources]
    if any(p.wait() for p in procs):
        raise SystemExit("hipcc failed")


def loop_members(lines, labels):
    """The indices of the instructions that lie in a natural loop of the kernel's control-flow graph: basic blocks from the labels and the branches, dominators by
    iteration, a back edge u -> v where v dominates u, the loop's body what reaches u without passing v."""
    starts = sorted(set([0] + list(labels.values()) + [i + 1 for i, ln in enumerate(lines) if re.match(r"s_c?branch|s_endpgm", ln)]))
    starts = [x for x in starts if x < len(lines)]
    block_of = {x: n for n, x in enumerate(starts)}
    ends = starts[1:] + [len(lines)]
    succ = []
    for n, (a, b) in enumerate(zip(starts, ends)):
        last, out = lines[b - 1], []
        br = re.match(r"s_c?branch\w*\s+(\.LBB\d+_\d+)$", last)
        if br and labels[br.group(1)] in block_of:
            out.append(block_of[labels[br.group(1)]])
        if not last.startswith(("s_branch", "s_endpgm")) and n + 1 < len(starts):
            out.append(n + 1)
        succ.append(out)
    pred = [[] for _ in starts]
    for n, out in enumerate(succ):
        for m in out:
            pred[m].append(n)
    everything = set(range(len(starts)))
    dom = [everything] * len(starts)
    dom[0] = {0}
    changed = True
    while changed:
        changed = False
        for n in range(1, len(starts)):
            new = {n} | (set.intersection(*[dom[q] for q in pred[n]]) if pred[n] else set())
            if new != dom[n]:
                dom[n], changed = new, True
    inside = set()
    for u, out in enumerate(succ):
        for v in out:
            if v in dom[u]:
                body, work = {v, u}, [u] if u != v else []
                while work:
                    for q in pred[work.pop()]:
                        if q not in body:
                            body.add(q); work.append(q)
                inside |= body
    return [i for n in inside for i in range(starts[n], ends[n])]


def kernels(path):
    """{kernel symbol: {"insts": [...], "in_loop": n, metadata fields}} of one .s file"""
    text = open(path).read()
    meta = {}
    for m in re.finditer(r"^  - \.agpr_count:.*?(?=^  - \.agpr_count:|^amdhsa\.target)", text, re.S | re.M):
        f = dict(re.findall(r"^\s+\.(\w+):\s+(\S+)$", m.group(0), re.M))
        meta[f["name"]] = {k: int(f.get(k, 0)) for k in ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count")}
    out = {}
    for name, md in meta.items():
        body = re.search(r"^%s:[^\n]*\n(.*?)^\.Lfunc_end\d+:" % re.escape(name), text, re.S | re.M).group(1)
        lines, labels = [], {}
        for ln in body.splitlines():
            ln = ln.split(";")[0].strip()
            lab = re.match(r"^(\.LBB\d+_\d+):", ln)
            if lab:
                labels[lab.group(1)] = len(lines)
            elif ln and not ln.startswith("."):
                lines.append(ln)
        out[name] = dict(md, insts=[re.sub(r"\.LBB\d+_", ".LBB_", ln) for ln in lines], in_loop=len(loop_members(lines, labels)))
    return out


def table(parent_dir, branch_dir):
    rows = []
    for f in sorted(os.listdir(parent_dir)):
        if not f.endswith(".s"):
            continue
        p, b = kernels(os.path.join(parent_dir, f)), kernels(os.path.join(branch_dir, f))
        for name in sorted(set(p) | set(b)):
            x, y = p.get(name), b.get(name)
            row = {"file": f[:-2], "kernel": subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip().split("(")[0]}
            for tag, k in (("parent", x), ("branch", y)):
                row[tag] = None if k is None else {"insts": len(k["insts"]), "in_loop": k["in_loop"], "vgprs": k["vgpr_count"], "sgprs": k["sgpr_count"],
                                                   "lds": k["group_segment_fixed_size"], "scratch": k["private_segment_fixed_size"],
                                                   "spills": k["vgpr_spill_count"] + k["sgpr_spill_count"]}
            row["identical"] = x is not None and y is not None and x["insts"] == y["insts"]
            rows.append(row)
    return rows


if __name__ == "__main__":
    if sys.argv[1] == "compile":
        compile_tree(sys.argv[2], sys.argv[3], sys.argv[4:])
    else:
        rows = table(sys.argv[2], sys.argv[3])
        if "--json" in sys.argv:
            with open(sys.argv[sys.argv.index("--json") + 1], "w") as fh:
                json.dump(rows, fh, indent=1)
        print("%-16s %-44s %14s %12s %9s %9s %13s  %s" % ("file", "kernel", "insts p/b", "in loop p/b", "vgpr p/b", "sgpr p/b", "lds p/b", "same"))
        for r in rows:
            p, b = r["parent"] or {}, r["branch"] or {}
            g = lambda k: "%s/%s" % (p.get(k, "-"), b.get(k, "-"))
            print("%-16s %-44s %14s %12s %9s %9s %13s  %s" % (r["file"], r["kernel"], g("insts"), g("in_loop"), g("vgprs"), g("sgprs"), g("lds"), "=" if r["identical"] else "DIFF"))
        bad = [r for r in rows if r["branch"] and (r["branch"]["scratch"] or r["branch"]["spills"])]
        print("kernels: %d, identical: %d, with scratch or spills on the branch: %d" % (len(rows), sum(r["identical"] for r in rows), len(bad)))
