#!/usr/bin/env python3
"""Static instruction mix of the loops of one kernel in libcc_hip.so's gfx950 device assembly (CPU only).

Compiles cc_engine.hip for gfx950 with build.py's flags (device side only, -S) unless an assembly file is given, splits the kernel's body into
basic blocks, builds the control-flow graph from the branches and finds its loops as strongly connected components (LLVM's own loop comments
miss loops the structurizer left with several entries, such as k_insert_par's firing loop). Per loop (nested loops included) it prints the
instruction classes: vector ALU, scalar ALU, SGPR spill traffic (v_writelane / v_readlane), divergent-branch bookkeeping (s_and_saveexec,
s_cbranch_execz), IEEE f32 divisions (v_div_scale_f32: two per division), square roots, memory, waits and s_nop. Counts are over the loop's
code, every path once: an iteration executes less where it branches (a rare path moved out of line stays in the count; executed counts come from
SQ_INSTS_VALU / SQ_INSTS_SALU). In k_insert_par<1, 8> the loop with the most vector stores is phase D (one firing per iteration); the
largest one is phase 0 (one firing per lane).

usage: python tools/asm_mix.py [--asm FILE.s] [--kernel SUBSTRING_OF_MANGLED_NAME] [--min 40] [-D MACRO ...]
"""
from __future__ import annotations

import argparse
import os
import re
import subprocess
import sys
import tempfile
from collections import Counter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "continuous_clustering_amd", "csrc")
sys.path.insert(0, ROOT)
from continuous_clustering_amd import build as hip_build  # noqa: E402

DEFAULT_KERNEL = "k_insert_parILi1ELi8E"  # k_insert_par<1, 8>: the launch of more than 160 streams

CLASSES = ["valu", "salu", "v_writelane", "v_readlane", "v_readfirstlane", "s_and_saveexec", "s_cbranch_execz", "v_div_scale_f32", "v_sqrt",
           "vmem_load", "vmem_store", "vmem_atomic", "smem", "lds", "s_waitcnt", "s_nop", "branch"]
SHORT = {"v_readfirstlane": "readfirst", "s_and_saveexec": "saveexec", "s_cbranch_execz": "execz", "v_div_scale_f32": "div_scale",
         "v_writelane": "writelane", "v_readlane": "readlane", "vmem_atomic": "vmem_atom", "vmem_load": "vmem_ld", "vmem_store": "vmem_st"}


def compile_asm(defines: list[str]) -> str:
    flags = [f for f in hip_build.HIPCC_FLAGS if f not in ("-shared", "-ldl")]
    out = os.path.join(tempfile.mkdtemp(prefix="asm_mix_"), "cc_engine.s")
    cmd = [hip_build.hipcc(), *flags, *[f"-D{d}" for d in defines], "--cuda-device-only", "-S", "-o", out, os.path.join(CSRC, "cc_engine.hip")]
    subprocess.check_call(cmd, cwd=CSRC)
    return out


def classify(op: str) -> list[str]:
    c = [name for name in ("v_writelane", "v_readlane", "v_readfirstlane", "v_div_scale_f32", "v_sqrt") if op.startswith(name)]
    if op.startswith("v_"):
        c.append("valu")
    elif op.startswith(("global_load", "buffer_load", "flat_load")):
        c.append("vmem_load")
    elif op.startswith(("global_store", "buffer_store", "flat_store")):
        c.append("vmem_store")
    elif op.startswith(("global_atomic", "buffer_atomic", "flat_atomic")):
        c.append("vmem_atomic")
    elif op.startswith(("s_load", "s_buffer_load")):
        c.append("smem")
    elif op.startswith("ds_"):
        c.append("lds")
    elif op.startswith("s_waitcnt"):
        c.append("s_waitcnt")
    elif op == "s_nop":
        c.append("s_nop")
    elif op.startswith(("s_branch", "s_cbranch", "s_setpc", "s_endpgm")):
        c.append("branch")
        if op == "s_cbranch_execz":
            c.append("s_cbranch_execz")
    elif op.startswith("s_"):
        c.append("salu")
        if op.startswith("s_and_saveexec"):
            c.append("s_and_saveexec")
    return c


def parse(asm_path: str, kernel: str):
    """-> kernel name, block labels, per-block Counters, successor lists"""
    lines = open(asm_path).read().splitlines()
    start = name = None
    for i, ln in enumerate(lines):
        m = re.match(r"^(_Z\S+):", ln)
        if m and kernel in m.group(1):
            start, name = i, m.group(1)
            break
    if start is None:
        raise SystemExit(f"kernel matching {kernel!r} not found in {asm_path}")
    labels, counts, targets, falls = ["entry"], [Counter()], [[]], [True]
    for ln in lines[start + 1:]:
        if ln.startswith(".Lfunc_end"):
            break
        s = ln.split(";")[0].strip()
        m = re.match(r"^\.L(BB\d+_\d+):", s)
        if not m and not s:
            m = re.match(r"^; %bb\.(\d+):", ln.strip())
        if m:
            labels.append(m.group(1))
            counts.append(Counter())
            targets.append([])
            falls.append(True)
            continue
        if not s or s.startswith("."):
            continue
        op = s.split()[0]
        for c in classify(op):
            counts[-1][c] += 1
        counts[-1]["total"] += 1
        if op.startswith(("s_branch", "s_cbranch")):
            t = re.search(r"\.L(BB\d+_\d+)", s)
            if t:
                targets[-1].append(t.group(1))
            if op == "s_branch":
                falls[-1] = False
        elif op in ("s_endpgm", "s_setpc_b64"):
            falls[-1] = False
    index = {lab: i for i, lab in enumerate(labels)}
    succ = []
    for i in range(len(labels)):
        s = [index[t] for t in targets[i] if t in index]
        if falls[i] and i + 1 < len(labels):
            s.append(i + 1)
        succ.append(s)
    return name, labels, counts, succ


def sccs(succ):
    """Tarjan's strongly connected components (iterative); only the cyclic ones are returned"""
    n = len(succ)
    index, low, on, stack, out = [-1] * n, [0] * n, [False] * n, [], []
    counter = 0
    for root in range(n):
        if index[root] >= 0:
            continue
        work = [(root, 0)]
        index[root] = low[root] = counter
        counter += 1
        stack.append(root)
        on[root] = True
        while work:
            v, i = work[-1]
            if i < len(succ[v]):
                work[-1] = (v, i + 1)
                w = succ[v][i]
                if index[w] < 0:
                    index[w] = low[w] = counter
                    counter += 1
                    stack.append(w)
                    on[w] = True
                    work.append((w, 0))
                elif on[w]:
                    low[v] = min(low[v], index[w])
                continue
            work.pop()
            if work:
                low[work[-1][0]] = min(low[work[-1][0]], low[v])
            if low[v] == index[v]:
                comp = []
                while True:
                    w = stack.pop()
                    on[w] = False
                    comp.append(w)
                    if w == v:
                        break
                if len(comp) > 1 or v in succ[v]:
                    out.append(sorted(comp))
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--asm", help="assembly file (default: compile cc_engine.hip with build.py's flags)")
    ap.add_argument("--kernel", default=DEFAULT_KERNEL)
    ap.add_argument("--min", type=int, default=40, help="list loops of at least this many instructions")
    ap.add_argument("-D", dest="defines", action="append", default=[], help="extra macro for the compile")
    a = ap.parse_args()
    path = a.asm or compile_asm(a.defines)
    name, labels, counts, succ = parse(path, a.kernel)
    whole = Counter()
    for c in counts:
        whole.update(c)
    rows = []
    for comp in sccs(succ):
        cnt = Counter()
        for b in comp:
            cnt.update(counts[b])
        if cnt["total"] >= a.min:
            rows.append((f"loop at {labels[comp[0]]} ({len(comp)} blocks)", cnt))
    rows.sort(key=lambda r: -r[1]["total"])
    stores = max(rows, key=lambda r: r[1]["vmem_store"]) if rows else None
    print(f"# {name}")
    print("# static instruction counts (every path of the code once); loops = cycles of the control-flow graph, inner loops included")
    print(f"{'code':<32}" + "".join(f"{SHORT.get(c, c):>10}" for c in ["total"] + CLASSES))
    for label, cnt in [("whole kernel", whole)] + rows:
        print(f"{label:<32}" + "".join(f"{cnt[c]:>10}" for c in ["total"] + CLASSES))
    if stores:
        print(f"# the loop with the most vector stores: {stores[0]}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
