"""Static counts of the GEMM kernels' prologues: how much code stands in front of a loader wave's first LDS-DMA.

Compiles faceposegenerator_amd/csrc/idb_gemm.hip to gfx950 assembly with the Makefile's flags (no GPU needed; about ten minutes of
compiler time), splits every kernel into basic blocks, and walks the SHORTEST path — in instructions — from the kernel's entry to its
first LDS-DMA instruction (`buffer_load_dword... lds`): the path a loader wave takes.  Per kernel instance it prints

    instructions on that path | integer-division expansions on it (v_rcp_iflag_f32: one per division by a run-time value) |
    scalar loads on it / s_waitcnt instructions that wait for them (lgkmcnt) | v_rcp_iflag_f32 in the whole kernel

and the same counts on the forward path with the MOST such waits (an upper bound for every launch: the loader of a 3x3 conv of several
sources with a split, which walks the K seek and the retap, is one of the paths it covers).

    python tools/gemm_prologue_isa.py                 # compile, print the f16 instances of the lw / patch / gn / ring / pl kernels
    python tools/gemm_prologue_isa.py --asm FILE.s    # use an assembly file made earlier (hipcc ... --cuda-device-only -S)
    python tools/gemm_prologue_isa.py --dtype all --kernels 'idb_gemm_kernel_lw'
"""
import argparse
import heapq
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "faceposegenerator_amd", "csrc")
DEFAULT_KERNELS = r"^(idb_gemm_kernel_lw|idb_conv_patch_kernel|idb_gemm_kernel_gn|idb_gemm_kernel|idb_gemm_kernel_pl)<"


def hipcc():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    default = re.search(r"^HIPCC\s*\?=\s*(\S+)", mk, re.M).group(1)
    for cand in (os.environ.get("HIPCC"), default, shutil.which("hipcc")):
        if cand and os.path.isfile(cand) and os.access(cand, os.X_OK):
            return cand
    return None


def makefile_flags():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    arch = re.search(r"^ARCH\s*\?=\s*(\S+)", mk, re.M).group(1)
    flags = re.search(r"^CXXFLAGS\s*=\s*(.+)$", mk, re.M).group(1).replace("$(ARCH)", arch).split()
    pre = re.search(r"^KERNARG_PRELOAD\s*=\s*(.+)$", mk, re.M)      # what idb_gemm.o is built with beside CXXFLAGS
    return flags + (pre.group(1).split() if pre else [])


def compile_asm(out):
    cc = hipcc()
    if cc is None:
        sys.exit("hipcc not found")
    cmd = [cc] + makefile_flags() + ["--cuda-device-only", "-S", "idb_gemm.hip", "-o", out]
    p = subprocess.run(cmd, cwd=CSRC, capture_output=True, text=True)
    if p.returncode != 0:
        sys.exit(p.stderr[-3000:])


def kernels(asm):
    """{mangled symbol: [instruction or label lines]} of every kernel (symbols with an .amdhsa_kernel record)."""
    names = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M))
    out = {}
    for m in re.finditer(r"^(\w+):[^\n]*\n(.*?)^\.Lfunc_end", asm, re.M | re.S):
        if m.group(1) not in names:
            continue
        body = m.group(2)
        # A kernel with preloaded kernel arguments begins with a stub for firmware without the preload (it loads the same arguments
        # and branches to the 256-byte-aligned real entry, where the hardware starts a wave otherwise): not part of the path.
        stub = re.match(r"(?:\s*(?:;|s_load_\w+|s_waitcnt|s_nop)[^\n]*\n|\s*\n)+\s*s_branch\s+(\S+)[^\n]*\n\s*\.p2align\s+8\n", body)
        if stub:
            body = body[stub.end():]
        lines = [ln.split(";")[0].strip() for ln in body.split("\n")]
        out[m.group(1)] = [ln for ln in lines if ln and (not ln.startswith(".") or ln.endswith(":"))]
    return out


def blocks(lines):
    """Basic blocks: [(label or None, [instructions], [successor labels], falls_through)]."""
    out, cur, label = [], [], None
    for ln in lines:
        if ln.endswith(":"):
            if cur or label is not None:
                out.append([label, cur, [], True])
            label, cur = ln[:-1], []
            continue
        cur.append(ln)
        m = re.match(r"s_(c?branch)\w*\s+(\S+)$", ln)
        if m or ln.startswith("s_endpgm"):
            out.append([label, cur, [m.group(2)] if m else [], bool(m) and m.group(1) == "cbranch"])
            label, cur = None, []
    if cur or label is not None:
        out.append([label, cur, [], False])
    return out


def is_dma(ln):
    return ln.startswith("buffer_load") and re.search(r"\blds\b", ln) is not None


def _count(instrs):
    sl = sum(1 for x in instrs if x.startswith(("s_load_", "s_buffer_load_")))
    sw = sum(1 for x in instrs if x.startswith("s_waitcnt") and "lgkmcnt" in x)
    return len(instrs), sum(1 for x in instrs if x.startswith("v_rcp_iflag_f32")), sl, sw


def shortest_to_dma(lines):
    """(instructions, divisions, scalar loads, lgkm waits) on the shortest entry -> first LDS-DMA path; None if the kernel has none."""
    bl = blocks(lines)
    at = {b[0]: i for i, b in enumerate(bl) if b[0] is not None}
    best = {0: (0, 0, 0, 0)}
    heap = [(0, 0)]
    answer, target = None, None
    while heap:
        dist, i = heapq.heappop(heap)
        if dist != best[i][0]:
            continue
        label, instrs, succ, fall = bl[i]
        k = next((j for j, x in enumerate(instrs) if is_dma(x)), None)
        if k is not None:
            c = _count(instrs[:k])
            cand = tuple(a + b for a, b in zip(best[i], c))
            if answer is None or cand[0] < answer[0]:
                answer, target = cand, i
            continue
        c = _count(instrs)
        here = tuple(a + b for a, b in zip(best[i], c))
        nxt = [at[s] for s in succ if s in at] + ([i + 1] if fall and i + 1 < len(bl) else [])
        for j in nxt:
            if j not in best or here[0] < best[j][0]:
                best[j] = here
                heapq.heappush(heap, (here[0], j))
    return answer, target


def worst_to_dma(lines, target, budget):
    """(instructions, divisions, scalar loads, lgkm waits) on the path from the entry to the SAME first LDS-DMA the shortest path ends
    at (block `target`) that has the MOST waits on scalar loads (ties: most instructions), among the paths that take no backward
    branch, meet no other LDS-DMA and are at most `budget` instructions long (twice the shortest path: the structurised control flow
    also holds forward paths through another role's whole K loop and epilogue, which no wave takes).  An upper bound for every launch
    of that role — a 3x3 conv of several sources with a split, whose loader walks every arm of the K seek and the retap, included."""
    bl = blocks(lines)
    at = {b[0]: i for i, b in enumerate(bl) if b[0] is not None}
    state = {0: {0: (0, 0, 0, 0)}}      # block -> {instructions so far: counts with the most waits}
    best = None
    for i in range(len(bl)):            # forward edges only: blocks in layout order
        if i not in state:
            continue
        label, instrs, succ, fall = bl[i]
        k = next((j for j, x in enumerate(instrs) if is_dma(x)), None)
        c = _count(instrs[:k]) if k is not None else _count(instrs)
        for n, t in state[i].items():
            here = tuple(a + b for a, b in zip(t, c))
            if here[0] > budget:
                continue
            if k is not None:
                if i == target and (best is None or (here[3], here[0]) > (best[3], best[0])):
                    best = here
                continue
            for j in [at[x] for x in succ if x in at] + ([i + 1] if fall and i + 1 < len(bl) else []):
                if j <= i:
                    continue
                d = state.setdefault(j, {})
                if here[0] not in d or here[3] > d[here[0]][3]:
                    d[here[0]] = here
    return best


def demangle(names):
    """_Z18idb_gemm_kernel_lwIDF16_Li1ELi2ELi4ELi4ELi4EEv10GemmParams -> idb_gemm_kernel_lw<f16,1,2,4,4,4> (the forms these kernels use)."""
    out = {}
    for n in names:
        m = re.match(r"_Z(\d+)", n)
        if not m:
            out[n] = n
            continue
        k = int(m.group(1))
        base, rest = n[m.end():m.end() + k], n[m.end() + k:]
        args = []
        if rest.startswith("I"):
            for t in re.finditer(r"DF16_|DF16b|Li(\d+)E|Lb([01])E|E", rest[1:]):
                if t.group(0) == "E":
                    break
                args.append("f16" if t.group(0) == "DF16_" else "bf16" if t.group(0) == "DF16b" else t.group(1) if t.group(1) is not None
                            else ("true" if t.group(2) == "1" else "false"))
        out[n] = base + ("<" + ",".join(args) + ">" if args else "")
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--asm", help="assembly file to read instead of compiling")
    ap.add_argument("--save-asm", help="keep the compiled assembly in this file")
    ap.add_argument("--dtype", choices=["f16", "bf16", "all"], default="f16")
    ap.add_argument("--kernels", default=DEFAULT_KERNELS, help="regular expression over the demangled kernel names")
    a = ap.parse_args()
    if a.asm:
        asm = open(a.asm).read()
    else:
        with tempfile.TemporaryDirectory() as td:
            out = os.path.join(td, "idb_gemm.s")
            compile_asm(out)
            asm = open(out).read()
            if a.save_asm:
                shutil.copyfile(out, a.save_asm)
    ks = kernels(asm)
    pretty = demangle(sorted(ks))
    want = {"f16": "<f16,", "bf16": "<bf16,"}.get(a.dtype)
    rows = []
    for sym in sorted(ks, key=lambda s: pretty[s]):
        name = pretty[sym]
        if not re.search(a.kernels, name) or (want and want not in name):
            continue
        r, target = shortest_to_dma(ks[sym])
        w = worst_to_dma(ks[sym], target, 2 * r[0]) if r is not None else None
        total_rcp = sum(1 for x in ks[sym] if x.startswith("v_rcp_iflag_f32"))
        rows.append((name, r, w, total_rcp))
    print(f"{'':64s} {'shortest path':>24s} | {'most waits (<= 2x instr)':>24s} |")
    print(f"{'kernel':64s} {'instr':>6s} {'div':>4s} {'s_load/wait':>12s} | {'instr':>6s} {'div':>4s} {'s_load/wait':>12s} | {'div(all)':>9s}")
    for name, r, w, total_rcp in rows:
        cols = ""
        for x in (r, w):
            if x is None:
                cols += f" {'-':>6s} {'-':>4s} {'-':>12s} |"
            else:
                cols += f" {x[0]:6d} {x[1]:4d} {str(x[2]) + ' / ' + str(x[3]):>12s} |"
        print(f"{name:64s}{cols} {total_rcp:9d}")


if __name__ == "__main__":
    main()
