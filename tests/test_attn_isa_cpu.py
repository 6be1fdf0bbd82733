"""The attention kernels' tile loop must not wait on vector-memory loads before its MFMAs (needs hipcc, no GPU).

Every attn_kernel instance prefetches the next K/V tile into registers at the top of the tile loop and writes it to LDS after the
tile's last PV MFMA.  A `s_waitcnt vmcnt(..)` between those loads and the loop's first MFMA makes every wave sit out the round
trip of the prefetch on every tile; results are identical with it, so nothing else notices.  (The Q-fragment loads of the
prologue once put four such waits there.)  This compiles idb_attn.hip to assembly with the Makefile's flags and looks at nothing
but wait counters, global loads, LDS writes and MFMAs."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "faceposegenerator_amd", "csrc")


def _hipcc():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    default = re.search(r"^HIPCC\s*\?=\s*(\S+)", mk, re.M).group(1)
    for cand in (os.environ.get("HIPCC"), default, shutil.which("hipcc")):
        if cand and os.path.isfile(cand) and os.access(cand, os.X_OK):
            return cand
    return None


def _makefile_flags():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    arch = re.search(r"^ARCH\s*\?=\s*(\S+)", mk, re.M).group(1)
    cxx = re.search(r"^CXXFLAGS\s*=\s*(.+)$", mk, re.M).group(1).replace("$(ARCH)", arch)
    extra = re.search(r"^idb_attn\.o:\s*EXTRA\s*=\s*(.+)$", mk, re.M).group(1)
    return cxx.split() + extra.split()


@pytest.fixture(scope="module")
def attn_asm(tmp_path_factory):
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("hipcc not found")
    out = tmp_path_factory.mktemp("attn_isa") / "idb_attn.s"
    cmd = [hipcc] + _makefile_flags() + ["--cuda-device-only", "-S", "idb_attn.hip", "-o", str(out)]
    p = subprocess.run(cmd, cwd=CSRC, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    return out.read_text()


def kernels(asm):
    """{symbol: [instruction or label lines]} of every attn_kernel instance."""
    out = {}
    for m in re.finditer(r"^(_Z\w*attn_kernel\w*):[^\n]*\n(.*?)^\.Lfunc_end", asm, re.M | re.S):
        lines = [ln.split(";")[0].strip() for ln in m.group(2).split("\n")]
        out[m.group(1)] = [ln for ln in lines if ln and (not ln.startswith(".") or ln.endswith(":"))]
    return out


def tile_loops(lines):
    """Innermost loops (label ... backward branch to it) that hold an MFMA: the instruction lists of their bodies."""
    label_at = {ln[:-1]: i for i, ln in enumerate(lines) if ln.endswith(":")}
    spans = []
    for i, ln in enumerate(lines):
        m = re.match(r"s_c?branch\w*\s+(\S+)$", ln)
        if m and label_at.get(m.group(1), i) < i:
            spans.append((label_at[m.group(1)], i))
    inner = [s for s in spans if not any(o != s and s[0] <= o[0] and o[1] <= s[1] for o in spans)]
    bodies = [[ln for ln in lines[a:b] if not ln.endswith(":")] for a, b in inner]
    return [b for b in bodies if any(ln.startswith("v_mfma") for ln in b)]


def _is_vm_wait(ln):
    return ln.startswith("s_waitcnt") and "vmcnt" in ln


def check_kernel(name, lines):
    """The list of violations of one kernel; also the number of prefetching tile loops found."""
    bad, prefetching = [], 0
    for n, body in enumerate(tile_loops(lines)):
        loads = [i for i, ln in enumerate(body) if ln.startswith("global_load")]
        if loads:
            prefetching += 1
            rot = body[loads[0]:] + body[:loads[0]]          # the loop seen from its first prefetch load
            first_mfma = next(i for i, ln in enumerate(rot) if ln.startswith("v_mfma"))
            for ln in rot[:first_mfma]:
                if _is_vm_wait(ln):
                    bad.append(f"{name} loop {n}: '{ln}' between the prefetch loads and the first MFMA")
        for i, ln in enumerate(body):
            if not _is_vm_wait(ln):
                continue
            nxt = next((x for x in body[i + 1:] if x.startswith(("ds_write", "v_mfma", "global_load"))), "end of loop")
            if not nxt.startswith("ds_write"):
                bad.append(f"{name} loop {n}: '{ln}' is followed by '{nxt.split()[0]}', not by a ds_write")
    return bad, prefetching


def test_parser_sees_the_stall_in_a_synthetic_loop():
    good = ["x:", ".LBB0_1:", "global_load_dwordx4 v[0:3], v[8:9], off", "s_waitcnt lgkmcnt(0)", "v_mfma_f32_32x32x16_f16 a, b, c, 0",
            "s_waitcnt vmcnt(0)", "ds_write_b128 v1, v[0:3]", "s_barrier", "s_cbranch_scc1 .LBB0_1"]
    assert check_kernel("k", good) == ([], 1)
    stalled = list(good)
    stalled[3] = "s_waitcnt vmcnt(0) lgkmcnt(0)"
    bad, n = check_kernel("k", stalled)
    assert n == 1 and len(bad) == 2, bad


def test_no_vmcnt_wait_between_prefetch_and_first_mfma(attn_asm):
    ks = kernels(attn_asm)
    # 2-, 4-, 8- and 12-wave forms x {bf16, f16}
    assert len(ks) == 8, sorted(ks)
    bad = []
    for name, lines in sorted(ks.items()):
        b, prefetching = check_kernel(name, lines)
        assert prefetching >= 1, f"{name}: no tile loop with prefetch loads and MFMAs found"
        bad += b
    assert not bad, "\n".join(bad)
