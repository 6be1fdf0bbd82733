"""Every case x input recipe of the idb_attention test matrix (tests/attn_matrix.py) on the device, both dtypes, against a float64
reference computed on the device from the same operand-dtype-rounded inputs, element by element.

lib.idb_attention is called directly (the engine's wrapper fixes scale, out_ld and the K/V allocation).  Every launch: the output
buffer and its guard rows and padding columns hold a canary bit pattern (a NaN in both dtypes) beforehand, so an unwritten element fails
and a write outside the ABI's output is seen; the row padding of Q, K and V holds NaN and K/V rows n_kv .. n_kv_alloc-1 hold zeros,
NaN or the largest finite value; the case's criterion (attn_matrix.bound, or bit-equality for const_v / one_hot) is asserted on every
element; idb_attention_plan must report the form the case was chosen for.  Also: the same launch twice is bit-identical (the kernel has
no atomics: any difference is a race), and a launch captured in a torch.cuda.graph on one stream replays to the eager bits.

One process, default environment: IDB_ATTN_KSPLIT = 0 / 2 are measurement switches read once per process and are not covered.

Worst err / bound measured on MI355X (test_form_summary prints one line per dtype and form; recorded for the next reader, not used
as thresholds):
    form       bf16                            f16
    2-wave     0.875 (w2_causal64/count)       0.843 (w2_causal128/count)
    4-wave     0.992 (w4_causal300/count)      0.966 (w4_causal600_long/count)
    8-wave     0.889 (w8_nkv544/count)         0.677 (w8_scale2/normal)
    12-wave    0.889 (w12_nkv544/count)        0.689 (w12_scale2/normal)
per recipe: count 0.992 / 0.966 (the output rounding alone), normal 0.890 / 0.805, peaked 0.497 / 0.461, wide_range 0.849 / 0.653; every
const_v and one_hot element was bit-exact.  All of C_O, C_P, C_A stay 1.  276 launches per dtype; the whole file runs in about 21 s on
one MI355X."""
import os
import sys
from collections import defaultdict

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_matrix as AM  # noqa: E402
import matrix_common as MC  # noqa: E402
from faceposegenerator_amd import _lib as L  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = ("bf16", "f16")
FORMS = (2, 4, 8, 12)

_SUMMARY = defaultdict(lambda: [0, 0.0, ""])       # (dtype, form) -> [launches, worst ratio, where]


def _run(lib, case, recipe, dtype):
    """Launch one (case, recipe, dtype); returns (out [batch][heads][n_q][64], inputs on the device, packed buffers)."""
    inp = AM.make_inputs(case, recipe, dtype)
    pk = AM.pack(case, inp, dtype, DEV)
    L.check(AM.launch(lib, case, pk, dtype, MC.stream()), f"idb_attention {case.name}")
    torch.cuda.synchronize()
    out, touched = AM.unpack_out(case, pk, dtype)
    assert touched == 0, f"{case.name} {dtype} {recipe}: {touched} elements outside the output lost their canary"
    return out, inp, pk


def _reference(case, inp):
    """float64 on the device, one batch entry at a time (the 4096-token cases hold 84M scores per entry)."""
    refs = [AM.reference(inp.q[b:b + 1].to(DEV), inp.k[b:b + 1].to(DEV), inp.v[b:b + 1].to(DEV), case.n_kv, case.scale, case.causal)
            for b in range(case.batch)]
    return AM.Ref(torch.cat([r.ref for r in refs]), torch.cat([r.absref for r in refs]), torch.cat([r.l for r in refs]),
                  max(r.vmax for r in refs))


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_matrix(lib, dtype, form):
    cases = [c for c in AM.cases(lib) if c.waves == form]
    assert cases
    failures = []
    for case in cases:
        assert AM.case_plan(lib, case)[0] == form, f"{case.name}: the plan no longer reports the {form}-wave form"
        for recipe in case.recipes:
            out, inp, _ = _run(lib, case, recipe, dtype)
            r = _reference(case, inp)
            ok, ratio, nbad = AM.check(out, AM.expected(inp, r, recipe), AM.bound(r, case.n_kv, dtype, recipe))
            print(f"{dtype} w{form} {case.name:28s} {recipe:10s} worst err/bound {ratio:.3f} bad {nbad}")
            s = _SUMMARY[dtype, form]
            s[0] += 1
            if recipe not in AM.EXACT and ratio > s[1]:
                s[1], s[2] = ratio, f"{case.name}/{recipe}"
            if not ok:
                failures.append(f"{case.name}/{recipe}: {nbad} of {out.numel()} elements beyond the criterion or not finite, worst ratio {ratio:.3g}")
    assert not failures, f"{dtype}, {form}-wave form:\n" + "\n".join(failures)


@pytest.mark.parametrize("dtype", DTYPES)
def test_relaunch_is_bit_identical(lib, dtype):
    by_name = {c.name: c for c in AM.cases(lib)}
    for name in ("w2_nkv77", "w4_causal300", "w8_nkv545", "w12_nq1600"):
        case = by_name[name]
        inp = AM.make_inputs(case, "normal", dtype)
        outs = []
        for _ in range(2):
            pk = AM.pack(case, inp, dtype, DEV)
            L.check(AM.launch(lib, case, pk, dtype, MC.stream()), name)
            torch.cuda.synchronize()
            outs.append(pk.obuf.clone())
        assert torch.equal(outs[0], outs[1]), f"{name} {dtype}: two launches on the same inputs differ"


@pytest.mark.parametrize("dtype", DTYPES)
def test_graph_replay_equals_eager(lib, dtype):
    """One launch captured on a single stream (one branch), replayed into a canary-refilled buffer."""
    case = {c.name: c for c in AM.cases(lib)}["w8_nkv545"]
    inp = AM.make_inputs(case, "normal", dtype)
    pk = AM.pack(case, inp, dtype, DEV)
    L.check(AM.launch(lib, case, pk, dtype, MC.stream()), "eager")
    torch.cuda.synchronize()
    eager = pk.obuf.clone()
    pk.obuf.fill_(AM.CANARY)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        L.check(AM.launch(lib, case, pk, dtype, MC.stream()), "capture")
    pk.obuf.fill_(AM.CANARY)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(pk.obuf, eager), f"{dtype}: the replayed graph differs from the eager launch"
    assert (eager != AM.CANARY).any()


def test_form_summary(lib):
    """One line per (dtype, form) of what test_matrix launched in this process (nothing to report when it did not run)."""
    print()
    for dtype in DTYPES:
        for form in FORMS:
            n, worst, where = _SUMMARY[dtype, form]
            print(f"attention matrix {dtype:4s} {form:2d}-wave form: {n:3d} launches, worst err / bound {worst:.3f} ({where})")
