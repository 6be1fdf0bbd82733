"""Every case x recipe of the training-attention matrix (tests/attn_bwd_matrix.py) and every idb_lora_grad case on the device, both
dtypes, element by element against the float64 reference.

Forward: idb_attention_fwd_train's `out` meets attn_matrix.bound (the forward matrix's own criterion, imported unchanged) and `lse` meets
lse_bound.  Backward: idb_attention_bwd is handed the REFERENCE's out (rounded to T) and lse (rounded to fp32), so its criteria do not
depend on the forward kernel; the gradients land in NaN-filled buffers between NaN guards, every element outside the ABI's outputs (row
padding, rows n_kv .. n_kv_alloc-1 of dk / dv, the workspace's guards) must keep its NaN, the K/V padding rows hold NaN or the largest
finite value, and a second run must be bit-equal.  The plan's form is asserted per case.

Worst err / bound measured on MI355X, bf16 / f16 (test_summary prints them; recorded for the next reader, never used as thresholds):
    normal    out 0.658 / 0.683  lse 0.170 / 0.156  dQ 0.453 / 0.484  dK 0.679 / 0.836  dV 0.923 / 0.853
    peaked    out 0.601 / 0.545  lse 0.254 / 0.258  dQ 0.321 / 0.309  dK 0.396 / 0.408  dV 0.867 / 0.646
    count     out 0.206 / 0.209  lse 0.381 / 0.381  dQ 0.326 / 0.332  dK exactly 0      dV 0.235 / 0.280 (exact where n_kv is a power of two)
    ones_dout out 0.280 / 0.312  lse 0.067 / 0.041  dQ 0.117 / 0.201  dK 0.748 / 0.848  dV 0.966 / 0.876
    one_hot   every element of out, lse, dQ, dK and dV exact
    chained (the backward on the forward kernel's own out and lse, twice the criterion): dQ 0.186 / 0.173, dK 0.290 / 0.272, dV 0.245 / 0.246
    idb_lora_grad: 0.033 / 0.041 of its worst-case bound; the integer cases exact; da exactly 0 with B = 0
The whole file runs in about 3 s on one MI355X."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_bwd_matrix as BM  # noqa: E402
import matrix_common as MC  # noqa: E402
from faceposegenerator_amd import _lib as L  # noqa: E402

pytestmark = pytest.mark.gpu
DTYPES = ("bf16", "f16")
_WORST = MC.Worst("training attention")
_REFS = {}


def _setup(case, recipe, dtype):
    key = (case.name, recipe, dtype)
    if key not in _REFS:
        inp = BM.make_inputs(case, recipe, dtype)
        _REFS[key] = (inp, BM.reference(inp, case))
    return _REFS[key]


@pytest.mark.parametrize("dtype", DTYPES)
def test_forward_matrix(lib, dtype):
    failures = []
    for case in BM.cases(lib):
        for recipe in case.recipes:
            inp, r = _setup(case, recipe, dtype)
            d = BM.Device(case, inp, dtype)
            L.check(d.forward(lib), f"idb_attention_fwd_train {case.name}")
            torch.cuda.synchronize()
            out, lse = d.forward_results()
            want_out, bnd_out = BM.forward_criterion(inp, r, case.n_kv, dtype)
            for name, got, want, bnd in (("out", out, want_out, bnd_out), ("lse", lse, r.lse, BM.lse_bound(r, case.n_kv))):
                ok, ratio, nbad = MC.check_t(got, want, bnd)
                _WORST.note(f"forward {name} {recipe:9s} {dtype}", ratio, case.name)
                if not ok:
                    failures.append(f"{case.name}/{recipe}/{name}: {nbad} elements beyond the criterion or not finite, worst ratio {ratio:.3g}")
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("dtype", DTYPES)
def test_backward_matrix(lib, dtype):
    failures = []
    for case in BM.cases(lib):
        assert BM.case_plan(lib, case)[0] == case.form, f"{case.name}: the plan no longer reports form {case.form}"
        for recipe in case.recipes:
            inp, r = _setup(case, recipe, dtype)
            out_t, lse32 = BM.saved(r, dtype)
            d = BM.Device(case, inp, dtype)
            before = lib.idb_launch_count()
            L.check(d.backward(lib, out_t, lse32), f"idb_attention_bwd {case.name}")
            assert lib.idb_launch_count() - before == BM.case_plan(lib, case)[3]
            torch.cuda.synchronize()
            got, raws = d.gradients()
            exp, bnd = BM.expected(inp, r, case, recipe, dtype), BM.bound(inp, r, case, recipe, dtype)
            for name in ("dq", "dk", "dv"):
                ok, ratio, nbad = MC.check_t(got[name], exp[name], bnd[name])
                print(f"{dtype} {case.name:30s} {recipe:9s} {name} worst err/bound {ratio:.3f} bad {nbad}")
                _WORST.note(f"backward {name} {recipe:9s} {dtype}", ratio, case.name)
                if not ok:
                    failures.append(f"{case.name}/{recipe}/{name}: {nbad} elements beyond the criterion or not finite, worst ratio {ratio:.3g}")
            # the same call again, into fresh buffers: bit-equal (no atomics, no order left to chance)
            d2 = BM.Device(case, inp, dtype)
            L.check(d2.backward(lib, out_t, lse32), "second run")
            torch.cuda.synchronize()
            for a, b in zip(raws, d2.gradients()[1]):
                MC.same_bits(f"{case.name}/{recipe}: second run", b, a)
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("dtype", DTYPES)
def test_backward_on_the_forward_kernels_own_results(lib, dtype):
    """The two kernels chained as the layer chains them (out and lse from idb_attention_fwd_train): the same criteria hold, because
    the forward's out is the reference's within its rounding and its lse within lse_bound, which the delta and E_P terms cover."""
    for case in (c for c in BM.cases(lib) if c.name in ("cross77_nan", "packed_self", "kb_three_ragged")):
        inp, r = _setup(case, "normal", dtype)
        d = BM.Device(case, inp, dtype)
        L.check(d.forward(lib), "forward")
        torch.cuda.synchronize()
        out, lse = d.forward_results()
        L.check(d.backward(lib, out, lse), "backward")
        torch.cuda.synchronize()
        got, _ = d.gradients()
        bnd = BM.bound(inp, r, case, "normal", dtype)
        for name, want in (("dq", r.dq), ("dk", r.dk), ("dv", r.dv)):
            # out differs from round_T(ref) by at most one more rounding: the delta term doubles, nothing else moves
            ok, ratio, nbad = MC.check_t(got[name], want, 2 * bnd[name])
            _WORST.note(f"chained {name} normal    {dtype}", ratio, case.name)
            assert ok, f"{case.name}/{name}: {nbad} beyond twice the criterion, worst {ratio:.3g}"


@pytest.mark.parametrize("dtype", DTYPES)
def test_lora_grad_matrix(lib, dtype):
    for case in BM.lora_cases():
        x, dy, a, b = BM.lora_inputs(case, dtype)
        da, db, bda, bdb = BM.lora_reference(case, x, dy, a, b)
        d = BM.LoraDevice(case, x, dy, a, b, dtype)
        before = lib.idb_launch_count()
        L.check(d.run(lib), f"idb_lora_grad {case.name}")
        assert lib.idb_launch_count() - before == 3
        torch.cuda.synchronize()
        gda, gdb, raw_a, raw_b = d.results()
        for name, got, want, bnd in (("da", gda, da, bda), ("db", gdb, db, bdb)):
            ok, ratio, nbad = MC.check_t(got, want, bnd)
            print(f"{dtype} lora_grad {case.name:14s} {name} worst err/bound {ratio:.3f} bad {nbad}")
            _WORST.note(f"lora_grad {name} {case.recipe:8s} {dtype}", ratio, case.name)
            assert ok, f"{case.name}/{name}: {nbad} elements beyond the bound, worst ratio {ratio:.3g}"
        if case.recipe == "b_zero":
            assert not gda.any() and gdb.abs().max() > 0
        L.check(d.run(lib), "second run")
        torch.cuda.synchronize()
        _, _, raw_a2, raw_b2 = d.results()
        MC.same_bits(f"{case.name}: da, second run", raw_a2, raw_a)
        MC.same_bits(f"{case.name}: db, second run", raw_b2, raw_b)


def test_summary(lib):
    print()
    _WORST.show()
