"""The CPU half of the training-attention matrix (tests/attn_bwd_matrix.py): the plan figures, every argument refusal of
idb_attention_fwd_train / idb_attention_bwd / idb_lora_grad (return code, a message naming the argument, zero launches), the defect-free
emulation against every criterion with its worst err / bound printed, and the teeth: each injected defect must fail the case and
recipe named for it.

Worst err / bound of the defect-free emulation, bf16 / f16 (test_emulation_meets_criteria prints them per recipe and gradient):
normal dQ 0.453 / 0.484, dK 0.679 / 0.836, dV 0.923 / 0.853; peaked 0.321 / 0.309, 0.396 / 0.408, 0.867 / 0.646; count dQ 0.326 / 0.332,
dV 0.235 / 0.280; ones_dout 0.117 / 0.201, 0.748 / 0.848, 0.966 / 0.876; every structured element (count's dK and power-of-two dV, all
of one_hot) is exact.  All constants of the criteria are 1 or a count of roundings; none had to be raised and no term was missing."""
import ctypes as C
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_bwd_matrix as BM  # noqa: E402
import matrix_common as MC  # noqa: E402
from faceposegenerator_amd import _lib as L  # noqa: E402

DTYPES = ("bf16", "f16")
_REFS = {}


def _setup(lib, case, recipe, dtype):
    """Inputs, reference and saved tensors of one (case, recipe, dtype), computed once per process."""
    key = (case.name, recipe, dtype)
    if key not in _REFS:
        inp = BM.make_inputs(case, recipe, dtype)
        r = BM.reference(inp, case)
        _REFS[key] = (inp, r, BM.saved(r, dtype))
    return _REFS[key]


def _verdicts(lib, case, recipe, dtype, defect=None):
    inp, r, (out_t, lse32) = _setup(lib, case, recipe, dtype)
    got = BM.emulate(inp, out_t, lse32, case, dtype, BM.case_plan(lib, case)[2], defect,
                     pad_value=math.nan if case.poison != "max" else torch.finfo(BM.TDT[dtype]).max)
    exp, bnd = BM.expected(inp, r, case, recipe, dtype), BM.bound(inp, r, case, recipe, dtype)
    return {n: MC.check_t(g, exp[n], bnd[n]) for n, g in zip(("dq", "dk", "dv"), got)}


# ---- plans ------------------------------------------------------------------------------------------------------------------------------
def test_plan_figures(lib):
    rc, (form, kb, rows, launches) = BM.plan(lib, 1, 1, 1, 1)
    assert (rc, form, kb, launches) == (0, 0, L.IDB_ATTN_BWD_KEY_BLOCK, 3) and rows % L.IDB_ATTN_BWD_SLICE == 0
    for case in BM.cases(lib):
        form, kb, rows, launches = BM.case_plan(lib, case)
        assert form == case.form, f"{case.name}: the plan reports form {form}"
        assert launches == (4 if form else 3) and rows % L.IDB_ATTN_BWD_SLICE == 0 and kb == L.IDB_ATTN_BWD_KEY_BLOCK
        assert (rows < case.n_q) == bool(form), (case.name, rows)
        need = lib.idb_attention_bwd_workspace_bytes(case.batch, case.heads, case.n_q, case.n_kv)
        delta = -(-case.batch * case.heads * case.n_q * 4 // 256) * 256
        chunks = -(-case.n_q // rows)
        assert need == delta + (2 * chunks * case.batch * case.heads * case.n_kv * 256 if form else 0), case.name
    # the SD-2.1 shapes (batch 2): which form each takes
    sd = {(5, 4096, 4096): 0, (10, 1024, 1024): 0, (20, 256, 256): 1, (20, 64, 64): 0, (5, 4096, 77): 1, (10, 1024, 77): 1, (20, 256, 77): 1,
          (20, 64, 77): 0}
    for (h, nq, nk), form in sd.items():
        assert BM.plan(lib, 2, h, nq, nk)[1][0] == form, (h, nq, nk)
    names = [c.name for c in BM.threshold_cases(lib)]
    assert len(names) == 4 and len({c.form for c in BM.threshold_cases(lib)}) == 2, names
    bad = [C.c_int32(0)] * 4
    assert lib.idb_attention_bwd_plan(1, 1, 0, 1, *[C.byref(x) for x in bad]) == MC.EINVAL and b"dims" in lib.idb_last_error()
    assert lib.idb_attention_bwd_workspace_bytes(1, 1, 0, 1) == 0


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def _bwd_ok():
    P, M = MC.P16, 1 << 24            # distinct, far apart, 16-byte aligned
    return dict(q=P, q_ld=128, k=P + M, v=P + 2 * M, kv_ld=128, out=P + 3 * M, out_ld=128, dout=P + 4 * M, dout_ld=128, lse=P + 5 * M, dq=P + 6 * M,
                dq_ld=128, dk=P + 7 * M, dv=P + 8 * M, dkv_ld=128, workspace=P + 9 * M, workspace_bytes=1 << 20, batch=1, heads=2, n_q=16, n_kv=16,
                n_kv_alloc=16, scale=0.125, dtype=L.IDB_F16)


def _bwd_call(lib):
    order = ("q", "q_ld", "k", "v", "kv_ld", "out", "out_ld", "dout", "dout_ld", "lse", "dq", "dq_ld", "dk", "dv", "dkv_ld", "workspace",
             "workspace_bytes", "batch", "heads", "n_q", "n_kv", "n_kv_alloc", "scale", "dtype")
    return lambda kw: lib.idb_attention_bwd(*[kw[n] for n in order], None)


def test_bwd_refusals(lib):
    ok, call = _bwd_ok(), _bwd_call(lib)
    ptrs = ("q", "k", "v", "out", "dout", "lse", "dq", "dk", "dv", "workspace")
    for name in ptrs:
        MC.refused(lib, call, ok, [{name: None}], f"{name} is null")
        MC.refused(lib, call, ok, [{name: ok[name] + (2 if name == "lse" else 4)}], f"{name} is not aligned")
    for name in ("q_ld", "kv_ld", "out_ld", "dout_ld", "dq_ld", "dkv_ld"):
        MC.refused(lib, call, ok, [{name: 120}, {name: 132}, {name: 0}, {name: -128}], name)       # below heads*64; not 16-byte rows
    MC.refused(lib, call, ok, [dict(workspace_bytes=0), dict(workspace_bytes=lib.idb_attention_bwd_workspace_bytes(1, 2, 16, 16) - 1)],
               "workspace_bytes")
    MC.refused(lib, call, ok, [dict(batch=0), dict(heads=0), dict(n_q=0), dict(n_kv=0), dict(n_q=-1)], "bad dims")
    MC.refused(lib, call, ok, [dict(n_kv_alloc=15)], "n_kv_alloc")
    MC.refused(lib, call, ok, [dict(scale=0.0), dict(scale=-1.0), dict(scale=math.inf), dict(scale=math.nan)], "scale")
    MC.refused(lib, call, ok, [dict(batch=40000, heads=2)], "too large")
    for o in ("dq", "dk", "dv"):
        for i in ("q", "k", "v", "out", "dout", "lse", "workspace"):
            MC.refused(lib, call, ok, [{o: ok[i]}, {o: ok[i] + 16}], f"{o} aliases {i}")
    # a dtype other than the two: IDB_EUNSUPPORTED, named, nothing launched
    before = lib.idb_launch_count()
    for kw in MC.BAD_DTYPES + [dict(dtype=L.IDB_F32)]:
        assert call({**ok, **kw}) == -2 and b"dtype" in lib.idb_last_error()
    assert lib.idb_launch_count() == before
    # the packed layout is accepted as far as the argument checks go: gradients interleaved with each other, not with the inputs
    packed = dict(k=ok["q"] + 256, v=ok["q"] + 512, q_ld=384, kv_ld=384, dk=ok["dq"] + 256, dv=ok["dq"] + 512, dq_ld=384, dkv_ld=384)
    MC.refused(lib, call, {**ok, **packed}, [dict(workspace_bytes=0)], "workspace_bytes")


def test_fwd_train_refusals(lib):
    P, M = MC.P16, 1 << 24
    ok = dict(q=P, q_ld=128, k=P + M, v=P + 2 * M, kv_ld=128, out=P + 3 * M, out_ld=128, lse=P + 4 * M, batch=1, heads=2, n_q=16, n_kv=16,
              n_kv_alloc=16, scale=0.125, dtype=L.IDB_BF16)
    order = ("q", "q_ld", "k", "v", "kv_ld", "out", "out_ld", "lse", "batch", "heads", "n_q", "n_kv", "n_kv_alloc", "scale", "dtype")
    call = lambda kw: lib.idb_attention_fwd_train(*[kw[n] for n in order], None)       # noqa: E731
    for name in ("q", "k", "v", "out", "lse"):
        MC.refused(lib, call, ok, [{name: None}], f"{name} is null")
    MC.refused(lib, call, ok, [dict(q=P + 4), dict(out=P + 8)], "unaligned")
    for name in ("q_ld", "kv_ld", "out_ld"):
        MC.refused(lib, call, ok, [{name: 120}, {name: 132}], name)
    MC.refused(lib, call, ok, [dict(n_kv_alloc=15)], "n_kv_alloc")
    MC.refused(lib, call, ok, [dict(scale=0.0)], "scale")
    MC.refused(lib, call, ok, [dict(batch=0), dict(n_kv=0)], "bad dims")
    before = lib.idb_launch_count()
    assert call({**ok, "dtype": L.IDB_F32}) == -2 and b"dtype" in lib.idb_last_error() and lib.idb_launch_count() == before


def test_lora_grad_refusals(lib):
    P, M = MC.P16, 1 << 24
    ok = dict(x=P, x_ld=64, dy=P + M, dy_ld=192, lora_a=P + 2 * M, lora_b=P + 3 * M, da=P + 4 * M, db=P + 5 * M, m=40, n_in=64, n_out=64, rank=4,
              scale=1.0, workspace=P + 6 * M, workspace_bytes=1 << 20, dtype=L.IDB_F16)
    order = ("x", "x_ld", "dy", "dy_ld", "lora_a", "lora_b", "da", "db", "m", "n_in", "n_out", "rank", "scale", "workspace", "workspace_bytes", "dtype")
    call = lambda kw: lib.idb_lora_grad(*[kw[n] for n in order], None)       # noqa: E731
    for name in ("x", "dy", "lora_a", "lora_b", "da", "db", "workspace"):
        MC.refused(lib, call, ok, [{name: None}], f"{name} is null")
        MC.refused(lib, call, ok, [{name: ok[name] + 2}], f"{name} is not aligned")
    MC.refused(lib, call, ok, [dict(x_ld=56), dict(x_ld=68)], "x_ld")
    MC.refused(lib, call, ok, [dict(dy_ld=56), dict(dy_ld=196)], "dy_ld")
    MC.refused(lib, call, ok, [dict(rank=0), dict(rank=L.IDB_LORA_MAX_RANK + 1)], "rank")
    MC.refused(lib, call, ok, [dict(n_in=96), dict(n_in=0)], "in must")
    MC.refused(lib, call, ok, [dict(n_out=32), dict(n_out=-64)], "out must")
    MC.refused(lib, call, ok, [dict(m=0)], "m must")
    MC.refused(lib, call, ok, [dict(workspace_bytes=lib.idb_lora_grad_workspace_bytes(40, 64, 64, 4) - 1)], "workspace_bytes")
    before = lib.idb_launch_count()
    assert call({**ok, "dtype": 7}) == -2 and b"dtype" in lib.idb_last_error() and lib.idb_launch_count() == before
    # the workspace: both projections [m][16] fp32 and one partial [rank][in + out] per chunk
    cr, cap = L.IDB_LORA_GRAD_CHUNK_ROWS, L.IDB_LORA_GRAD_MAX_CHUNKS
    for m in (1, cr, cr + 1, cr * cap, cr * cap + 1):
        chunks = -(-m // BM.lora_chunk_rows(m))
        assert chunks <= cap
        assert lib.idb_lora_grad_workspace_bytes(m, 64, 128, 5) == m * 16 * 4 * 2 + chunks * 5 * 192 * 4, m
    assert lib.idb_lora_grad_workspace_bytes(0, 64, 128, 5) == 0


# ---- the emulation meets the criteria; the defects do not -------------------------------------------------------------------------------
def test_emulation_meets_criteria(lib):
    worst = MC.Worst("attention backward emulation")
    for case in BM.cases(lib):
        for recipe in case.recipes:
            for dtype in DTYPES:
                for name, (ok, ratio, nbad) in _verdicts(lib, case, recipe, dtype).items():
                    assert ok, f"{case.name}/{recipe}/{dtype}/{name}: {nbad} elements beyond the criterion, worst ratio {ratio:.3g}"
                    worst.note(f"{recipe:9s} {dtype:4s} {name}", ratio, case.name)
    worst.show()


def test_structured_recipes_are_exact(lib):
    """The expectations of the structured recipes, confirmed rather than taken on trust: count's dK and (n_kv a power of two) dV,
    and all three gradients of one_hot, have a bound of 0 and the defect-free emulation meets it."""
    seen = set()
    for case in BM.cases(lib):
        for recipe in set(case.recipes) & {"count", "one_hot"}:
            inp, r, _ = _setup(lib, case, recipe, "bf16")
            bnd = BM.bound(inp, r, case, recipe, "bf16")
            assert not bnd["dk"].any()
            if recipe == "one_hot":
                assert not bnd["dq"].any() and not bnd["dv"].any()
                assert r.dq.abs().max() < 1e-60 and r.dk.abs().max() < 1e-60          # the float64 gradient agrees: dS vanishes
            elif BM._pow2(case.n_kv):
                assert not bnd["dv"].any()
                seen.add("count_pow2")
            seen.add(recipe)
    assert seen == {"count", "one_hot", "count_pow2"}


# defect -> (case, recipe, the gradients that must fail)
TEETH = {
    "extra_key": ("kb_full", "count", ("dq",)),
    "missing_key": ("kb_full", "count", ("dq", "dk", "dv")),
    "extra_query": ("slice_one_ragged", "count", ("dv",)),
    "missing_query": ("slice_one_ragged", "count", ("dq", "dv")),
    "skip_first_slice": ("chunks_ragged", "count", ("dv",)),
    "skip_last_tile": ("kb_full", "count", ("dq",)),
    "no_delta": ("kb_full", "one_hot", ("dq", "dk")),
    "lse_unscaled": ("kb_full", "one_hot", ("dv",)),
    "p_trunc": ("one_query_long", "ones_dout", ("dv",)),
    "dk_no_scale": ("slice_one", "normal", ("dk",)),
    "slab_left_out": ("chunks_ragged", "count", ("dv",)),
    "pad_attended": ("cross77_nan", "normal", ("dq",)),      # dK / dV of the padding rows themselves land outside the outputs: the GPU file's canary
}


@pytest.mark.parametrize("defect", BM.DEFECTS)
def test_teeth(lib, defect):
    name, recipe, must_fail = TEETH[defect]
    case = {c.name: c for c in BM.cases(lib)}[name]
    assert recipe in case.recipes
    for dtype in DTYPES:
        clean = _verdicts(lib, case, recipe, dtype)
        assert all(v[0] for v in clean.values())
        got = _verdicts(lib, case, recipe, dtype, defect)
        for g in must_fail:
            assert not got[g][0], f"{defect} passes {name}/{recipe}/{dtype}/{g} (worst ratio {got[g][1]:.3g})"
    if defect == "pad_attended":
        mx = {c.name: c for c in BM.cases(lib)}["cross77_max"]
        assert not all(v[0] for v in _verdicts(lib, mx, "normal", "f16", defect).values())


def test_teeth_cover_every_defect():
    assert set(TEETH) == set(BM.DEFECTS)


# ---- idb_lora_grad ----------------------------------------------------------------------------------------------------------------------
def test_lora_grad_emulation_and_teeth():
    worst = MC.Worst("lora_grad emulation")
    for case in BM.lora_cases():
        for dtype in DTYPES:
            x, dy, a, b = BM.lora_inputs(case, dtype)
            da, db, bda, bdb = BM.lora_reference(case, x, dy, a, b)
            eda, edb = BM.lora_emulate(case, x, dy, a, b)
            for n, got, want, bnd in (("da", eda, da, bda), ("db", edb, db, bdb)):
                ok, ratio, nbad = MC.check_t(got, want, bnd)
                assert ok, f"{case.name}/{dtype}/{n}: {nbad} beyond the bound, worst {ratio:.3g}"
                worst.note(f"{case.recipe:8s} {dtype} {n}", ratio, case.name)
            if case.recipe == "b_zero":
                assert not bda.any() and not eda.any() and db.abs().max() > 0
            if case.recipe == "integer":
                assert not bda.any() and not bdb.any() and da.abs().max() > 0
            for defect in ("chunk_left_out", "no_scale"):
                if defect == "chunk_left_out" and case.m <= BM.lora_chunk_rows(case.m):
                    continue
                fda, fdb = BM.lora_emulate(case, x, dy, a, b, defect)
                assert not MC.check_t(fdb, db, bdb)[0], f"{defect} passes {case.name}/{dtype}/db"
                if case.recipe != "b_zero":
                    assert not MC.check_t(fda, da, bda)[0], f"{defect} passes {case.name}/{dtype}/da"
    worst.show()
