"""Host-only side of the norm test matrix (tests/norm_matrix.py), no GPU call:

- idb_groupnorm_plan against norm_matrix.py_plan (the geometry and form rules restated in Python) and against GN_TABLE for every case,
  in all three forms; the case list reaches both slice geometries, chunks = 1 / mid / 64, a short and an empty last chunk, slices that
  straddle x0 | x1, group widths that do not divide the 8-channel vector, and workgroups with idle threads;
- the argument validation of idb_groupnorm, idb_groupnorm_fp8, idb_groupnorm_stats, idb_groupnorm_plan, idb_layernorm, idb_softmax_rows,
  each IDB_REQUIRE once, with dummy addresses that are never dereferenced;
- the float64 references against torch.nn.functional.group_norm / layer_norm / softmax in float64;
- the defect-free emulation meets every criterion on every case and recipe, both dtypes (large tensors on their first and last sample
  and, beyond 4 Mi elements per sample, on the channels of their first slice; tensors of >= 8 Mi elements and the threshold cases on
  `normal` and `count` only, GnCase.cpu_recipes: a calibration of the bound that has to stay a CPU test of about a minute; the GPU
  test launches every recipe on every case and compares every element), with the worst err / criterion printed per recipe;
- teeth: every defect of norm_matrix.DEFECTS fails the criterion of at least one named (case, recipe), next to what today's tensor-wide
  criterion makes of it on `normal` inputs (OLD_CRITERION_TABLE);
- the conditioning envelope of the one-pass variance (printed)."""
import os
import sys
from collections import defaultdict

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import norm_matrix as NM  # noqa: E402
from faceposegenerator_amd import _lib as L  # noqa: E402

DTYPES = ("bf16", "f16")
PTR = NM.PTR
EINVAL = -1
FP8_INV_SCALE = 200.0


# ------------------------------------------------------------------------------------------------------------------------------------
# the plan query
# ------------------------------------------------------------------------------------------------------------------------------------
def test_plan_matches_the_rules_and_the_case_table(lib):
    cases = NM.gn_cases(lib)
    assert len({c.name for c in cases}) == len(cases)
    seen = defaultdict(int)
    for c in cases:
        for sync_len, pch in ((0, 0), (NM.SYNC_LEN, 0)) + (((0, c.hw // 64),) if c.pin_ok else ()):
            rc, p = NM.plan(lib, c.c0, c.c1, c.batch, c.hw, c.groups, sync_len, pch)
            assert rc == 0, (c.name, lib.idb_last_error())
            assert p == NM.py_plan(c.c0, c.c1, c.batch, c.hw, c.groups, sync_len, pch), (c.name, sync_len, pch, p)
            assert p.sw * p.slices == c.c and p.sw % c.cpg == 0 and p.sw % 8 == 0 and p.pr == 256 // p.cols
            assert p.chunks * p.chunk_len >= c.hw and 1 <= p.chunks <= 64
            seen["form", p.form] += 1
            if sync_len:
                assert (p.form == 1) == c.single, f"{c.name}: single-launch eligibility is not what the table says"
                if p.form == 1:
                    assert -(-p.chunk_len // p.pr) <= 4 and p.chunks * p.slices * c.batch <= 1024 and p.apply_blocks == 0
            if pch:
                assert (p.form, p.chunks, p.chunk_len) == (2, c.hw // 64, 64)
        p = NM.plan(lib, c.c0, c.c1, c.batch, c.hw, c.groups)[1]
        assert (p.form, p.sw, p.chunks) == (0, c.sw, c.chunks), f"{c.name}: chosen for {c.sw}-channel slices and {c.chunks} chunks, the plan reports {p}"
        aligned = c.batch * c.hw * c.c >= NM.GN_ALIGN
        if c.name.startswith("big_"):
            assert aligned and p.sw % 64 == 0, c.name
        if c.name.startswith("twin_"):
            assert not aligned and p.sw == NM.py_plan(c.c0, c.c1, 1, 1, c.groups).sw, c.name
        seen["aligned" if aligned and p.sw % 64 == 0 and c.cpg in (10, 20, 30, 40, 60, 80) else "plain"] += 1
        seen["chunks1" if p.chunks == 1 else "chunks64" if p.chunks == 64 else "chunksmid"] += 1
        seen["straddle" if c.c1 and c.c0 % p.sw else "whole"] += 1
        seen["cpg_not_dividing_8" if 8 % c.cpg and c.cpg % 8 else "cpg_divides"] += 1
        seen["idle_threads" if p.pr * p.cols < 256 else "all_threads"] += 1
        seen["len_multiple_of_pr" if p.chunk_len % p.pr == 0 else "len_not_multiple"] += 1
        last = c.hw - (p.chunks - 1) * p.chunk_len
        seen["last_empty" if last <= 0 else "last_short" if last < p.chunk_len else "last_full"] += 1
        seen["c0<c1" if 0 < c.c0 < c.c1 else "c0>c1" if c.c0 > c.c1 > 0 else "other"] += 1
    for key in ("aligned", "plain", "chunks1", "chunksmid", "chunks64", "straddle", "whole", "cpg_not_dividing_8", "idle_threads", "all_threads",
                "len_multiple_of_pr", "len_not_multiple", "last_empty", "last_short", "last_full", "c0<c1", "c0>c1", ("form", 0), ("form", 1), ("form", 2)):
        assert seen[key] >= 2, (key, dict(seen))
    assert seen["aligned"] >= 6
    thr = {c.name: c for c in NM.threshold_cases(lib)}
    for name in ("thr_chunks64", "thr_blocks1024"):
        lo, hi = thr[name + "_lo"], thr[name + "_hi"]
        assert lo.single and not hi.single and hi.hw == lo.hw + 1
    assert (thr["thr_chunks64_lo"].hw, thr["thr_blocks1024_lo"].hw) == (6400, 3200)
    # the sync_len limit: 2 * batch * slices counters are enough, one fewer is not
    assert NM.plan(lib, 320, 0, 2, 1024, 32, 16)[1].form == 1 and NM.plan(lib, 320, 0, 2, 1024, 32, 15)[1].form == 0
    # at most 4 passes per chunk never decides alone (see threshold_cases): the library reports the single-launch form exactly where the
    # other three conditions hold
    for c, batch in ((320, 1), (640, 3), (96, 8), (960, 2), (512, 5), (1280, 7)):
        for hw in range(1, 9000, 7):
            two, p = NM.plan(lib, c, 0, batch, hw, 32)[1], NM.plan(lib, c, 0, batch, hw, 32, NM.SYNC_LEN)[1]
            fch = -(-hw // (4 * two.pr))
            want = fch <= 64 and fch * two.slices * batch <= 1024 and 2 * batch * two.slices <= NM.SYNC_LEN
            assert (p.form == 1) == want, (c, batch, hw, p)
    pin_stat = tuple(c.name for c in cases if c.pin_ok and (lambda p: (p.chunks, p.chunk_len) == (c.hw // 64, 64))(NM.plan(lib, c.c0, c.c1, c.batch, c.hw, c.groups)[1]))
    assert pin_stat == NM.PIN_STAT_CASES, pin_stat
    for c, batch, side in NM.GEMM_PIN:
        p = NM.plan(lib, c, 0, batch, side * side, 32)[1]
        assert (p.chunks, p.chunk_len) != (side * side // 64, 64), (c, batch, side, p)


def test_plan_refuses_what_idb_groupnorm_refuses(lib):
    bad = [(0, 0, 1, 1, 32, 0, 0), (320, -8, 1, 1, 32, 0, 0), (320, 0, 0, 1, 32, 0, 0), (320, 0, 1, 0, 32, 0, 0), (320, 0, 1, 1, 0, 0, 0),
           (324, 0, 1, 1, 4, 0, 0), (320, 4, 1, 1, 4, 0, 0), (320, 0, 1, 1, 33, 0, 0), (32, 0, 1, 1, 32, 0, 0),
           (2056, 0, 1, 1, 8, 0, 0), (320, 0, 65536, 1, 32, 0, 0), (320, 0, 1, 1, 32, -1, 0),
           (320, 320, 1, 64, 32, 0, 1), (320, 0, 1, 65, 32, 0, 1), (320, 0, 1, 128, 32, 0, 1), (320, 0, 1, 8192, 32, 0, 128)]
    for args in bad:
        rc, _ = NM.plan(lib, *args)
        assert rc == EINVAL, args
        assert b"idb_groupnorm_plan" in lib.idb_last_error()
    assert lib.idb_groupnorm_plan(320, 0, 1, 64, 32, 0, 0, None, None, None, None, None, None, None) == EINVAL


def test_argument_validation(lib):
    """Each IDB_REQUIRE of the five entry points once; all return before any HIP call (no device here, the addresses are dummies).
    (c0, c1, groups) = (2056, 0, 8) passes the channel checks (cpg 257) and is refused by the "unsupported geometry" check: its slice
    is lcm(257, 8) = 2056 channels, 257 vector columns for 256 threads."""
    launches = lib.idb_launch_count()
    gn = dict(x0=PTR, c0=320, x1=None, c1=0, batch=1, hw=64, groups=32, eps=1e-5, gamma=PTR, beta=PTR, silu=1, out=PTR, dtype=L.IDB_BF16, ws=PTR,
              ws_bytes=1 << 20, sync=None, sync_len=0, pin=None, pch=0, stream=None)
    bad_gn = [(dict(dtype=L.IDB_F32), b"dtype"), (dict(x0=None), b"null/unaligned"), (dict(out=PTR + 8), b"null/unaligned"), (dict(gamma=PTR + 4), b"null/unaligned"),
              (dict(beta=None), b"null/unaligned"), (dict(batch=0), b"bad dims"), (dict(hw=0), b"bad dims"), (dict(groups=0), b"bad dims"), (dict(c0=0), b"bad dims"),
              (dict(c1=-8), b"bad dims"), (dict(c1=320), b"x1/c1 mismatch"), (dict(x1=PTR), b"x1/c1 mismatch"), (dict(x1=PTR + 2, c1=320), b"x1 unaligned"),
              (dict(c0=324, groups=4), b"unsupported"), (dict(groups=33), b"unsupported"), (dict(c0=32), b"at least 2 channels"),
              (dict(c0=2056, groups=8), b"unsupported geometry"), (dict(batch=65536), b"unsupported geometry"),
              (dict(ws=None), b"workspace too small"), (dict(ws_bytes=64 * 32 * 8 - 1), b"workspace too small"),
              (dict(sync=PTR, sync_len=0), b"bad sync"), (dict(sync=PTR + 2, sync_len=64), b"bad sync"),
              (dict(pin=PTR, pch=2), b"partials_in"), (dict(pin=PTR, pch=1, x1=PTR, c1=320), b"partials_in"), (dict(pin=PTR + 4, pch=1), b"partials_in"),
              (dict(pin=PTR, pch=1, hw=65), b"partials_in"), (dict(pin=PTR, pch=128, hw=8192), b"partials_in")]
    for kw, msg in bad_gn:
        a = dict(gn, **kw)
        assert lib.idb_groupnorm(*a.values()) == EINVAL, kw
        assert msg in lib.idb_last_error() and b"idb_groupnorm:" in lib.idb_last_error(), (kw, lib.idb_last_error())
    f8 = dict(x0=PTR, c0=320, x1=None, c1=0, batch=1, hw=64, groups=32, eps=1e-5, gamma=PTR, beta=PTR, silu=1, out=PTR, inv=1.0, dtype=L.IDB_BF16,
              ws=PTR, ws_bytes=1 << 20, pin=None, pch=0, stream=None)
    bad_f8 = [(dict(inv=0.0), b"out_inv_scale"), (dict(out=None), b"out_inv_scale"), (dict(out=PTR + 4), b"out_inv_scale"),
              (dict(dtype=99), b"bad pointers"), (dict(x0=PTR + 8), b"bad pointers"), (dict(gamma=None), b"bad pointers"), (dict(beta=PTR + 4), b"bad pointers"),
              (dict(batch=0), b"bad dims"), (dict(c1=320), b"bad dims"), (dict(x1=PTR + 8, c1=320), b"bad dims"),
              (dict(c0=324, groups=4), b"unsupported"), (dict(c0=32), b"unsupported"), (dict(c0=2056, groups=8), b"unsupported geometry"),
              (dict(ws_bytes=100), b"workspace too small"), (dict(pin=PTR, pch=2), b"bad partials_in")]
    for kw, msg in bad_f8:
        a = dict(f8, **kw)
        assert lib.idb_groupnorm_fp8(*a.values()) == EINVAL, kw
        assert msg in lib.idb_last_error() and b"idb_groupnorm_fp8:" in lib.idb_last_error(), (kw, lib.idb_last_error())
    import ctypes as C
    chunks = C.c_int32(-1)
    st = dict(x0=PTR, c0=320, x1=None, c1=0, batch=1, hw=64, groups=32, partials=PTR, pbytes=1 << 20, chunks=C.byref(chunks), dtype=L.IDB_F16, stream=None)
    bad_st = [(dict(x0=None), b"null or unaligned"), (dict(partials=PTR + 8), b"null or unaligned"), (dict(chunks=None), b"null or unaligned"),
              (dict(x1=PTR + 8, c1=320), b"null or unaligned"), (dict(dtype=L.IDB_F32), b"bad arguments"), (dict(hw=0), b"bad arguments"),
              (dict(c0=324, groups=4), b"unsupported"), (dict(c1=320), b"unsupported"), (dict(c0=32), b"unsupported"),
              (dict(c0=2056, groups=8), b"unsupported geometry"), (dict(batch=65536), b"unsupported geometry"), (dict(pbytes=2 * 32 * 8 - 1), b"too small")]
    for kw, msg in bad_st:
        a = dict(st, **kw)
        assert lib.idb_groupnorm_stats(*a.values()) == EINVAL, kw
        assert msg in lib.idb_last_error() and b"idb_groupnorm_stats:" in lib.idb_last_error(), (kw, lib.idb_last_error())
    assert chunks.value == -1
    ln = dict(x=PTR, out=PTR, rows=4, c=320, eps=1e-5, gamma=PTR, beta=PTR, dtype=L.IDB_BF16, stream=None)
    bad_ln = [(dict(dtype=L.IDB_F32), b"dtype"), (dict(x=None), b"null/unaligned"), (dict(out=PTR + 8), b"null/unaligned"), (dict(gamma=PTR + 4), b"null/unaligned"),
              (dict(beta=None), b"null/unaligned"), (dict(rows=0), b"unsupported"), (dict(c=0), b"unsupported"), (dict(c=324), b"unsupported"),
              (dict(c=1544), b"unsupported"), (dict(rows=1 << 33), b"too many rows")]
    for kw, msg in bad_ln:
        a = dict(ln, **kw)
        assert lib.idb_layernorm(*a.values()) == EINVAL, kw
        assert msg in lib.idb_last_error(), (kw, lib.idb_last_error())
    for args in ((PTR, 4, 64, L.IDB_F32, None), (None, 4, 64, L.IDB_BF16, None), (PTR + 8, 4, 64, L.IDB_BF16, None), (PTR, 0, 64, L.IDB_BF16, None),
                 (PTR, 1 << 31, 64, L.IDB_BF16, None), (PTR, 4, 0, L.IDB_BF16, None), (PTR, 4, 60, L.IDB_BF16, None)):
        assert lib.idb_softmax_rows(*args) == EINVAL, args
        assert b"idb_softmax_rows" in lib.idb_last_error()
    assert lib.idb_launch_count() == launches


# ------------------------------------------------------------------------------------------------------------------------------------
# the references
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b,hw,c,groups,silu,eps", [(2, 100, 320, 32, True, 1e-5), (1, 7, 96, 32, False, 1e-6), (3, 64, 64, 1, True, 1e-5)])
def test_groupnorm_reference_matches_torch(b, hw, c, groups, silu, eps):
    g = torch.Generator().manual_seed(2)
    x, gamma, beta = torch.randn(b, hw, c, generator=g, dtype=torch.float64) * 3 + 1, torch.randn(c, generator=g, dtype=torch.float64), torch.randn(c, generator=g, dtype=torch.float64)
    r = NM.gn_reference(x, gamma, beta, groups, eps, silu)
    want = F.group_norm(x.permute(0, 2, 1), groups, gamma, beta, NM.eps32(eps)).permute(0, 2, 1)
    want = F.silu(want) if silu else want
    assert (r.ref - want).abs().max().item() < 1e-12
    xg = x.view(b, hw, groups, c // groups)
    assert torch.allclose(r.var.view(b, groups, -1)[..., 0], xg.var(dim=(1, 3), unbiased=False), rtol=1e-12, atol=0)


def test_layernorm_and_softmax_references_match_torch():
    g = torch.Generator().manual_seed(3)
    x, gamma, beta = torch.randn(5, 504, generator=g, dtype=torch.float64) * 3 + 1, torch.randn(504, generator=g, dtype=torch.float64), torch.randn(504, generator=g, dtype=torch.float64)
    assert (NM.ln_reference(x, gamma, beta, 1e-5)[0] - F.layer_norm(x, (504,), gamma, beta, NM.eps32(1e-5))).abs().max().item() < 1e-12
    assert (NM.sm_reference(x * 10) - torch.softmax(x * 10, -1)).abs().max().item() < 1e-15


def test_fp8_reference_rounds_to_nearest_even_and_saturates():
    y = torch.tensor([0.0, 17.0, 19.0, 18.0, 1000.0, -1000.0, 2.0 ** -10, 3 * 2.0 ** -11, 464.0], dtype=torch.float64)
    assert NM.fp8_value(y, 1.0).tolist() == [0.0, 16.0, 20.0, 18.0, 448.0, -448.0, 0.0, 2.0 ** -9, 448.0]


# ------------------------------------------------------------------------------------------------------------------------------------
# the criteria hold for the kernels' arithmetic
# ------------------------------------------------------------------------------------------------------------------------------------
def _sample(case, p, x, gamma, beta):
    """First and last sample; beyond 4 Mi elements per sample the channels of the first slice only (whole groups, same geometry)."""
    c0, groups = case.c0, case.groups
    if case.batch > 2:
        x = x[[0, -1]]
    if case.hw * case.c > 1 << 22:
        x, gamma, beta, groups, c0 = x[..., :p.sw].contiguous(), gamma[:p.sw], beta[:p.sw], p.sw // case.cpg, min(c0, p.sw)
    return x, gamma, beta, groups, c0


def _exact_partials(x, p, groups):
    want, _ = NM.gn_partial_sums(x, p, groups)
    return want


def _forms(lib, case, recipe):
    """(label, plan) of every form the case is launched in."""
    out = [("two", NM.plan(lib, case.c0, case.c1, case.batch, case.hw, case.groups)[1])]
    if case.single:
        out.append(("single", NM.plan(lib, case.c0, case.c1, case.batch, case.hw, case.groups, NM.SYNC_LEN)[1]))
    if case.pin_ok:
        out.append(("pin", NM.plan(lib, case.c0, case.c1, case.batch, case.hw, case.groups, 0, case.hw // 64)[1]))
    return out


def test_groupnorm_emulation_meets_criteria(lib):
    worst = defaultdict(float)
    for case in NM.gn_cases(lib):
        for dtype in DTYPES:
            for recipe in case.cpu_recipes:
                xf, ga, be = NM.gn_inputs(case, recipe, dtype)
                for label, p in _forms(lib, case, recipe):
                    if label != "two" and recipe not in ("normal", "count", "offset"):
                        continue
                    x, gamma, beta, groups, c0 = _sample(case, p, xf, ga, be)
                    r = NM.gn_reference(x, gamma, beta, groups, case.eps, case.silu)
                    if label == "pin":      # (a): float64 sums of the 64-pixel chunks rounded to fp32
                        pin = _exact_partials(x, p, groups).float()
                        out = NM.emulate_gn(x, c0, gamma, beta, groups, case.eps, case.silu, dtype, p, pin=pin)
                    else:
                        part = NM.emulate_gn_partials(x, c0, groups, p)
                        want, mag = NM.gn_partial_sums(x, p, groups)
                        if recipe in NM.EXACT_SUMS:
                            assert torch.equal(part.double(), want), f"{case.name} {dtype} {recipe} {label}: a partial sum is not the exact integer"
                        else:
                            assert ((part.double() - want).abs() <= NM.gn_depth(p) * NM.E24 * mag).all(), (case.name, dtype, recipe, label)
                        out = NM.emulate_gn(x, c0, gamma, beta, groups, case.eps, case.silu, dtype, p, pin=part)
                    ok, ratio, nbad = NM.check(out, r.ref, NM.gn_bound(r, p, dtype, recipe))
                    assert ok, f"{case.name} {dtype} {recipe} {label}: {nbad} elements beyond the criterion, worst ratio {ratio}"
                    worst[dtype, recipe] = max(worst[dtype, recipe], ratio)
                    if case.fp8 and label != "single":
                        o8 = NM.emulate_gn(x, c0, gamma, beta, groups, case.eps, case.silu, dtype, p, pin=pin if label == "pin" else part, fp8_inv_scale=FP8_INV_SCALE)
                        lo, hi = NM.fp8_interval(r, p, dtype, recipe, FP8_INV_SCALE)
                        assert ((o8 >= lo) & (o8 <= hi)).all(), f"{case.name} {dtype} {recipe} {label}: fp8 byte outside the allowed interval"
                        if recipe == "normal":
                            assert (o8.abs() == 448).any() and ((o8 != 0) & (o8.abs() < 2.0 ** -6)).any(), f"{case.name}: no saturated / subnormal e4m3 value"
    print()
    for (dtype, recipe), w in sorted(worst.items()):
        print(f"groupnorm emulation vs float64, {dtype:4s} {recipe:15s}: worst err / criterion {w:.3f}")
    assert max(worst.values()) <= 1.0


def test_layernorm_and_softmax_emulation_meet_criteria():
    worst = defaultdict(float)
    for dtype in DTYPES:
        for c in NM.LN_C:
            for rows in NM.LN_ROWS:
                for recipe in NM.LN_RECIPES:
                    x, gamma, beta = NM.ln_inputs(rows, c, recipe, dtype)
                    ref, bnd = NM.ln_bound(x, gamma, beta, 1e-5, dtype, recipe)
                    ok, ratio, nbad = NM.check(NM.emulate_ln(x, gamma, beta, 1e-5, dtype), ref, bnd)
                    assert ok, f"layernorm {rows}x{c} {dtype} {recipe}: {nbad} elements beyond the criterion, worst ratio {ratio}"
                    worst["layernorm", dtype, recipe] = max(worst["layernorm", dtype, recipe], ratio)
        for cols in NM.SM_COLS:
            for rows in NM.SM_ROWS:
                for recipe in NM.SM_RECIPES:
                    x = NM.sm_inputs(rows, cols, recipe, dtype)
                    ref, bnd = NM.sm_bound(x, dtype)
                    ok, ratio, nbad = NM.check(NM.emulate_sm(x, dtype), ref, bnd)
                    assert ok, f"softmax {rows}x{cols} {dtype} {recipe}: {nbad} elements beyond the criterion, worst ratio {ratio}"
                    worst["softmax", dtype, recipe] = max(worst["softmax", dtype, recipe], ratio)
    print()
    for (op, dtype, recipe), w in sorted(worst.items()):
        print(f"{op} emulation vs float64, {dtype:4s} {recipe:13s}: worst err / criterion {w:.3f}")


# ------------------------------------------------------------------------------------------------------------------------------------
# teeth
# ------------------------------------------------------------------------------------------------------------------------------------
def _gn_defect_run(lib, case, recipe, dtype, defect):
    """The emulation with one defect under the case's criterion: (applicable, fails)."""
    form = "single" if defect == "stale_partial" else "pin" if defect == "apply_wrong_chunks" else "two"
    plans = dict(_forms(lib, case, recipe))
    if form not in plans or (defect in NM.FP8_DEFECTS and not case.fp8):
        return False, False
    p = plans[form]
    xf, ga, be = NM.gn_inputs(case, recipe, dtype)
    x, gamma, beta, groups, c0 = _sample(case, p, xf, ga, be)
    r = NM.gn_reference(x, gamma, beta, groups, case.eps, case.silu)
    kw = {}
    if defect == "stale_partial":
        xs = _sample(case, p, *NM.gn_inputs(case, recipe, dtype, seed=31))[0]
        kw["stale"] = NM.emulate_gn_partials(xs, c0, groups, p)
    if defect == "apply_wrong_chunks":
        kw["pin"], kw["wrong"] = _exact_partials(x, p, groups).float(), plans["two"]
        if plans["two"].chunks == p.chunks:
            return False, False
    if defect in NM.FP8_DEFECTS:
        o8 = NM.emulate_gn(x, c0, gamma, beta, groups, case.eps, case.silu, dtype, p, defect=defect, fp8_inv_scale=FP8_INV_SCALE)
        lo, hi = NM.fp8_interval(r, p, dtype, recipe, FP8_INV_SCALE)
        return True, not bool((torch.isfinite(o8) & (o8 >= lo) & (o8 <= hi)).all())
    out = NM.emulate_gn(x, c0, gamma, beta, groups, case.eps, case.silu, dtype, p, defect=defect, **kw)
    return True, not NM.check(out, r.ref, NM.gn_bound(r, p, dtype, recipe))[0]


TEETH_RECIPES = {"no_eps": ("constant_group",), "no_clamp": ("constant_offset", "offset"), "neighbour_gamma": ("normal",), "silu_skipped": ("normal",),
                 "fp8_no_saturation": ("normal",), "fp8_double_rounding": ("normal",)}
OLD_GN = ("u1280p640_hw100", "u640_hw1024", "cpg2_hw256", "u320_hw4096")


def test_teeth(lib):
    """Every defect fails the new criteria on a named (case, recipe), in both dtypes; and the old criterion's verdict on `normal` inputs."""
    cases = [c for c in NM.gn_cases(lib) if not c.big]
    by_name = {c.name: c for c in cases}
    caught, tried = defaultdict(list), defaultdict(int)
    for defect in NM.GN_DEFECTS:
        for dtype in DTYPES:
            for case in cases:
                for recipe in TEETH_RECIPES.get(defect, ("count",)):
                    if recipe not in case.cpu_recipes or len(caught[defect, dtype]) >= 2:
                        continue
                    applicable, fails = _gn_defect_run(lib, case, recipe, dtype, defect)
                    tried[defect, dtype] += applicable
                    if fails:
                        caught[defect, dtype].append(f"{case.name}/{recipe}")
    for defect in NM.LN_DEFECTS:
        for dtype in DTYPES:
            for c, rows, recipe in ((504, 5, "count"), (640, 77, "normal"), (1032, 3, "offset"), (1280, 5, "offset")):
                x, gamma, beta = NM.ln_inputs(rows, c, recipe, dtype)
                ref, bnd = NM.ln_bound(x, gamma, beta, 1e-5, dtype, recipe)
                tried[defect, dtype] += 1
                if not NM.check(NM.emulate_ln(x, gamma, beta, 1e-5, dtype, defect), ref, bnd)[0]:
                    caught[defect, dtype].append(f"layernorm {rows}x{c}/{recipe}")
    for defect in NM.SM_DEFECTS:
        for dtype in DTYPES:
            for cols, rows, recipe in ((2048, 3, "normal"), (4096, 3, "shifted"), (9216, 3, "constant_row"), (504, 3, "normal")):
                x = NM.sm_inputs(rows, cols, recipe, dtype)
                ref, bnd = NM.sm_bound(x, dtype)
                tried[defect, dtype] += 1
                if not NM.check(NM.emulate_sm(x, dtype, defect), ref, bnd)[0]:
                    caught[defect, dtype].append(f"softmax {rows}x{cols}/{recipe}")
    # today's criterion on its own ground: `normal` inputs, tensor-wide; "-": the defect does not apply to the shape
    table = {}
    for defect in NM.DEFECTS:
        row = []
        for dtype in DTYPES:
            v = ""
            if defect in NM.GN_DEFECTS:
                for name in OLD_GN:
                    case = by_name[name]
                    form = "single" if defect == "stale_partial" else "pin" if defect == "apply_wrong_chunks" else "two"
                    plans = dict(_forms(lib, case, "normal"))
                    if form not in plans or defect in NM.FP8_DEFECTS:
                        v += "-"
                        continue
                    p = plans[form]
                    x, gamma, beta = NM.gn_inputs(case, "normal", dtype)
                    kw = {}
                    if defect == "stale_partial":
                        kw["stale"] = NM.emulate_gn_partials(NM.gn_inputs(case, "normal", dtype, seed=31)[0], case.c0, case.groups, p)
                    if defect == "apply_wrong_chunks":
                        kw["pin"], kw["wrong"] = _exact_partials(x, p, case.groups).float(), plans["two"]
                    out = NM.emulate_gn(x, case.c0, gamma, beta, case.groups, case.eps, case.silu, dtype, p, defect=defect, **kw)
                    v += "P" if NM.old_criterion(out, NM.gn_reference(x, gamma, beta, case.groups, case.eps, case.silu).ref, dtype) else "F"
            elif defect in NM.LN_DEFECTS:
                for rows, c in ((77, 640), (513, 1280), (64, 64)):
                    x, gamma, beta = NM.ln_inputs(rows, c, "normal", dtype)
                    v += "P" if NM.old_criterion(NM.emulate_ln(x, gamma, beta, 1e-5, dtype, defect), NM.ln_reference(x, gamma, beta, 1e-5)[0], dtype) else "F"
            else:
                x = NM.sm_inputs(30, 4096, "normal", dtype)
                v += "P" if NM.old_criterion(NM.emulate_sm(x, dtype, defect), NM.sm_reference(x), dtype, 0.5) else "F"
            row.append(v)
        table[defect] = tuple(row)
    print()
    print(f"old criterion on `normal` inputs (GroupNorm: {' / '.join(OLD_GN)}; LayerNorm 77x640 / 513x1280 / 64x64; softmax 30x4096): P passes, F fails, - not applicable")
    for defect in NM.DEFECTS:
        for i, dtype in enumerate(DTYPES):
            print(f"{defect:20s} {dtype:4s}: new criteria fail on {', '.join(caught[defect, dtype]) or 'NOTHING'} (of {tried[defect, dtype]} tried); old criterion {table[defect][i]}")
    for defect in NM.DEFECTS:
        for dtype in DTYPES:
            assert caught[defect, dtype], f"{defect} / {dtype}: no case of the list fails its criterion"
    assert table == NM.OLD_CRITERION_TABLE, f"update norm_matrix.OLD_CRITERION_TABLE (documentation of what the old criterion lets through):\n{table}"


# ------------------------------------------------------------------------------------------------------------------------------------
# the conditioning envelope of the one-pass variance
# ------------------------------------------------------------------------------------------------------------------------------------
def test_conditioning_envelope(lib):
    """For the three sum lengths that matter, the emulation's worst |got - ref| / (u |ref|) at |mean| / std = R and the smallest R at
    which the criterion's statistics lines alone exceed one output ulp somewhere (2 u |ref|)."""
    print()
    for case in NM.envelope_cases():
        p = NM.plan(lib, case.c0, case.c1, case.batch, case.hw, case.groups)[1]
        for dtype in DTYPES:
            line, first = [], None
            for ratio in NM.ENVELOPE_R:
                x, gamma, beta = NM.envelope_inputs(case, ratio, dtype)
                if case.hw * case.c > 1 << 22:
                    x, gamma, beta = x[..., :p.sw].contiguous(), gamma[:p.sw], beta[:p.sw]
                groups = x.shape[-1] // case.cpg
                r = NM.gn_reference(x, gamma, beta, groups, case.eps, False)
                out = NM.emulate_gn(x, case.c0, gamma, beta, groups, case.eps, False, dtype, p)
                meas, stat = NM.envelope_figures(out, r, p, dtype)
                assert NM.check(out, r.ref, NM.gn_bound(r, p, dtype, "offset"))[0], (case.name, dtype, ratio)
                line.append(f"R={ratio}: {meas:.2f} u (criterion {stat:.2g} u)")
                if first is None and stat > 2.0:
                    first = ratio
            print(f"envelope {case.name} ({case.hw * case.cpg} elements per group) {dtype}: " + "; ".join(line) + f"; criterion exceeds one ulp from R={first}")
