"""Host-only side of the idb_attention test matrix (tests/attn_matrix.py), no GPU call:

- idb_attention_plan: every form is reached by the case list, every threshold of the plan function has a case on each side, rows and
  blocks agree with ceil(n_q / rows) * heads * batch, invalid dims are refused;
- idb_attention's argument validation, each IDB_REQUIRE once, with dummy addresses that are never dereferenced;
- the float64 reference against torch's scaled_dot_product_attention;
- the criteria hold for the reference arithmetic: the defect-free emulation meets the criterion of every case and recipe in both
  dtypes (cases with many scores on a sample of heads and query rows: this is a calibration of the bound, the GPU test compares every
  element), the worst err / bound ratio is printed and is <= 1, and every const_v case has its exactness margin;
- teeth: every defect of attn_matrix.DEFECTS makes the emulation fail the criterion of at least one small case in both dtypes, and
  the table of what the old tensor-wide criterion let through is printed."""
import os
import sys
from collections import defaultdict

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_matrix as AM  # noqa: E402
from faceposegenerator_amd import _lib as L  # noqa: E402

DTYPES = ("bf16", "f16")
PTR = AM.PTR
EINVAL = -1          # idb_status IDB_EINVAL (include/idb_kernels.h)


# ------------------------------------------------------------------------------------------------------------------------------------
# the plan query
# ------------------------------------------------------------------------------------------------------------------------------------
def test_plan_reaches_every_form_and_threshold(lib):
    cases = AM.cases(lib)
    assert len({c.name for c in cases}) == len(cases)
    forms = defaultdict(int)
    for c in cases:
        waves, key_split, rows, blocks = AM.case_plan(lib, c)
        assert waves == c.waves, f"{c.name}: chosen for the {c.waves}-wave form, the plan reports {waves}"
        assert (waves, key_split, rows) in ((2, 1, 64), (4, 1, 128), (8, 2, 128), (12, 2, 192)), (c.name, waves, key_split, rows)
        assert blocks == -(-c.n_q // rows) * c.heads * c.batch, (c.name, blocks)
        forms[waves, c.causal] += 1
    for f in (2, 4, 8, 12):
        assert forms[f, False] >= 10, forms
    assert forms[2, True] >= 6 and forms[4, True] >= 3, forms
    # one case on each side of each threshold, and the two sides launch different forms (threshold_cases asserts it while searching)
    thr = {c.name: c for c in AM.threshold_cases(lib)}
    for name, rows, lo, hi, _ in AM.THRESHOLDS:
        for side, target in (("lo", lo), ("hi", hi)):
            c = thr[f"thr_{name}_{side}"]
            assert -(-c.n_q // rows) * c.heads * c.batch == target, c
        assert thr[f"thr_{name}_lo"].waves != thr[f"thr_{name}_hi"].waves
    assert (thr["thr_nkv_511"].waves, thr["thr_nkv_512"].waves) == (4, 8)
    assert (thr["thr_blocks128_127_128_lo"].waves, thr["thr_blocks128_127_128_hi"].waves) == (2, 4)
    assert (thr["thr_blocks128_127_128_long_lo"].waves, thr["thr_blocks128_127_128_long_hi"].waves) == (2, 8)
    assert (thr["thr_blocks128_256_257_lo"].waves, thr["thr_blocks128_256_257_hi"].waves) == (8, 12)
    assert (thr["thr_blocks128_511_512_lo"].waves, thr["thr_blocks128_511_512_hi"].waves) == (8, 4)
    assert (thr["thr_blocks192_256_257_lo"].waves, thr["thr_blocks192_256_257_hi"].waves) == (12, 8)
    # causal never takes a key-split form, whatever the grid
    assert AM.plan(lib, 1, 26, 600, 600, 1)[1][0] == 4


def test_plan_refuses_invalid_dims(lib):
    for args in ((0, 1, 1, 1, 0), (1, 0, 1, 1, 0), (1, 1, 0, 1, 0), (1, 1, 1, 0, 0), (-1, 1, 1, 1, 0), (65536, 1, 1, 1, 0), (1, 65536, 1, 1, 0),
                 (1, 1, 64, 65, 1)):
        rc, _ = AM.plan(lib, *args)
        assert rc == EINVAL, args
    assert lib.idb_attention_plan(1, 1, 1, 1, 0, None, None, None, None) == EINVAL
    assert AM.plan(lib, 65535, 1, 1, 1, 0)[0] == 0


def test_attention_argument_validation(lib):
    """Each IDB_REQUIRE of idb_attention once; all of them return before any HIP call (no device here, the addresses are dummies)."""
    good = dict(q=PTR, q_ld=128, k=PTR, v=PTR, kv_ld=128, out=PTR, out_ld=128, batch=1, heads=2, n_q=4, n_kv=4, n_kv_alloc=4, scale=0.125,
                causal=0, dtype=L.IDB_BF16, stream=None)
    order = list(good)
    launches = lib.idb_launch_count()

    def call(**kw):
        a = dict(good, **kw)
        return lib.idb_attention(*[a[k] for k in order])

    bad = [dict(dtype=L.IDB_F32), dict(dtype=99),
           dict(q=None), dict(k=None), dict(v=None), dict(out=None),
           dict(q=PTR + 8), dict(k=PTR + 2), dict(v=PTR + 4), dict(out=PTR + 8),
           dict(batch=0), dict(heads=0), dict(n_q=0), dict(n_kv=0), dict(n_kv_alloc=3),
           dict(q_ld=132), dict(kv_ld=132), dict(out_ld=130),
           dict(q_ld=120), dict(kv_ld=120), dict(out_ld=124),
           dict(batch=65536), dict(heads=65536, q_ld=65536 * 64, kv_ld=65536 * 64, out_ld=65536 * 64),
           dict(causal=1, n_q=4, n_kv=5, n_kv_alloc=5)]
    for kw in bad:
        assert call(**kw) == EINVAL, kw
        assert lib.idb_last_error()
    assert lib.idb_launch_count() == launches


# ------------------------------------------------------------------------------------------------------------------------------------
# the reference
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_q,n_kv,alloc,scale,causal", [(70, 77, 80, 0.125, False), (5, 130, 130, 1.0, False), (129, 129, 129, 0.125, True),
                                                         (1, 1, 1, 0.5, True)])
def test_reference_matches_sdpa(n_q, n_kv, alloc, scale, causal):
    g = torch.Generator().manual_seed(1)
    q, k, v = [torch.randn(2, 3, n, 64, generator=g, dtype=torch.float64) for n in (n_q, alloc, alloc)]
    r = AM.reference(q, k, v, n_kv, scale, causal)
    want = F.scaled_dot_product_attention(q, k[:, :, :n_kv], v[:, :, :n_kv], is_causal=causal, scale=scale)
    assert (r.ref - want).abs().max().item() < 1e-12
    wabs = F.scaled_dot_product_attention(q, k[:, :, :n_kv], v[:, :, :n_kv].abs(), is_causal=causal, scale=scale)
    assert (r.absref - wabs).abs().max().item() < 1e-12
    assert (r.l >= 1).all()


# ------------------------------------------------------------------------------------------------------------------------------------
# the criteria hold for the reference arithmetic
# ------------------------------------------------------------------------------------------------------------------------------------
def _sample(case, inp, max_scores=1 << 21):
    """First and last (batch, head), and when the score matrix is large a sample of query rows that keeps the first and last 70."""
    q, k, v, ex = inp.q[[0, -1]][:, [0, -1]], inp.k[[0, -1]][:, [0, -1]], inp.v[[0, -1]][:, [0, -1]], inp.exact
    ex = None if ex is None else ex[[0, -1]][:, [0, -1]]
    pos = torch.arange(case.n_q)
    if case.n_q * case.n_kv > max_scores:
        keep = max(140, max_scores // case.n_kv)
        pos = torch.cat([pos[:70], pos[70:-70][:: max(1, (case.n_q - 140) // (keep - 140) + 1)], pos[-70:]])
        q, ex = q[:, :, pos], None if ex is None else ex[:, :, pos]
    return AM.Inputs(q, k, v, ex), pos


def test_emulation_meets_criteria(lib):
    worst = defaultdict(float)
    margins = []
    for case in AM.cases(lib):
        for dtype in DTYPES:
            for recipe in case.recipes:
                inp, pos = _sample(case, AM.make_inputs(case, recipe, dtype))
                r = AM.reference(inp.q, inp.k, inp.v, case.n_kv, case.scale, case.causal, pos)
                split = case.waves >= 8
                out = AM.emulate(inp.q, inp.k, inp.v, case.n_kv, case.scale, case.causal, dtype, tiled=split, split=split, q_pos=pos)
                ok, ratio, nbad = AM.check(out, AM.expected(inp, r, recipe), AM.bound(r, case.n_kv, dtype, recipe))
                assert ok, f"{case.name} {dtype} {recipe}: {nbad} elements beyond the criterion, worst ratio {ratio}"
                if recipe not in AM.EXACT:
                    worst[dtype, recipe] = max(worst[dtype, recipe], ratio)
                if recipe == "one_hot":
                    # the construction's promise: the float64 softmax itself is the dominant V row to far below half an output ulp
                    assert ((r.ref - inp.exact).abs() <= 1e-12).all(), case.name
                if recipe == "const_v":
                    # exactness margin: (sum of rounded P) / (sum of P) stays within u/4 of 1 before the output rounding
                    s = AM._scores(inp.q, inp.k, case.n_kv, case.scale, case.causal, pos)
                    p = torch.exp(s - s.amax(-1, keepdim=True))
                    dev = ((AM.rnd(p, dtype).sum(-1) / p.sum(-1)) - 1).abs().max().item()
                    margins.append((case.name, dtype, dev / AM.UNIT[dtype]))
                    assert dev <= AM.UNIT[dtype] / 4, f"{case.name} {dtype}: const_v deviation {dev:.3e} is not below u/4"
    print()
    for (dtype, recipe), w in sorted(worst.items()):
        print(f"emulation vs float64, {dtype:4s} {recipe:10s}: worst err / bound {w:.3f}")
    for dtype in DTYPES:
        w = max(v for (d, _), v in worst.items() if d == dtype)
        print(f"emulation vs float64, {dtype}: worst err / bound over the whole case list {w:.3f}")
        assert w <= 1.0
    for dtype in DTYPES:
        m = [x for x in margins if x[1] == dtype]
        print(f"const_v, {dtype}: {len(m)} cases, worst |sum(rounded P) / sum(P) - 1| = {max(x[2] for x in m):.3f} u (limit 0.25 u; a flipped bit needs 0.5 u)")


# ------------------------------------------------------------------------------------------------------------------------------------
# teeth
# ------------------------------------------------------------------------------------------------------------------------------------
def _small(case):
    return case.batch * case.heads * case.n_q * case.n_kv <= 12_000_000 and case.n_q <= 300


def _applicable(defect, case, recipe):
    if defect in ("causal_plus", "causal_minus"):
        return case.causal
    if defect in AM.SPLIT_DEFECTS:
        return case.waves >= 8
    if defect == "p_trunc":
        return recipe == "const_v"
    if defect in ("skip_last_full_tile",):
        return case.n_kv >= 64
    if defect == "missing_key":
        return case.n_kv > 1
    if defect == "skip_first_tile":
        return case.n_kv > 64
    return True


def test_teeth(lib):
    """Every defect fails the new criteria somewhere, in both dtypes; and what the old criterion made of the same defects."""
    cases = [c for c in AM.cases(lib) if _small(c)]
    caught = defaultdict(list)
    tried = defaultdict(int)
    for case in cases:
        for dtype in DTYPES:
            for recipe in case.recipes:
                if recipe not in ("count", "one_hot", "const_v"):
                    continue
                full = AM.make_inputs(case, recipe, dtype)
                inp = AM.Inputs(full.q[:1, :1], full.k[:1, :1], full.v[:1, :1], None if full.exact is None else full.exact[:1, :1])
                r = AM.reference(inp.q, inp.k, inp.v, case.n_kv, case.scale, case.causal)
                want, bnd = AM.expected(inp, r, recipe), AM.bound(r, case.n_kv, dtype, recipe)
                for defect in AM.DEFECTS:
                    if not _applicable(defect, case, recipe) or len(caught[defect, dtype]) >= 3:
                        continue
                    tried[defect, dtype] += 1
                    out = AM.emulate(inp.q, inp.k, inp.v, case.n_kv, case.scale, case.causal, dtype, defect=defect)
                    ok, ratio, _ = AM.check(out, want, bnd)
                    if not ok:
                        caught[defect, dtype].append(f"{case.name}/{recipe} ({ratio:.3g}x)")
    print()
    for defect in AM.DEFECTS:
        for dtype in DTYPES:
            print(f"new criteria, {defect:20s} {dtype:4s}: fails on {', '.join(caught[defect, dtype]) or 'NOTHING'} (of {tried[defect, dtype]} tried)")
            assert caught[defect, dtype], f"{defect} / {dtype}: no case of the list fails its criterion"

    # the old criterion on its own ground: N(0,1) inputs, seed 60, scale 1/8, 256 queries, n_kv of the old shape lists
    print("old criterion (tensor-wide max-abs, 2^-7 / 2^-9 * max(1, |ref|max), N(0,1) inputs), per n_kv 77 / 545 / 1000 / 4096: P = passes, F = fails")
    table = {}
    for defect in AM.DEFECTS:
        row = []
        for dtype in DTYPES:
            verdicts = ""
            for n in (77, 545, 1000, 4096):
                causal = defect.startswith("causal")
                case = AM.Case("old", 0, 1, 1, n if causal else 256, n, recipes=("normal",), causal=causal)
                inp = AM.make_inputs(case, "normal", dtype)
                r = AM.reference(inp.q, inp.k, inp.v, n, 0.125, causal)
                out = AM.emulate(inp.q, inp.k, inp.v, n, 0.125, causal, dtype, defect=defect)
                verdicts += "P" if AM.old_criterion(out, r.ref, dtype)[0] else "F"
            row.append(verdicts)
        table[defect] = tuple(row)
        print(f"    {defect:20s} bf16 {row[0]}   f16 {row[1]}")
    assert table == AM.OLD_CRITERION_TABLE, "update attn_matrix.OLD_CRITERION_TABLE (documentation of what the old criterion let through)"
