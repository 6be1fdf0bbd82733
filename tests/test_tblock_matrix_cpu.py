"""The CPU half of the transformer block's kernel matrix (tests/tblock_matrix.py): every argument refusal of idb_layernorm_bwd /
idb_geglu_fwd / idb_geglu_bwd / idb_adamw_clip_step_table (return code, a message naming the argument, zero launches), the defect-free
emulations against every criterion with the worst err / bound printed, the teeth (each injected defect must fail the case named for it;
no defect-free case fails), and cosine_lr against its closed form.

Worst err / bound of the defect-free emulations (test_*_emulation_meets_criteria print them): every figure is below 1; the structured
elements (`integer`'s nonzero gradients, one_hot's zeros) are exact.  No constant of a criterion had to be raised."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import matrix_common as MC  # noqa: E402
import tblock_matrix as TM  # noqa: E402
from faceposegenerator_amd import _lib as L  # noqa: E402
from faceposegenerator_amd.lorablock import cosine_lr  # noqa: E402

DTYPES = MC.DTYPES
EUNSUPPORTED = -2


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def _unsupported(lib, call, ok):
    before = lib.idb_launch_count()
    for kw in MC.BAD_DTYPES + [dict(dtype=L.IDB_F32)]:
        assert call({**ok, **kw}) == EUNSUPPORTED and b"dtype" in lib.idb_last_error()
    assert lib.idb_launch_count() == before


def test_layernorm_bwd_refusals(lib):
    P, M = MC.P16, 1 << 24
    ok = dict(x=P, dy=P + M, add=P + 2 * M, gamma=P + 3 * M, dx=P + 4 * M, rows=5, c=320, eps=1e-5, dtype=L.IDB_F16)
    order = ("x", "dy", "add", "gamma", "dx", "rows", "c", "eps", "dtype")
    call = lambda kw: lib.idb_layernorm_bwd(*[kw[n] for n in order], None)       # noqa: E731
    for name in ("x", "dy", "gamma", "dx"):
        MC.refused(lib, call, ok, [{name: None}], f"{name} is null")
        MC.refused(lib, call, ok, [{name: ok[name] + 8}], f"{name} is not aligned")
    MC.refused(lib, call, ok, [dict(add=ok["add"] + 8)], "add is not aligned")
    MC.refused(lib, call, ok, [dict(rows=0), dict(rows=-1)], "rows")
    MC.refused(lib, call, ok, [dict(c=0), dict(c=100), dict(c=1544), dict(c=-8)], "c=")
    MC.refused(lib, call, ok, [dict(eps=0.0), dict(eps=-1.0), dict(eps=math.inf), dict(eps=math.nan)], "eps")
    MC.refused(lib, call, ok, [dict(rows=1 << 34)], "rows too large")
    MC.refused(lib, call, ok, [dict(dx=ok["x"]), dict(dx=ok["x"] + 16)], "dx aliases x")
    MC.refused(lib, call, ok, [dict(dx=ok["gamma"])], "dx aliases gamma")
    MC.refused(lib, call, ok, [dict(dx=ok["dy"] + 16)], "dx aliases dy")
    MC.refused(lib, call, ok, [dict(dx=ok["add"] + 16)], "dx aliases add")
    _unsupported(lib, call, ok)
    # accepted as far as the argument checks go: no add, dx on add, dx on dy (probed with the next refusal in line)
    for kw in (dict(add=None), dict(dx=ok["add"]), dict(dx=ok["dy"])):
        MC.refused(lib, call, {**ok, **kw}, [dict(rows=1 << 34)], "rows too large")


def test_geglu_refusals(lib):
    P, M = MC.P16, 1 << 26
    ok = dict(hg=P, hg_ld=512, dout=P + M, out=P + 2 * M, rows=3, inner=256, dtype=L.IDB_BF16)
    fwd = lambda kw: lib.idb_geglu_fwd(kw["hg"], kw["hg_ld"], kw["out"], kw["rows"], kw["inner"], kw["dtype"], None)       # noqa: E731
    bwd = lambda kw: lib.idb_geglu_bwd(kw["hg"], kw["hg_ld"], kw["dout"], kw["out"], kw["rows"], kw["inner"], kw["dtype"], None)       # noqa: E731
    for call, ptrs, outname in ((fwd, ("hg", "out"), "out"), (bwd, ("hg", "dout", "out"), "dhg")):
        for name in ptrs:
            shown = outname if name == "out" else name
            MC.refused(lib, call, ok, [{name: None}], f"{shown} is null")
            MC.refused(lib, call, ok, [{name: ok[name] + 4}], f"{shown} is not aligned")
        MC.refused(lib, call, ok, [dict(rows=0), dict(rows=-3)], "rows must be positive")
        MC.refused(lib, call, ok, [dict(inner=0), dict(inner=4), dict(inner=260), dict(inner=-8)], "inner must")
        MC.refused(lib, call, ok, [dict(hg_ld=504), dict(hg_ld=516), dict(hg_ld=0)], "hg_ld")
        MC.refused(lib, call, ok, [dict(rows=1 << 27)], "too large")
        MC.refused(lib, call, ok, [dict(out=ok["hg"]), dict(out=ok["hg"] + 512)], f"{outname} aliases hg")
        _unsupported(lib, call, ok)
    MC.refused(lib, bwd, ok, [dict(out=ok["dout"]), dict(out=ok["dout"] - 512)], "dhg aliases dout")


def _adam_ok():
    P, M = MC.P16, 1 << 20
    return dict(count=3, weights=P, grads=P + M, exp_avg=P + 2 * M, exp_avg_sq=P + 3 * M, numel=P + 4 * M, lr=1e-4, beta1=0.9, beta2=0.999, eps=1e-8,
                weight_decay=1e-2, max_norm=1.0, inv_scale=1.0, step=1, total_norm=P + 5 * M, skipped=P + 6 * M, ws=P + 7 * M, ws_bytes=3 * 8192)


def test_adamw_refusals(lib):
    ok = _adam_ok()
    order = tuple(ok)
    call = lambda kw: lib.idb_adamw_clip_step_table(*[kw[n] for n in order], None)       # noqa: E731
    MC.refused(lib, call, ok, [dict(count=0), dict(count=L.IDB_ADAMW_TABLE_MAX + 1), dict(count=-1)], "count")
    for name in ("weights", "grads", "exp_avg", "exp_avg_sq", "numel", "total_norm", "skipped", "ws"):
        MC.refused(lib, call, ok, [{name: None}], f"{name} is null")
        MC.refused(lib, call, ok, [{name: ok[name] + (2 if name == "skipped" else 4 if name != "ws" else 8)}], f"{name} is not aligned")
    nan = math.nan
    MC.refused(lib, call, ok, [dict(lr=-1e-4), dict(lr=1e5), dict(lr=nan)], "lr")
    MC.refused(lib, call, ok, [dict(beta1=1.0), dict(beta1=-0.1), dict(beta1=nan)], "beta1")
    MC.refused(lib, call, ok, [dict(beta2=1.0), dict(beta2=-0.1), dict(beta2=nan)], "beta2")
    MC.refused(lib, call, ok, [dict(eps=-1e-8), dict(eps=2.0), dict(eps=nan)], "eps")
    MC.refused(lib, call, ok, [dict(weight_decay=-1.0), dict(weight_decay=1e5), dict(weight_decay=nan)], "weight_decay")
    MC.refused(lib, call, ok, [dict(max_norm=0.0), dict(max_norm=-1.0), dict(max_norm=1e31), dict(max_norm=nan)], "max_norm")
    MC.refused(lib, call, ok, [dict(inv_scale=0.0), dict(inv_scale=-1.0), dict(inv_scale=math.inf), dict(inv_scale=nan)], "inv_scale")
    MC.refused(lib, call, ok, [dict(step=0), dict(step=-5)], "step")
    MC.refused(lib, call, ok, [dict(ws_bytes=0), dict(ws_bytes=3 * 8192 - 1)], "ws_bytes")
    for n in (1, 3, 16, L.IDB_ADAMW_TABLE_MAX):
        assert lib.idb_adamw_clip_table_workspace_bytes(n) == 8 * 1024 * n
    assert lib.idb_adamw_clip_table_workspace_bytes(0) == 0 and lib.idb_adamw_clip_table_workspace_bytes(L.IDB_ADAMW_TABLE_MAX + 1) == 0


# ---- the plans: what the cases cover ----------------------------------------------------------------------------------------------------
def test_cases_cover_the_issue():
    ln = TM.ln_cases()
    assert {c.c for c in ln} == set(TM.LN_C) and {c.rows for c in ln} == set(TM.LN_ROWS)
    assert {(c.c, c.rows) for c in ln if c.recipe == "normal"} == {(c, r) for c in TM.LN_C for r in TM.LN_ROWS}
    assert {c.recipe for c in ln} == set(TM.LN_RECIPES) and {c.add for c in ln} == {"none", "add", "alias"}
    assert {c.nch for c in ln} == {1, 2, 3} and any(c.rows % 4 and c.rows > 4 for c in ln)
    ge = TM.geglu_cases()
    assert {(c.inner, c.rows) for c in ge} >= {(i, r) for i in TM.GEGLU_INNER for r in TM.GEGLU_ROWS}
    totals = [c.rows * c.inner // 8 for c in ge]
    assert any(t < TM.GEGLU_BLOCK for t in totals) and any(t > TM.GEGLU_BLOCK and t % TM.GEGLU_BLOCK for t in totals) \
        and any(t % TM.GEGLU_BLOCK == 0 for t in totals)
    ad = TM.adam_cases()
    assert {c.tensors for c in ad} == {1, 3, 16} and {1, 2} < {c.step for c in ad} and max(c.step for c in ad) >= 10 ** 5
    assert {c.poison for c in ad} == {None, "inf", "nan"} and any(c.wd == 0 for c in ad) and any(c.inv_scale != 1 for c in ad)
    assert set(TM.ADAMW_NUMEL) == {1, 4, 255, 4097, 1280} and set(ad[-1].numel) == set(TM.ADAMW_NUMEL)
    clipped = set()
    for c in ad:
        if c.poison is None:
            _, g, _, _ = TM.adam_inputs(c)
            norm = c.inv_scale * math.sqrt(sum(float((a.astype(np.float64) ** 2).sum()) for a in g))
            clipped.add(norm > c.max_norm)
            if "clipped" in c.name:
                assert ("unclipped" in c.name) == (norm <= c.max_norm), (c.name, norm)
    assert clipped == {True, False}


# ---- LayerNorm backward -----------------------------------------------------------------------------------------------------------------
_LN = {}


def _ln(case, dt):
    if (case, dt) not in _LN:
        x, dy, add, gamma = TM.ln_inputs(case, dt)
        ref = TM.ln_reference(case, x, dy, add, gamma)
        _LN[(case, dt)] = (x, dy, add, gamma, ref, TM.ln_bound(case, ref, add, dt))
    return _LN[(case, dt)]


def _ln_verdict(case, dt, defect=None):
    x, dy, add, gamma, ref, bnd = _ln(case, dt)
    return MC.check(TM.ln_emulate(case, x, dy, add, gamma, dt, defect), ref["dx"], bnd)


def test_ln_emulation_meets_criteria():
    worst = MC.Worst("layernorm_bwd emulation")
    for case in TM.ln_cases():
        for dt in DTYPES:
            res = _ln_verdict(case, dt)
            assert res[0], MC.describe(f"{case.name}/{dt}", res)
            worst.note(f"{case.recipe:9s} {dt}", res[1], case.name)
    worst.show()


def test_ln_structured_recipes():
    """const_row: xhat is exactly 0 and rstd = 1 / sqrt(eps) in the reference; integer: the closed form 3/8 a s + q / 2 + add, met bit for
    bit by the emulation wherever it is not 0."""
    for case in TM.ln_cases():
        x, dy, add, gamma, ref, bnd = _ln(case, "bf16")
        if case.recipe == "const_row":
            assert not ref["xhat"].any() and np.allclose(ref["rstd"], 1.0 / math.sqrt(case.eps), rtol=1e-15)
        if case.recipe == "integer":
            assert (ref["mean"] == 0).all() and (ref["var"] == 1).all() and (ref["rstd"] == 0.5).all()
            assert (ref["dx"] * 8 == np.round(ref["dx"] * 8)).all() and np.abs(ref["dx"]).max() < 8
            assert (bnd[ref["dx"] != 0] == 0).all() and (ref["dx"] != 0).mean() > 0.5


LN_TEETH = {
    "no_mean_g": TM.LnCase(5, 72, "integer", "add"),
    "padded_count": TM.LnCase(5, 72, "integer", "add"),
    "clamped_summed": TM.LnCase(5, 72, "normal", "none"),
    "gamma_after_means": TM.LnCase(70, 320, "normal", "add"),
    "var_c_minus_1": TM.LnCase(3, 8, "normal", "none"),
    "no_add": TM.LnCase(5, 1536, "integer", "alias"),
    "skip_partial_workgroup": TM.LnCase(5, 64, "normal", "add"),
}


@pytest.mark.parametrize("defect", TM.LN_DEFECTS)
def test_ln_teeth(defect):
    case = LN_TEETH[defect]
    assert case in TM.ln_cases()
    for dt in DTYPES:
        assert _ln_verdict(case, dt)[0]
        res = _ln_verdict(case, dt, defect)
        assert not res[0], f"{defect} passes {case.name}/{dt} (worst ratio {res[1]:.3g})"


# ---- GEGLU ------------------------------------------------------------------------------------------------------------------------------
_GE = {}


def _ge(case, dt):
    if (case, dt) not in _GE:
        value, gate, dout = TM.geglu_inputs(case, dt)
        ref = TM.geglu_reference(value, gate, dout)
        _GE[(case, dt)] = (value, gate, dout, ref, TM.geglu_bound(ref, value, gate, dout, dt))
    return _GE[(case, dt)]


def _ge_verdicts(case, dt, defect=None):
    value, gate, dout, ref, bnd = _ge(case, dt)
    got = TM.geglu_emulate(case, value, gate, dout, dt, defect)
    return {n: MC.check(got[n], ref[n], bnd[n]) for n in ("out", "dvalue", "dgate")}


def test_geglu_emulation_meets_criteria():
    worst = MC.Worst("geglu emulation")
    for case in TM.geglu_cases():
        for dt in DTYPES:
            for n, res in _ge_verdicts(case, dt).items():
                assert res[0], MC.describe(f"{case.name}/{dt}/{n}", res)
                worst.note(f"{case.recipe:8s} {dt} {n}", res[1], case.name)
    worst.show()


def test_geglu_structured_recipes():
    """one_hot: every gradient off the one nonzero dout of a row is exactly 0 with a bound of 0; special: the tails of the derivative."""
    for case in TM.geglu_cases():
        value, gate, dout, ref, bnd = _ge(case, "f16")
        if case.recipe == "one_hot":
            off = dout == 0
            assert off.sum() == off.size - case.rows
            assert not ref["dvalue"][off].any() and not ref["dgate"][off].any() and not bnd["dvalue"][off].any() and not bnd["dgate"][off].any()
        if case.recipe == "special":
            assert set(np.unique(gate)) >= {0.0, 10.0, -10.0, 1.0, -1.0, 3.0, -3.0} and (np.abs(gate + 0.7518) < 1e-3).any()
            slope = ref["cdf"] + gate * ref["pdf"]
            assert np.abs(slope[gate == 10.0] - 1).max() < 1e-20 and np.abs(slope[gate == -10.0]).max() < 1e-20
            assert np.abs(slope[np.abs(gate + 0.7518) < 1e-3]).max() < 2e-3               # the minimum of GELU: the derivative vanishes


GEGLU_TEETH = {
    "halves_swapped": (TM.GegluCase(3, 1280, "normal", pad=16), ("out", "dvalue", "dgate")),
    "tanh_gelu": (TM.GegluCase(3, 1280, "special", pad=16), ("out", "dvalue", "dgate")),
    "no_gate_pdf": (TM.GegluCase(3, 1280, "special", pad=16), ("dgate",)),
    "tail_block_unprocessed": (TM.GegluCase(3, 1280, "one_hot", pad=16), ("out", "dvalue", "dgate")),
}


@pytest.mark.parametrize("defect", TM.GEGLU_DEFECTS)
def test_geglu_teeth(defect):
    case, must_fail = GEGLU_TEETH[defect]
    assert case in TM.geglu_cases()
    for dt in DTYPES:
        assert all(v[0] for v in _ge_verdicts(case, dt).values())
        got = _ge_verdicts(case, dt, defect)
        for n in must_fail:
            assert not got[n][0], f"{defect} passes {case.name}/{dt}/{n} (worst ratio {got[n][1]:.3g})"
    if defect == "tail_block_unprocessed":           # a total below one workgroup is all tail
        assert not any(v[0] for v in _ge_verdicts(TM.GegluCase(3, 8, "normal"), "f16", defect).values())


# ---- AdamW ------------------------------------------------------------------------------------------------------------------------------
_AD = {}


def _ad(case):
    if case.name not in _AD:
        st = TM.adam_inputs(case)
        _AD[case.name] = (st, TM.adam_oracle(case, *st))
    return _AD[case.name]


def _ad_verdict(case, defect=None):
    """(ok, worst err / ulp, detail) of the emulation against the oracle: w, m, v, the norm and the skip flag."""
    (w, g, m, v), (ow, om, ov, onorm, oskip) = _ad(case)
    ew, em, ev, enorm, eskip = TM.adam_emulate(case, w, g, m, v, defect)
    if oskip:
        same = eskip and all(MC.bit_equal(a, b)[0] for got, was in ((ew, w), (em, m), (ev, v)) for a, b in zip(got, was))
        return same and not math.isfinite(enorm), 0.0, "skipped"
    ok = (not eskip) and abs(enorm - onorm) <= TM.adam_norm_bound(case, onorm)
    worst, where = 0.0, ""
    for name, got, want in (("w", ew, ow), ("m", em, om), ("v", ev, ov)):
        o, r, at = TM.adam_verdict(name, got, want)
        ok &= o
        if r >= worst:
            worst, where = r, at
    return ok, worst, where


def test_adamw_emulation_meets_criteria():
    worst = MC.Worst("adamw emulation", ratio="err / ulp")
    for case in TM.adam_cases():
        ok, ratio, where = _ad_verdict(case)
        assert ok, (case.name, ratio, where)
        worst.note(case.name, ratio, where)
    worst.show()


ADAM_TEETH = {"bias_step_minus_1": "three_step2_clipped", "coupled_decay": "three_step2_clipped", "eps_inside_root": "sixteen_large_step",
              "clip_after_moments": "three_step2_clipped", "skip_still_decays": "three_inf"}


@pytest.mark.parametrize("defect", TM.ADAM_DEFECTS)
def test_adamw_teeth(defect):
    case = {c.name: c for c in TM.adam_cases()}[ADAM_TEETH[defect]]
    assert _ad_verdict(case)[0]
    ok, ratio, where = _ad_verdict(case, defect)
    assert not ok, f"{defect} passes {case.name} (worst {ratio:.3g} ulp)"
    if defect == "bias_step_minus_1":                # at step 1 the defect divides by zero
        assert not _ad_verdict(TM.adam_cases()[0], defect)[0]


def test_teeth_cover_every_defect():
    assert set(LN_TEETH) == set(TM.LN_DEFECTS) and set(GEGLU_TEETH) == set(TM.GEGLU_DEFECTS) and set(ADAM_TEETH) == set(TM.ADAM_DEFECTS)


# ---- the schedule -----------------------------------------------------------------------------------------------------------------------
def test_cosine_lr_closed_form():
    """diffusers' get_cosine_schedule_with_warmup (num_cycles = 0.5): linear warm-up, then 0.5 (1 + cos(pi progress))."""
    assert cosine_lr(0, 100) == 1.0 and cosine_lr(100, 100) == pytest.approx(0.0, abs=1e-16) and cosine_lr(50, 100) == pytest.approx(0.5, abs=1e-15)
    for total, warm in ((100, 0), (400, 50), (8, 0), (10, 10), (1, 0)):
        for step in range(total + 1):
            want = step / max(1, warm) if step < warm else 0.5 * (1 + math.cos(math.pi * (step - warm) / max(1, total - warm)))
            assert cosine_lr(step, total, warm) == pytest.approx(max(0.0, want), abs=1e-15), (step, total, warm)
    assert [cosine_lr(s, 400, 50) for s in (0, 25, 50)] == [0.0, 0.5, 1.0]
    vals = [cosine_lr(s, 400, 50) for s in range(50, 401)]
    assert all(a >= b for a, b in zip(vals, vals[1:]))
