"""The CPU half of idb_groupnorm_bwd's matrix (tests/gnbwd_matrix.py): every argument refusal through the ABI (return code, a message naming
the argument, zero launches: validation precedes any HIP call), the plan query against the pure-Python statement of its rules, the
defect-free emulation under the criterion with the worst err / bound printed per recipe, the structured recipes' closed forms, and the
teeth: each injected defect must fail the case named for it in both dtypes, and no defect-free case fails.

Worst err / bound of the defect-free emulation (test_emulation_meets_criterion prints them): below 1 on every recipe; `integer`'s nonzero
gradients are exact.  No constant of the criterion had to be raised."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gnbwd_matrix as GM  # noqa: E402
import matrix_common as MC  # noqa: E402
import norm_matrix as NM  # noqa: E402
from faceposegenerator_amd import _lib as L  # noqa: E402

DTYPES = MC.DTYPES
EUNSUPPORTED = -2
ORDER = ("x0", "c0", "x1", "c1", "stat_partials", "stat_chunks", "dy", "add", "gamma", "beta", "eps", "silu", "dx0", "dx1", "batch", "hw", "groups", "dtype",
         "workspace", "workspace_bytes")


def _ok(two=False):
    P, M = MC.P16, 1 << 26
    d = dict(x0=P, c0=640, x1=None, c1=0, stat_partials=P + M, stat_chunks=3, dy=P + 2 * M, add=P + 3 * M, gamma=P + 4 * M, beta=P + 5 * M, eps=1e-5,
             silu=1, dx0=P + 6 * M, dx1=None, batch=2, hw=100, groups=32, dtype=L.IDB_F16, workspace=P + 7 * M, workspace_bytes=2 * 64 * 32 * 8)
    if two:
        d.update(x1=P + 8 * M, c1=320, dx1=P + 9 * M)
    return d


def test_refusals(lib):
    call = lambda kw: lib.idb_groupnorm_bwd(*[kw[n] for n in ORDER], None)       # noqa: E731
    for two in (False, True):
        ok = _ok(two)
        for name in ("x0", "stat_partials", "dy", "gamma", "beta", "dx0", "workspace"):
            MC.refused(lib, call, ok, [{name: None}], f"{name} is null")
            MC.refused(lib, call, ok, [{name: ok[name] + 8}], f"{name} is not aligned")
        MC.refused(lib, call, ok, [dict(add=ok["add"] + 8)], "add is not aligned")
        MC.refused(lib, call, ok, [dict(batch=0), dict(batch=-1)], "batch")
        MC.refused(lib, call, ok, [dict(batch=65536, workspace_bytes=1 << 40)], "unsupported geometry")
        MC.refused(lib, call, ok, [dict(hw=0), dict(hw=-4)], "hw")
        MC.refused(lib, call, ok, [dict(groups=0), dict(groups=-32)], "groups")
        MC.refused(lib, call, ok, [dict(c0=0), dict(c0=100), dict(c0=-8)], "c0=")
        MC.refused(lib, call, ok, [dict(c1=4), dict(c1=-8)], "c1=")
        MC.refused(lib, call, ok, [dict(groups=7), dict(groups=33)], "groups=")
        MC.refused(lib, call, ok, [dict(groups=ok["c0"] + ok["c1"])], "fewer than 2 channels per group")
        MC.refused(lib, call, ok, [dict(stat_chunks=0), dict(stat_chunks=65), dict(stat_chunks=-1)], "stat_chunks")
        MC.refused(lib, call, ok, [dict(eps=0.0), dict(eps=-1.0), dict(eps=math.inf), dict(eps=math.nan)], "eps")
        MC.refused(lib, call, ok, [dict(silu=2), dict(silu=-1)], "silu")
        MC.refused(lib, call, ok, [dict(workspace_bytes=0), dict(workspace_bytes=ok["workspace_bytes"] - 1)], "workspace_bytes")
        MC.refused(lib, call, ok, [dict(dx0=ok["x0"]), dict(dx0=ok["x0"] + 16)], "dx0 aliases x0")
        MC.refused(lib, call, ok, [dict(dx0=ok["dy"] + 16)], "dx0 aliases dy")
        MC.refused(lib, call, ok, [dict(dx0=ok["add"] + 16)], "dx0 aliases add")
        MC.refused(lib, call, ok, [dict(dx0=ok["gamma"])], "dx0 aliases gamma")
        MC.refused(lib, call, ok, [dict(dx0=ok["beta"] - 16)], "dx0 aliases beta")
        MC.refused(lib, call, ok, [dict(dx0=ok["workspace"])], "dx0 aliases workspace")
        MC.refused(lib, call, ok, [dict(dx0=ok["stat_partials"])], "dx0 aliases stat_partials")
        before = lib.idb_launch_count()
        for kw in MC.BAD_DTYPES + [dict(dtype=L.IDB_F32)]:
            assert call({**ok, **kw}) == EUNSUPPORTED and b"dtype" in lib.idb_last_error()
        assert lib.idb_launch_count() == before
    one, two = _ok(False), _ok(True)
    MC.refused(lib, call, one, [dict(x1=two["x1"])], "x1 must be given exactly when c1 > 0")
    MC.refused(lib, call, one, [dict(dx1=two["dx1"])], "dx1 must be given exactly when c1 > 0")
    MC.refused(lib, call, two, [dict(x1=None)], "x1 must be given exactly when c1 > 0")
    MC.refused(lib, call, two, [dict(dx1=None)], "dx1 must be given exactly when c1 > 0")
    MC.refused(lib, call, two, [dict(x1=two["x1"] + 8)], "x1 is not aligned")
    MC.refused(lib, call, two, [dict(dx1=two["dx1"] + 8)], "dx1 is not aligned")
    MC.refused(lib, call, two, [dict(dx1=two["x1"])], "dx1 aliases x1")
    MC.refused(lib, call, two, [dict(dx1=two["dy"])], "dx1 aliases dy")
    MC.refused(lib, call, two, [dict(dx0=two["dy"])], "dx0 aliases dy")               # whole-tensor aliasing needs one source
    MC.refused(lib, call, two, [dict(dx0=two["add"])], "dx0 aliases add")
    MC.refused(lib, call, two, [dict(dx1=two["dx0"])], "dx0 aliases dx1")
    # accepted as far as the argument checks go: no add, dx0 on add, dx0 on dy (probed with the next refusal in line)
    for kw in (dict(add=None), dict(dx0=one["add"]), dict(dx0=one["dy"])):
        MC.refused(lib, call, {**one, **kw}, [dict(workspace_bytes=8)], "workspace_bytes")
    assert lib.idb_groupnorm_bwd_workspace_bytes(2, 100, 32) == 2 * 64 * 32 * 8 and lib.idb_groupnorm_bwd_workspace_bytes(0, 100, 32) == 0


def test_plan_query_matches_its_rules(lib):
    """Every case's geometry, a sweep of shapes, and the refusals of the query itself."""
    shapes = [(c.c0, c.c1, c.batch, c.hw, c.groups) for c in GM.cases()]
    shapes += [(c0, c1, b, hw, g) for (c0, c1, g) in GM.SHAPES + ((96, 0, 32), (160, 0, 32), (512, 0, 8), (64, 0, 1), (24, 40, 32), (2560, 0, 32), (8192, 0, 2))
               for b in (1, 2, 8, 64) for hw in (1, 2, 49, 50, 51, 256, 3201, 4096, 16384)]
    seen = set()
    for c0, c1, b, hw, g in shapes:
        rc, p = GM.plan(lib, c0, c1, b, hw, g)
        if not GM.py_supported(c0, c1, b, hw, g):
            assert rc == MC.EINVAL, (c0, c1, b, hw, g)
            continue
        assert rc == 0 and p == GM.py_plan(c0, c1, b, hw, g), (c0, c1, b, hw, g, p, GM.py_plan(c0, c1, b, hw, g))
        assert p.sw * p.slices == c0 + c1 and p.sw % ((c0 + c1) // g) == 0 and p.sw % 8 == 0 and 1 <= p.chunks <= 64 and p.chunks * p.chunk_len >= hw
        seen.add((p.sw, p.chunks > 1, p.chunks * p.chunk_len > hw))
    assert {s[0] for s in seen} >= {8, 64, 80, 120} and {s[1:] for s in seen} >= {(False, False), (True, False), (True, True)}
    assert any(not GM.py_supported(*s) for s in shapes)                       # 8192 channels in 2 groups: a 4096-channel slice has 512 vector columns
    # below its large-tensor threshold the forward's two-launch geometry is the same
    for c0, c1, b, hw, g in shapes[:40]:
        f = NM.plan(lib, c0, c1, b, hw, g)[1]
        p = GM.plan(lib, c0, c1, b, hw, g)[1]
        assert (f.sw, f.slices, f.chunks, f.chunk_len) == (p.sw, p.slices, p.chunks, p.chunk_len)
    P = [L.C.c_int32() for _ in range(5)]
    ref = [L.C.byref(v) for v in P]
    for bad in ((0, 0, 2, 100, 32), (640, 4, 2, 100, 32), (640, 0, 0, 100, 32), (640, 0, 2, 0, 32), (640, 0, 2, 100, 0), (640, 0, 2, 100, 7), (64, 0, 2, 100, 64)):
        assert lib.idb_groupnorm_bwd_plan(*bad, *ref) == MC.EINVAL and lib.idb_last_error()
    assert lib.idb_groupnorm_bwd_plan(640, 0, 2, 100, 32, None, *ref[1:]) == MC.EINVAL and b"null" in lib.idb_last_error()


def test_cases_cover_the_issue(lib):
    cs = GM.cases()
    normal = {(c.c0, c.c1, c.groups, c.hw) for c in cs if c.recipe == "normal"}
    assert normal >= {(c0, c1, g, hw) for (c0, c1, g) in GM.SHAPES for hw in GM.HWS}
    cross = {(c.c0, c.c1, c.groups, c.hw, c.batch) for c in cs if c.recipe == "normal" and c.stat == "device"}
    assert cross >= {(c0, c1, g, hw, b) for (c0, c1, g) in GM.SHAPES for hw in GM.HWS for b in GM.BATCHES} and len(cross) >= 135
    assert {(c.silu, c.add) for c in cs if c.recipe == "normal"} >= {(s, a) for s in (0, 1) for a in ("add", "none")}
    for c0, c1, g in GM.SHAPES:
        assert {c.batch for c in cs if (c.c0, c.c1, c.groups) == (c0, c1, g)} == {1, 2, 3}, (c0, c1)
    for hw in GM.HWS:
        assert {c.batch for c in cs if c.hw == hw} == {1, 2, 3}
    assert {c.recipe for c in cs} == set(GM.RECIPES) and {c.silu for c in cs} == {0, 1} and {c.add for c in cs} == set(GM.ADD_MODES)
    assert all(c.c1 == 0 for c in cs if c.add in ("alias", "alias_dy"))
    # a statistics chunk count that is not the backward's own
    differ = [c for c in cs if c.stat == "hw64" and c.stat_chunks != GM.plan(lib, c.c0, c.c1, c.batch, c.hw, c.groups)[1].chunks]
    assert differ and all(c.hw % 64 == 0 for c in cs if c.stat == "hw64")
    for recipe in GM.RECIPES[1:]:
        mine = [c for c in cs if c.recipe == recipe]
        plans = [GM.plan(lib, c.c0, c.c1, c.batch, c.hw, c.groups)[1] for c in mine]
        assert any(p.chunks > 1 and p.chunks * p.chunk_len > c.hw for c, p in zip(mine, plans)), recipe      # a ragged last chunk
        assert any(c.hw == 1 for c in mine) and any(c.c1 for c in mine) and any(p.sw == 120 for p in plans) and any(c.cpg == 2 for c in mine)


_PROBLEM = {}


def _problem(lib, case, dt):
    if (case, dt) not in _PROBLEM:
        inp = GM.inputs(case, dt)
        ref = GM.reference(case, inp)
        fwd = GM.forward_plan(lib, case)
        own = GM.plan(lib, case.c0, case.c1, case.batch, case.hw, case.groups)[1]
        stat = GM.host_partials(inp["x"], case.groups, case.stat_chunks or fwd.chunks)
        _PROBLEM[(case, dt)] = (inp, ref, own, stat, GM.bound(case, ref, inp, dt, NM.gn_depth(fwd), own))
    return _PROBLEM[(case, dt)]


def _verdict(lib, case, dt, defect=None):
    inp, ref, own, stat, bnd = _problem(lib, case, dt)
    stale = None
    if defect == "stale_partial":
        stale = GM.emulate_sums(case, GM.inputs(case, dt, seed=82), stat, own)
    return GM.judge(case, ref, bnd, *GM.emulate(case, inp, stat, own, dt, defect, stale))


def test_emulation_meets_criterion(lib):
    worst = MC.Worst("groupnorm_bwd emulation")
    for case in GM.cases():
        for dt in DTYPES:
            ok, ratio, text = _verdict(lib, case, dt)
            assert ok, f"{dt}: {text}"
            worst.note(f"{case.recipe:14s} {dt}", ratio, case.name)
        if case.batch * case.hw * case.c > 1 << 20:
            for dt in DTYPES:
                _PROBLEM.pop((case, dt), None)               # the large cases' float64 arrays are not kept
    worst.show()


def test_structured_recipes(lib):
    for case in GM.cases():
        if case.recipe not in GM.EXACT_SUMS:
            continue
        inp, ref, own, stat, bnd = _problem(lib, case, "bf16")
        if case.recipe in ("constant_group", "silu_special"):
            assert not ref["xhat"].any() and not ref["var"].any() and np.allclose(ref["rstd"], 1.0 / math.sqrt(GM.eps32(case.eps)), rtol=1e-15)
            mean, rstd = GM.emulate_forward_stats(stat, case.hw, case.cpg, case.eps)
            assert np.array_equal(np.repeat(mean, case.cpg, axis=1)[:, None, :] * np.ones_like(inp["x"]), inp["x"])       # the mean is exact
        if case.recipe == "silu_special":
            assert {float(v) for v in np.unique(ref["y"])} == {float(np.float32(v)) for v in GM.SPECIAL_Y}
            f = ref["f"]
            assert abs(f[ref["y"] == 0].max() - 0.5) < 1e-15 and np.abs(f[ref["y"] == -10.0]).max() < 5e-4 and np.abs(f[ref["y"] == 10.0] - 1).max() < 5e-4
            assert abs(f.max() - 1.09984) < 1e-4 and np.abs(f[np.abs(ref["y"] + 1.2785) < 1e-3]).max() < 1e-4          # SiLU's minimum: f = 0
        if case.recipe == "integer":
            assert not ref["mean"].any() and (ref["var"] == 1).all() and (ref["rstd"] == 0.5).all()
            assert (ref["dx"] * 8 == np.round(ref["dx"] * 8)).all() and np.abs(ref["dx"]).max() < 8
            assert (bnd[ref["dx"] != 0] == 0).all() and (ref["dx"] != 0).mean() > 0.5


@pytest.mark.parametrize("defect", GM.DEFECTS)
def test_teeth(lib, defect):
    case = GM.DEFECT_CASE[defect]
    assert case in GM.cases()
    for dt in DTYPES:
        assert _verdict(lib, case, dt)[0]
        ok, ratio, text = _verdict(lib, case, dt, defect)
        assert not ok, f"{defect} passes {case.name}/{dt} (worst ratio {ratio:.3g})"


def test_teeth_cover_every_defect():
    assert set(GM.DEFECT_CASE) == set(GM.DEFECTS) and len(GM.DEFECTS) == 13
