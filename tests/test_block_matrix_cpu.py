"""The CPU half of the trunk kernels' per-entry test matrix (tests/block_matrix.py), no GPU: every plan figure the cases were chosen
for, asserted through the library's host-only queries (idb_blk_conv_workspace_bytes, idb_blk_bn_workspace_bytes) against the plan
restated in Python; what the input recipes plant; the float64 references against the oracle's own pieces; the teeth (every defect of
block_matrix.DEFECTS fails its named case, every unmodified emulation meets its bound within its share: half, or whole where the
module docstring says the quantity is a single rounding); and the argument checks of every entry, which answer before any HIP call."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import block_matrix as M  # noqa: E402
import frblock_oracle as BO  # noqa: E402
import matrix_common as MC  # noqa: E402

F32, F64 = np.float32, np.float64
W = MC.Worst("block matrix, emulation")
WHOLE = ("sc", "sh", "running_mean", "running_var", "gamma", "beta", "slope", "gc")       # single roundings: asked whole


# ---- plans ---------------------------------------------------------------------------------------------------------------------------
def test_cases_are_the_issues():
    assert len(M.CONV_CASES) == 12 and set(M.CONV_REACHES) == set(M.CONV_CASES)
    assert M.BN_ROWS == tuple(sorted(M.BN_PLAN)) and len(M.bn_cases()) == 14
    assert all(ch == 64 for r, ch in M.bn_cases() if r in M.BN_CAP_ROWS)
    assert M.col_tile(64) == 64 and M.col_tile(128) == 128 and M.col_tile(192) == 64 and M.col_tile(256) == 128 and M.col_tile(512) == 128


@pytest.mark.parametrize("case", M.CONV_CASES, ids=str)
def test_conv_plan_figures_through_the_library(lib, case):
    p, g = M.conv_plan(case), M.conv_geo(case)
    for k, v in M.CONV_REACHES[case].items():
        assert p[k] == v, (case, k, p[k], v)
    if case in M.CONV_MO:
        assert g["Mo"] == M.CONV_MO[case]
    sl, rt = C.c_int32(-1), C.c_int32(-1)
    need = lib.idb_blk_conv_workspace_bytes(*case, C.byref(sl), C.byref(rt))
    # the slice count depends on the column tile (256 / (K tiles x column tiles) workgroups): the restated rule is cross-checked here
    assert (need, sl.value, rt.value) == (p["bytes"], p["slices"], p["dgrad_row_tiles"]), (case, need, sl.value, rt.value, p)
    assert p["last_slice_rows"] >= 1 and (p["slices"] - 1) * p["per"] * M.TK < g["Mo"]
    assert max(p["class_rows"]) == p["class_rows"][0] and sum(p["class_rows"]) == case[0] * case[1] * case[2]


def test_conv_cases_reach_what_they_are_for():
    plans = {c: M.conv_plan(c) for c in M.CONV_CASES}
    assert max(p["fwd_col_tiles"] for p in plans.values()) == 3 and max(p["dgrad_col_tiles"] for p in plans.values()) == 3
    assert any(p["fwd_col_tiles"] == 2 and M.col_tile(c[4]) == 128 for c, p in plans.items())
    assert any(p["dgrad_col_tiles"] == 2 and M.col_tile(c[3]) == 128 for c, p in plans.items())
    assert all(M.conv_geo(c)["Ho"] != M.conv_geo(c)["Wo"] for c in M.CONV_CASES)                 # no square output map
    assert all(c[1] != c[2] for c in M.CONV_CASES)
    assert max(p["slices"] for p in plans.values()) == M.MAX_WSLICES
    assert any(0 < p["last_slice_rows"] % M.TK < p["last_slice_rows"] or p["last_slice_rows"] < M.TK for p in plans.values())
    assert any(0 in p["class_rows"] for p in plans.values())
    assert M.no_tap_mask(M.CONV_CASES[3]).sum() == 5 * 4 - 3 * 2 and not M.no_tap_mask(M.CONV_CASES[1]).any()
    assert 1728 % M.TM != 0 and 36 < M.TM


@pytest.mark.parametrize("rows", M.BN_ROWS)
def test_bn_plan_figures_through_the_library(lib, rows):
    for ch in M.BN_CH:
        p = M.bn_plan(rows, ch)
        assert (p["per"], p["slices"], p["last"]) == M.BN_PLAN[rows]
        sl = C.c_int32(-1)
        assert lib.idb_blk_bn_workspace_bytes(rows, ch, C.byref(sl)) == p["bytes"] and sl.value == p["slices"]
    assert (M.BN_PLAN[16385][1] > 64, M.BN_PLAN[33275][1] > 128, M.BN_PLAN[262145][0] > 256, M.BN_PLAN[307193][1]) == (True, True, True, 1024)
    assert lib.idb_blk_bn_workspace_bytes(0, 64, None) == 0 and lib.idb_blk_bn_workspace_bytes(2, 96, None) == 0
    assert lib.idb_blk_conv_workspace_bytes(2, 3, 5, 32, 64, 3, 1, None, None) == 0


# ---- recipes -------------------------------------------------------------------------------------------------------------------------
def test_recipes_are_exact_fp32_and_plant_what_they_say():
    for case in M.CONV_CASES[:3]:
        for a in M.conv_inputs(case):
            assert np.array_equal(a, a.astype(F32).astype(F64))
    x, prm = M.bn_inputs(257, 64)
    assert np.array_equal(x, x.astype(F32).astype(F64))
    col = x[:, M.OFFSET_CH]
    assert 9999.9 < col.min() and col.max() < 10000.1 and 5e-3 < np.ptp(col) < 3e-2
    assert (M.bn_inputs(257, 64, "const")[0][:, M.CONST_CH] == 1.25).all() and np.isinf(M.bn_inputs(257, 64, "inf")[0]).sum() == 1
    i = M.bnb_inputs(2, 64)
    y = i["c"] * i["affine"][0] + i["affine"][1]
    assert (y[:, M.Y0_CH] == 0).all() and y[0, M.TINY_CH] == 2.0 ** -126 and y[1, M.TINY_CH] == -(2.0 ** -126)
    assert np.array_equal(i["c"], i["c"].astype(F32).astype(F64)) and i["g"][0, M.Y0_CH] > 0 > i["g"][1, M.Y0_CH]
    big = M.bnb_inputs(257, 192)
    y = big["c"] * big["affine"][0] + big["affine"][1]
    assert (y > 0).mean() > 0.2 and (y < 0).mean() > 0.2 and np.array_equal(M.fma32(big["c"].astype(F32), np.broadcast_to(
        big["affine"][0].astype(F32), y.shape), np.broadcast_to(big["affine"][1].astype(F32), y.shape)).reshape(y.shape), y.astype(F32))
    assert (big["add"] < 0).any() and (big["add"] > 0).any()


def test_bn_reference_is_the_oracles_where_the_oracle_is_accurate():
    x, prm = M.bn_inputs(257, 192)
    val, bound = M.bn_forward_reference(x, prm)
    st, af, _, run = BO.bn_forward(x, prm, "bn")
    keep = np.arange(192) != M.OFFSET_CH
    assert np.allclose(val["mean"][keep], st[0][keep], rtol=0, atol=1e-14) and np.allclose(val["invstd"], st[1], rtol=1e-9)
    assert np.allclose(val["sc"], af[0], rtol=1e-9) and np.allclose(val["running_var"], run["bn.running_var"], rtol=1e-12)
    assert bound["mean"][M.OFFSET_CH] < 2e-12 and abs(val["mean"][M.OFFSET_CH] - 1e4) < 1e-2


# ---- teeth ---------------------------------------------------------------------------------------------------------------------------
def test_defect_list_is_complete():
    assert set(M.DEFECT_CASES) == set(M.DEFECTS) and len(M.DEFECTS) == 20 and M.HARMLESS == ()


@pytest.mark.parametrize("defect", M.DEFECTS)
def test_every_defect_fails_its_named_case(defect):
    assert M.defect_fails(defect), (defect, M.DEFECT_CASES[defect])


def _emulated_mode(n, case):
    modes = M.conv_modes(case)
    return modes if n < 2 else (modes[n % len(modes)],)


@pytest.mark.parametrize("n,case", list(enumerate(M.CONV_CASES)), ids=lambda v: str(v))
def test_conv_emulations_pass(n, case):
    for mode in _emulated_mode(n, case):
        for op in ("fwd", "dgrad", "wgrad"):
            if op == "dgrad" and (case[3] == 4 or mode != M.conv_modes(case)[0]):
                continue
            ref, bound = M.conv_reference(case, mode, op)
            emu = M.emulate_conv_dgrad(case) if op == "dgrad" else (M.emulate_conv_fwd if op == "fwd" else M.emulate_conv_wgrad)(case, mode)
            res = M.check(emu, ref, bound)
            assert res[0] and res[1] <= 0.5, M.describe(f"{op} {case} {mode}", res)
            W.note(f"conv {op}", res[1])
            if op == "dgrad":
                zero = np.broadcast_to(M.no_tap_mask(case)[None, :, :, None], emu.shape)
                assert (emu.view(np.uint32)[zero] == 0).all() and (bound[zero] == 0).all() and (bound[~zero] > 0).all()


@pytest.mark.parametrize("rows,ch", [c for c in M.bn_cases() if c[1] == 64 or c[0] in (2, 257)])
def test_bn_forward_emulation_passes(rows, ch):
    x, prm = M.bn_inputs(rows, ch)
    ref, bound = M.bn_forward_reference(x, prm)
    emu = M.emulate_bn_forward(x, prm)
    ok, res = M.judge_all(emu, ref, bound)
    for k, r in res.items():
        assert r[0] and r[1] <= (1.0 if k in WHOLE else 0.5), M.describe(f"bn forward {rows} x {ch} {k}", r)
        W.note(f"bn forward {k}", r[1])
    assert emu["flags"] == (0, 0)


def test_bn_forward_emulation_flags_and_eval():
    x, prm = M.bn_inputs(257, 64, "const")
    emu = M.emulate_bn_forward(x, prm, eps=0.0)
    ref, bound = M.bn_forward_reference(x, prm, eps=0.0)
    assert emu["flags"] == (0, 1)
    keep = np.arange(64) != M.CONST_CH
    for k in ref:
        assert M.check(emu[k][keep], ref[k][keep], bound[k][keep])[0], k
    x, prm = M.bn_inputs(257, 64, "inf")
    assert M.emulate_bn_forward(x, prm)["flags"] == (1, 0)
    x, prm = M.bn_inputs(2, 64)
    ref, bound = M.bn_forward_reference(x[:1], prm, training=False)
    assert M.judge_all(M.emulate_bn_forward(x[:1], prm, training=False), ref, bound)[0] and (bound["mean"] == 0).all()
    for mom in (0.0, 1.0):
        ref, bound = M.bn_forward_reference(x, prm, momentum=mom)
        assert M.judge_all(M.emulate_bn_forward(x, prm, momentum=mom), ref, bound)[0]
        if mom == 0.0:
            assert np.array_equal(ref["running_mean"], prm["bn.running_mean"])


@pytest.mark.parametrize("rows,ch", [c for c in M.bn_cases() if c[1] == 64 or c[0] in (2, 257)])
def test_bn_backward_emulation_passes(rows, ch):
    for form in (M.BNB_FORMS if rows <= 257 else M.BNB_FORMS[3:]):
        ref, bound = M.bn_backward_reference(rows, ch, *form)
        ok, res = M.judge_all(M.emulate_bn_backward(rows, ch, *form), ref, bound)
        for k, r in res.items():
            assert r[0], M.describe(f"bn backward {rows} x {ch} {form} {k}", r)          # every output is a single rounding: whole
            W.note(f"bn backward {k}", r[1])
    if rows == 2:
        ref, _ = M.bn_backward_reference(rows, ch, True, False)
        assert ref["slope"][M.Y0_CH] == 0.0                                              # y == 0: d slope gets nothing


@pytest.mark.parametrize("rows,ch", [(2, 64), (257, 192)])
def test_affine_emulation_passes(rows, ch):
    for form in M.AFFINE_FORMS:
        ref, bound = M.affine_reference(rows, ch, *form)
        res = M.check(M.emulate_affine(rows, ch, *form), ref, bound)
        assert res[0], M.describe(f"affine {rows} x {ch} {form}", res)                    # single roundings: whole
        W.note("affine", res[1])


def test_pack_emulation_is_the_copy():
    for shape in M.PACK_SHAPES:
        ref = M.pack_reference(shape)
        assert np.array_equal(M.emulate_pack(shape).view(np.uint32), ref.view(np.uint32)) and (ref[..., 3].view(np.uint32) == 0).all()
    assert [b * h * w for b, h, w in M.PACK_SHAPES] == [1, 15, 510, 768]


def test_summary():
    W.show()


# ---- argument checks: every IDB_REQUIRE answers before any HIP call --------------------------------------------------------------------
P16, OFF = MC.P16, MC.OFF


def _desc(a):
    from faceposegenerator_amd import _lib as L
    d = L.BlkConvDesc()
    for k in ("b", "h", "w", "cin", "cout", "ksize", "stride", "x", "affine", "slope", "weight"):
        setattr(d, k, a[k])
    return d


CONV_OK = dict(b=2, h=3, w=5, cin=64, cout=64, ksize=3, stride=1, x=P16, affine=P16, slope=P16, weight=P16, out=P16, g_out=P16, g_in=P16,
               d_weight=P16, ws=P16, ws_bytes=1 << 30)
DESC_BAD = [dict(x=OFF), dict(weight=OFF), dict(affine=OFF), dict(slope=OFF)]


def test_conv_argument_checks(lib):
    fwd = lambda a: lib.idb_blk_conv_forward(C.byref(_desc(a)), a["out"], None)                                        # noqa: E731
    dgr = lambda a: lib.idb_blk_conv_dgrad(C.byref(_desc(a)), a["g_out"], a["g_in"], None)                              # noqa: E731
    wgr = lambda a: lib.idb_blk_conv_wgrad(C.byref(_desc(a)), a["g_out"], a["d_weight"], a["ws"], a["ws_bytes"], None)  # noqa: E731
    for name, f in (("forward", fwd), ("dgrad", dgr), ("wgrad", wgr)):
        MC.refused(lib, f, CONV_OK, DESC_BAD, f"idb_blk_conv_{name}: x, weight, affine and slope 16-byte aligned")
        MC.refused(lib, f, CONV_OK, [dict(affine=None)], f"idb_blk_conv_{name}: a PReLU slope without")
        MC.refused(lib, f, CONV_OK, [dict(x=None), dict(weight=None)], f"idb_blk_conv_{name}: null pointer")
        MC.refused(lib, f, CONV_OK, [dict(cin=32), dict(cin=8), dict(cout=32), dict(h=129), dict(w=0), dict(b=1025), dict(ksize=2), dict(stride=3)],
                 f"idb_blk_conv_{name}: b in 1..1024")
    MC.refused(lib, fwd, CONV_OK, [dict(out=OFF), dict(out=None)], "idb_blk_conv_forward: out null or not 16-byte aligned")
    MC.refused(lib, dgr, CONV_OK, [dict(g_out=OFF), dict(g_in=OFF), dict(g_out=None), dict(g_in=None)], "idb_blk_conv_dgrad: g_out or g_in null")
    MC.refused(lib, dgr, CONV_OK, [dict(cin=4, affine=None, slope=None)], "idb_blk_conv_dgrad: cin % 64 == 0 (the stem's image gradient is not built)")
    MC.refused(lib, wgr, CONV_OK, [dict(g_out=OFF), dict(g_out=None), dict(d_weight=None)], "idb_blk_conv_wgrad: g_out or d_weight null")
    need = lib.idb_blk_conv_workspace_bytes(2, 3, 5, 64, 64, 3, 1, None, None)
    assert need == M.conv_plan((2, 3, 5, 64, 64, 3, 1))["bytes"]
    MC.refused(lib, wgr, CONV_OK, [dict(ws=OFF), dict(ws=None), dict(ws_bytes=need - 1), dict(ws_bytes=0)], "idb_blk_conv_wgrad: workspace too small or unaligned")


BN_OK = dict(x=P16, rows=257, ch=64, training=1, eps=1e-5, momentum=0.1, gamma=P16, beta=P16, rmean=P16, rvar=P16, stat=P16, affine=P16,
             flags=P16, ws=P16, ws_bytes=1 << 30, stream=None)


def test_bn_forward_argument_checks(lib):
    f = lambda a: lib.idb_blk_bn_forward(*a.values())      # noqa: E731
    MC.refused(lib, f, BN_OK, [dict(training=2), dict(training=-1)], "idb_blk_bn_forward: training must be 0 or 1")
    MC.refused(lib, f, BN_OK, [dict(eps=-1e-9), dict(eps=1.5), dict(momentum=-0.1), dict(momentum=1.0 + 1e-9), dict(eps=float("nan")),
                             dict(momentum=float("nan"))], "idb_blk_bn_forward: eps in [0, 1], momentum in [0, 1]")
    MC.refused(lib, f, BN_OK, [dict(rows=1)], "idb_blk_bn_forward: one value per channel")
    MC.refused(lib, f, BN_OK, [dict(rows=0), dict(ch=96), dict(ch=32), dict(ch=2112), dict(rows=1024 * 128 * 128 + 1)], "idb_blk_bn_forward: rows in 1..")
    MC.refused(lib, f, BN_OK, [dict(affine=OFF), dict(stat=OFF)], "idb_blk_bn_forward: affine 16-byte, stat 8-byte aligned")
    MC.refused(lib, f, BN_OK, [{k: None} for k in ("x", "gamma", "beta", "rmean", "rvar", "stat", "affine", "flags")], "idb_blk_bn_forward: null pointer")
    need = M.bn_plan(257, 64)["bytes"]
    MC.refused(lib, f, BN_OK, [dict(ws=OFF), dict(ws=None), dict(ws_bytes=need - 1)], "idb_blk_bn_forward: workspace too small or unaligned")


BNB_OK = dict(c=P16, g=P16, rows=257, ch=64, stat=P16, affine=P16, gamma=P16, slope=P16, add=P16, d_gamma=P16, d_beta=P16, d_slope=P16, g_c=P16,
              ws=P16, ws_bytes=1 << 30, stream=None)


def test_bn_backward_argument_checks(lib):
    f = lambda a: lib.idb_blk_bn_backward(*a.values())      # noqa: E731
    MC.refused(lib, f, BNB_OK, [dict(rows=1), dict(rows=0), dict(ch=96)], "idb_blk_bn_backward: rows in 2..")
    MC.refused(lib, f, BNB_OK, [dict(slope=None), dict(d_slope=None)], "idb_blk_bn_backward: slope and d_slope go together")
    MC.refused(lib, f, BNB_OK, [dict(c=OFF), dict(g=OFF), dict(add=OFF), dict(g_c=OFF), dict(stat=OFF)], "idb_blk_bn_backward: c, g, add and g_c 16-byte")
    MC.refused(lib, f, BNB_OK, [{k: None} for k in ("c", "g", "stat", "affine", "gamma", "d_gamma", "d_beta", "g_c")], "idb_blk_bn_backward: null pointer")
    need = M.bn_plan(257, 64)["bytes"]
    MC.refused(lib, f, BNB_OK, [dict(ws=OFF), dict(ws=None), dict(ws_bytes=need - 1)], "idb_blk_bn_backward: workspace too small or unaligned")


AFF_OK = dict(c=P16, affine=P16, slope=P16, identity=P16, id_affine=P16, rows=3, ch=64, out=P16, stream=None)


def test_affine_pack_and_sgd_argument_checks(lib):
    f = lambda a: lib.idb_blk_affine(*a.values())      # noqa: E731
    MC.refused(lib, f, AFF_OK, [{k: OFF} for k in ("c", "affine", "slope", "identity", "id_affine", "out")], "idb_blk_affine: every pointer 16-byte aligned")
    MC.refused(lib, f, AFF_OK, [dict(identity=None)], "idb_blk_affine: an identity affine pair without the identity")
    MC.refused(lib, f, AFF_OK, [dict(c=None), dict(affine=None), dict(out=None)], "idb_blk_affine: null pointer")
    MC.refused(lib, f, AFF_OK, [dict(rows=0), dict(ch=4), dict(ch=100)], "idb_blk_affine: rows in 1..")
    pk = dict(images=P16, b=2, h=15, w=17, out=P16, stream=None)
    f = lambda a: lib.idb_blk_pack_images(*a.values())      # noqa: E731
    MC.refused(lib, f, pk, [dict(h=129), dict(w=129), dict(h=0), dict(b=0), dict(b=1025)], "idb_blk_pack_images: b in 1..1024")
    MC.refused(lib, f, pk, [dict(out=OFF), dict(out=None), dict(images=None)], "idb_blk_pack_images: null pointer, or out not 16-byte aligned")
    sg = dict(count=3, w=P16, g=P16, buf=P16, n=P16, lr=0.1, momentum=0.9, wd=5e-4, max_norm=5.0, first=1, total=P16, ws=P16, ws_bytes=1 << 30,
              stream=None)
    f = lambda a: lib.idb_sgd_clip_step_table(*a.values())      # noqa: E731
    MC.refused(lib, f, sg, [dict(count=0), dict(count=1025), dict(count=-1)], "idb_sgd_clip_step_table: 1..1024 tensors")
    MC.refused(lib, f, sg, [{k: OFF} for k in ("w", "g", "buf", "n", "total")], "idb_sgd_clip_step_table: total_norm and the tables 8-byte aligned")
    MC.refused(lib, f, sg, [dict(ws_bytes=8 * 3 * 1024 - 1), dict(ws=OFF)], "idb_sgd_clip_step_table: workspace too small or unaligned")
    assert lib.idb_sgd_clip_table_workspace_bytes(0) == 0 and lib.idb_sgd_clip_table_workspace_bytes(1025) == 0
    assert lib.idb_sgd_clip_table_workspace_bytes(1) == 8 * 1024 and lib.idb_sgd_clip_table_workspace_bytes(1024) == 8 * 1024 * 1024
