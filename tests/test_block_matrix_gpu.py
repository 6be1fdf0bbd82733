"""Every case of the trunk kernels' per-entry test matrix (tests/block_matrix.py) on the device, each C entry of csrc/idb_block.hip called
directly with exact fp32 inputs, element by element against the float64 references and the bounds derived in frblock_oracle.py with
every inherited error term 0 (the module docstring of block_matrix.py states each criterion).

Every output buffer, the wgrad and BatchNorm workspaces (passed at exactly their stated size), the running statistics and the flags
lie between 64 guard words of a NaN bit pattern; outputs and workspaces are pre-filled with that pattern.  After the launch the guards
are unchanged, and an element the kernel did not write keeps its NaN and fails its criterion.  A repeat of every call is bit-identical.
The load-path activation (conv_forward / conv_wgrad with affine and slope) is bit-identical to the same entry on
idb_blk_affine(x, affine, slope) with neither, and dgrad does not depend on the affine pair its descriptor carries.

test_summary prints the worst err / bound per entry and output.  Measured on an MI355X, 127 tests, all passing, 16 s in all, the slowest
(the backward at 307 193 rows) 2 s (never used as thresholds):

  conv forward 0.2047 (the stem case)   dgrad 0.0188 (1x1 stride 1)   wgrad 0.3062 ((2, 1, 5, 64, 64, 3, 2), affine only)
               the load-path activation and every repeat bit-identical on every case
  bn forward   mean 0.0001  invstd 0.0199  sc 0.9799  sh 0.9797  running mean 0.9828  running var 0.9647
  bn backward  g_c 0.9997  d gamma 0.9679  d beta 0.9737  d slope 0.8346        affine 0.9995
               (sc, sh, the running statistics, the backward's outputs and the affine's are double-precision values rounded once to
               fp32: a correctly rounded value attains u |value|, the bound's leading term)
  table SGD    weight 0.9547  momentum 0.9562 (1024 tensors, step 1)
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import block_matrix as M  # noqa: E402
import frtail_oracle as TO  # noqa: E402
import matrix_common as MC  # noqa: E402
from faceposegenerator_amd import _lib as L  # noqa: E402

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
W = MC.Worst("block matrix")


# ---- convolutions --------------------------------------------------------------------------------------------------------------------
def _desc(case, x_ptr, aff, sl, w):
    d = L.BlkConvDesc()
    d.b, d.h, d.w, d.cin, d.cout, d.ksize, d.stride = case
    d.x, d.affine, d.slope, d.weight = x_ptr, MC.ptr(aff), MC.ptr(sl), MC.ptr(w)
    return d


class _Conv:
    def __init__(self, case, mode):
        self.case, self.mode, self.g = case, mode, M.conv_geo(case)
        x, w, go, aff, sl = M.conv_operands(case, mode)
        self.x, self.w, self.go, self.aff, self.sl = (MC.dev(v, F32) for v in (x, w, go, aff, sl))
        self.desc = _desc(case, self.x.data_ptr(), self.aff, self.sl, self.w)
        self.what = f"{case} {mode}"

    def preactivated(self, lib):
        """The descriptor of the same conv on idb_blk_affine(x, affine, slope) with no affine pair."""
        g = self.g
        self.pre = MC.Guarded(self.x.numel())
        L.check(lib.idb_blk_affine(self.x.data_ptr(), self.aff.data_ptr(), MC.ptr(self.sl), None, None, g["B"] * g["H"] * g["W"], g["cin"], self.pre.ptr,
                                   MC.stream()), "idb_blk_affine " + self.what)
        return _desc(self.case, self.pre.ptr, None, None, self.w)


CONV_PARAMS = [(c, m) for c in M.CONV_CASES for m in M.conv_modes(c)]


@pytest.mark.parametrize("case,mode", CONV_PARAMS, ids=lambda v: str(v))
def test_conv_forward(lib, case, mode):
    cv = _Conv(case, mode)
    what, n = "idb_blk_conv_forward " + cv.what, cv.g["Mo"] * cv.g["cout"]
    out, again = MC.Guarded(n), MC.Guarded(n)
    for o in (out, again):
        L.check(lib.idb_blk_conv_forward(C.byref(cv.desc), o.ptr, MC.stream()), what)
    pre = None
    if cv.aff is not None:
        pre = MC.Guarded(n)
        L.check(lib.idb_blk_conv_forward(C.byref(cv.preactivated(lib)), pre.ptr, MC.stream()), what + " (pre-activated)")
    torch.cuda.synchronize()
    ref, bound = M.conv_reference(case, mode, "fwd")
    got = out.f32(what)
    W.judge("conv forward", what, got.reshape(ref.shape), ref, bound)
    MC.same_bits(what + ": a repeat", got, again.f32(what))
    if pre is not None:
        MC.same_bits(what + ": the load-path activation against idb_blk_affine's", got, pre.f32(what))


@pytest.mark.parametrize("case", M.CONV_CASES, ids=str)
def test_conv_dgrad(lib, case):
    g = M.conv_geo(case)
    n = g["B"] * g["H"] * g["W"] * g["cin"]
    outs = []
    for mode in M.conv_modes(case) + M.conv_modes(case)[:1]:          # every mode, and a repeat of the first
        cv = _Conv(case, mode)
        what = "idb_blk_conv_dgrad " + cv.what
        gi = MC.Guarded(n)
        rc = lib.idb_blk_conv_dgrad(C.byref(cv.desc), cv.go.data_ptr(), gi.ptr, MC.stream())
        torch.cuda.synchronize()
        if g["cin"] == 4:
            assert rc != 0 and b"cin % 64 == 0" in lib.idb_last_error() and gi.untouched(what), what
            continue
        L.check(rc, what)
        outs.append(gi.f32(what))
    if g["cin"] == 4:
        return
    ref, bound = M.conv_reference(case, "plain", "dgrad")
    W.judge("conv dgrad", what, outs[0].reshape(ref.shape), ref, bound)
    zero = np.broadcast_to(M.no_tap_mask(case)[None, :, :, None], ref.shape).reshape(-1)
    assert (outs[0].view(np.uint32)[zero] == 0).all(), f"{what}: a pixel no tap reaches is not an exact +0"
    for o in outs[1:]:
        MC.same_bits(what + ": a repeat, or another affine pair in the descriptor", outs[0], o)


@pytest.mark.parametrize("case,mode", CONV_PARAMS, ids=lambda v: str(v))
def test_conv_wgrad(lib, case, mode):
    cv = _Conv(case, mode)
    g, p = cv.g, M.conv_plan(case)
    what, n = "idb_blk_conv_wgrad " + cv.what, cv.g["cout"] * cv.g["K"]
    need = lib.idb_blk_conv_workspace_bytes(*case, None, None)
    assert need == p["bytes"] and need % 4 == 0
    descs = [cv.desc, cv.desc] + ([cv.preactivated(lib)] if cv.aff is not None else [])
    outs, works = [MC.Guarded(n) for _ in descs], [MC.Guarded(need // 4) for _ in descs]
    for d, o, ws in zip(descs, outs, works):
        L.check(lib.idb_blk_conv_wgrad(C.byref(d), cv.go.data_ptr(), o.ptr, ws.ptr, need, MC.stream()), what)
    torch.cuda.synchronize()
    ref, bound = M.conv_reference(case, mode, "wgrad")
    got = outs[0].f32(what)
    W.judge("conv wgrad", what, got.reshape(ref.shape), ref, bound)
    assert np.isfinite(works[0].f32(what + " workspace")[:p["slices"] * n]).all(), f"{what}: an element of a slice's partial was not written"
    MC.same_bits(what + ": a repeat", got, outs[1].f32(what))
    if len(descs) == 3:
        MC.same_bits(what + ": the load-path activation against idb_blk_affine's", got, outs[2].f32(what))
        works[2].raw(what + " workspace")


# ---- BatchNorm forward ---------------------------------------------------------------------------------------------------------------
def _bn_forward(lib, x, prm, what, training=1, eps=M.EPS, momentum=M.MOMENTUM):
    rows, ch = x.shape
    need = lib.idb_blk_bn_workspace_bytes(rows, ch, None)
    assert need == M.bn_plan(rows, ch)["bytes"]
    dx = x if torch.is_tensor(x) else MC.dev(x, F32)
    gam, beta = MC.dev(prm["bn.weight"], F32), MC.dev(prm["bn.bias"], F32)
    rm, rv = MC.Guarded(ch, init=prm["bn.running_mean"].astype(F32)), MC.Guarded(ch, init=prm["bn.running_var"].astype(F32))
    stat, aff, flags, ws = MC.Guarded(4 * ch), MC.Guarded(2 * ch), MC.Guarded(2, init=np.zeros(2, np.int32)), MC.Guarded(need // 4)
    L.check(lib.idb_blk_bn_forward(dx.data_ptr(), rows, ch, training, eps, momentum, gam.data_ptr(), beta.data_ptr(), rm.ptr, rv.ptr, stat.ptr, aff.ptr,
                                   flags.ptr, ws.ptr, need, MC.stream()), what)
    torch.cuda.synchronize()
    ws.raw(what + " workspace")
    st, af = stat.f64(what).reshape(2, ch), aff.f32(what).reshape(2, ch)
    return dict(mean=st[0], invstd=st[1], sc=af[0], sh=af[1], running_mean=rm.f32(what), running_var=rv.f32(what)), tuple(int(v) for v in flags.raw(what))


def _judge_bn(what, got, ref, bound, keep=None):
    for k in ref:
        sel = slice(None) if keep is None else keep
        W.judge(f"bn forward {k}", f"{what} {k}", got[k][sel].reshape(ref[k][sel].shape), ref[k][sel], bound[k][sel])


@pytest.mark.parametrize("rows,ch", M.bn_cases())
def test_bn_forward(lib, rows, ch):
    what = f"idb_blk_bn_forward {rows} x {ch}"
    x, prm = M.bn_inputs(rows, ch)
    dx = MC.dev(x, F32)
    got, flags = _bn_forward(lib, dx, prm, what)
    again, _ = _bn_forward(lib, dx, prm, what)
    ref, bound = M.bn_forward_reference(x, prm)
    _judge_bn(what, got, ref, bound)
    assert flags == (0, 0), (what, flags)
    for k in got:
        MC.same_bits(f"{what} {k}: a repeat", got[k], again[k])


def test_bn_forward_planted_channels_eval_and_momentum(lib):
    rows, ch = 257, 64
    x, prm = M.bn_inputs(rows, ch, "const")
    what = "idb_blk_bn_forward, a constant channel with eps == 0"
    got, flags = _bn_forward(lib, x, prm, what, eps=0.0)
    ref, bound = M.bn_forward_reference(x, prm, eps=0.0)
    assert flags == (0, 1), (what, flags)
    _judge_bn(what, got, ref, bound, np.arange(ch) != M.CONST_CH)
    x, prm = M.bn_inputs(rows, ch, "inf")
    what = "idb_blk_bn_forward, one +inf"
    got, flags = _bn_forward(lib, x, prm, what)
    ref, bound = M.bn_forward_reference(x, prm)
    assert flags == (1, 0), (what, flags)
    _judge_bn(what, got, ref, bound, np.arange(ch) != M.INF_CH)
    x, prm = M.bn_inputs(2, 192)
    what = "idb_blk_bn_forward, eval mode with one row"
    got, flags = _bn_forward(lib, x[:1], prm, what, training=0)
    ref, bound = M.bn_forward_reference(x[:1], prm, training=False)
    _judge_bn(what, got, ref, bound)
    assert flags == (0, 0)
    MC.same_bits(what + ": the running mean is left as it was", got["running_mean"], prm["bn.running_mean"].astype(F32))
    MC.same_bits(what + ": the running variance is left as it was", got["running_var"], prm["bn.running_var"].astype(F32))
    for mom in (0.0, 1.0):
        what = f"idb_blk_bn_forward, momentum {mom}"
        got, flags = _bn_forward(lib, x, prm, what, momentum=mom)
        ref, bound = M.bn_forward_reference(x, prm, momentum=mom)
        _judge_bn(what, got, ref, bound)
        assert flags == (0, 0)
        if mom == 0.0:
            MC.same_bits(what + ": the running mean is left as it was", got["running_mean"], prm["bn.running_mean"].astype(F32))


# ---- BatchNorm backward and the affine kernel ------------------------------------------------------------------------------------------
class _Bnb:
    def __init__(self, rows, ch):
        i = M.bnb_inputs(rows, ch)
        self.rows, self.ch = rows, ch
        self.c, self.g, self.add, self.gamma, self.slope = (MC.dev(i[k], F32) for k in ("c", "g", "add", "gamma", "slope"))
        self.aff, self.id_aff = MC.dev(i["affine"], F32), MC.dev(i["id_affine"], F32)
        self.stat = torch.from_numpy(np.array(i["stat"], F64)).to(MC.DEV)

    def backward(self, lib, with_slope, with_add, what):
        rows, ch = self.rows, self.ch
        need = lib.idb_blk_bn_workspace_bytes(rows, ch, None)
        dgam, dbeta, dsl, gc, ws = MC.Guarded(ch), MC.Guarded(ch), (MC.Guarded(ch) if with_slope else None), MC.Guarded(rows * ch), MC.Guarded(need // 4)
        L.check(lib.idb_blk_bn_backward(self.c.data_ptr(), self.g.data_ptr(), rows, ch, self.stat.data_ptr(), self.aff.data_ptr(), self.gamma.data_ptr(),
                                        MC.ptr(self.slope) if with_slope else None, MC.ptr(self.add) if with_add else None, dgam.ptr, dbeta.ptr,
                                        dsl.ptr if with_slope else None, gc.ptr, ws.ptr, need, MC.stream()), what)
        torch.cuda.synchronize()
        ws.raw(what + " workspace")
        out = dict(gc=gc.f32(what), gamma=dgam.f32(what), beta=dbeta.f32(what))
        if with_slope:
            out["slope"] = dsl.f32(what)
        return out

    def affine(self, lib, with_slope, identity, what):
        out = MC.Guarded(self.rows * self.ch)
        L.check(lib.idb_blk_affine(self.c.data_ptr(), self.aff.data_ptr(), MC.ptr(self.slope) if with_slope else None,
                                   None if identity == "none" else self.add.data_ptr(), self.id_aff.data_ptr() if identity == "affine" else None,
                                   self.rows, self.ch, out.ptr, MC.stream()), what)
        torch.cuda.synchronize()
        return out.f32(what)


@pytest.mark.parametrize("rows,ch", M.bn_cases())
def test_bn_backward(lib, rows, ch):
    dev = _Bnb(rows, ch)
    for form in (M.BNB_FORMS if rows not in M.BN_CAP_ROWS else M.BNB_FORMS[3:]):
        what = f"idb_blk_bn_backward {rows} x {ch} slope {form[0]} add {form[1]}"
        got = dev.backward(lib, *form, what)
        ref, bound = M.bn_backward_reference(rows, ch, *form)
        for k in ref:
            W.judge(f"bn backward {k}", f"{what} {k}", got[k].reshape(ref[k].shape), ref[k], bound[k])
        if form == M.BNB_FORMS[3]:
            again = dev.backward(lib, *form, what)
            for k in got:
                MC.same_bits(f"{what} {k}: a repeat", got[k], again[k])


@pytest.mark.parametrize("rows,ch", M.bn_cases())
def test_affine(lib, rows, ch):
    dev = _Bnb(rows, ch)
    for form in (M.AFFINE_FORMS if rows not in M.BN_CAP_ROWS else M.AFFINE_FORMS[5:]):
        what = f"idb_blk_affine {rows} x {ch} slope {form[0]} identity {form[1]}"
        got = dev.affine(lib, *form, what)
        ref, bound = M.affine_reference(rows, ch, *form)
        W.judge("affine", what, got.reshape(ref.shape), ref, bound)
        if form == M.AFFINE_FORMS[5]:
            MC.same_bits(what + ": a repeat", got, dev.affine(lib, *form, what))


# ---- pack and the table SGD ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", M.PACK_SHAPES, ids=str)
def test_pack_images(lib, shape):
    what = f"idb_blk_pack_images {shape}"
    b, h, w = shape
    img = MC.dev(M.pack_input(shape), F32)
    out, again = MC.Guarded(b * h * w * 4), MC.Guarded(b * h * w * 4)
    for o in (out, again):
        L.check(lib.idb_blk_pack_images(img.data_ptr(), b, h, w, o.ptr, MC.stream()), what)
    torch.cuda.synchronize()
    MC.same_bits(what, out.f32(what), M.pack_reference(shape))
    MC.same_bits(what + ": a repeat", out.f32(what), again.f32(what))


@pytest.mark.parametrize("count", M.SGD_COUNTS)
def test_sgd_table(lib, count):
    sizes = M.sgd_sizes(count)
    tensors = lambda salt: [((TO._h(np.arange(n) + 5 * i + salt, 201) - 100) / 100.0).astype(F32) for i, n in enumerate(sizes)]      # noqa: E731
    table = lambda ts: torch.tensor([t.ptr for t in ts], dtype=torch.int64).to(MC.DEV)                                              # noqa: E731
    w0 = tensors(2)
    ws, bufs = [MC.Guarded(n, init=w) for n, w in zip(sizes, w0)], [MC.Guarded(n) for n in sizes]
    ref_w, ref_b, total = [w.astype(F64) for w in w0], None, sum(sizes)
    eb, ew = [np.zeros(n) for n in sizes], [np.zeros(n) for n in sizes]
    lr, mom, wd = 0.1, 0.9, 5e-4
    need = lib.idb_sgd_clip_table_workspace_bytes(count)
    work, norm = MC.Guarded(need // 4), MC.Guarded(2)
    numel = torch.tensor(sizes, dtype=torch.int64).to(MC.DEV)
    tw, tb = table(ws), table(bufs)
    for step, scale in enumerate((0.5, 0.01)):
        what = f"idb_sgd_clip_step_table, {count} tensors, step {step + 1}"
        g0 = [g * F32(scale) for g in tensors(11 + step)]
        gs = [MC.dev(g, F32) for g in g0]
        tg = torch.tensor([g.data_ptr() for g in gs], dtype=torch.int64).to(MC.DEV)
        ref_w, ref_b, ref_norm = TO.sgd_step(ref_w, [g.astype(F64) for g in g0], ref_b, lr, mom, wd, 5.0)
        L.check(lib.idb_sgd_clip_step_table(count, tw.data_ptr(), tg.data_ptr(), tb.data_ptr(), numel.data_ptr(), lr, mom, wd, 5.0, int(step == 0),
                                            norm.ptr, work.ptr, need, MC.stream()), what)
        torch.cuda.synchronize()
        work.raw(what + " workspace")
        assert abs(float(norm.f64(what)[0]) - ref_norm) <= (total + 8) * TO.U64 * ref_norm, what
        coef = min(1.0, 5.0 / (ref_norm + 1e-6))
        gw = np.concatenate([w.f32(what) for w in ws])
        gb = np.concatenate([b.f32(what) for b in bufs])
        for i in range(count):
            eb[i], ew[i] = TO.sgd_bound(ref_w[i], ref_b[i], eb[i], ew[i], lr, mom, wd, coef * np.abs(g0[i].astype(F64)), total)
        W.judge("table sgd weight", what + " weight", gw, np.concatenate(ref_w), np.concatenate(ew))
        W.judge("table sgd momentum", what + " momentum", gb, np.concatenate(ref_b), np.concatenate(eb))


# ---- refusals leave guards and outputs as they were ------------------------------------------------------------------------------------
def test_refusals_leave_outputs_untouched(lib):
    case = M.CONV_CASES[4]
    cv = _Conv(case, "prelu")
    g, n = cv.g, cv.g["Mo"] * cv.g["cout"]
    out, dw = MC.Guarded(n), MC.Guarded(g["cout"] * g["K"])
    need = lib.idb_blk_conv_workspace_bytes(*case, None, None)
    ws = MC.Guarded(need // 4)
    before = lib.idb_launch_count()
    d = _desc(case, cv.x.data_ptr(), None, cv.sl, cv.w)                                       # a slope without the affine pair
    assert lib.idb_blk_conv_forward(C.byref(d), out.ptr, MC.stream()) != 0 and b"a PReLU slope without" in lib.idb_last_error()
    d = _desc(case, cv.x.data_ptr() + 4, cv.aff, cv.sl, cv.w)                                   # x misaligned
    assert lib.idb_blk_conv_forward(C.byref(d), out.ptr, MC.stream()) != 0 and b"16-byte aligned" in lib.idb_last_error()
    assert lib.idb_blk_conv_wgrad(C.byref(cv.desc), cv.go.data_ptr(), dw.ptr, ws.ptr, need - 1, MC.stream()) != 0      # one byte short
    assert b"workspace too small" in lib.idb_last_error()
    dev = _Bnb(2, 64)
    gc, dgam, dbeta, dsl, bws = MC.Guarded(2 * 64), MC.Guarded(64), MC.Guarded(64), MC.Guarded(64), MC.Guarded(lib.idb_blk_bn_workspace_bytes(2, 64, None) // 4)
    args = lambda rows, sl, dsl_: (dev.c.data_ptr(), dev.g.data_ptr(), rows, 64, dev.stat.data_ptr(), dev.aff.data_ptr(), dev.gamma.data_ptr(), sl, None,      # noqa: E731
                                   dgam.ptr, dbeta.ptr, dsl_, gc.ptr, bws.ptr, 4 * bws.n, MC.stream())
    assert lib.idb_blk_bn_backward(*args(1, dev.slope.data_ptr(), dsl.ptr)) != 0 and b"rows in 2.." in lib.idb_last_error()
    assert lib.idb_blk_bn_backward(*args(2, dev.slope.data_ptr(), None)) != 0 and b"go together" in lib.idb_last_error()
    assert lib.idb_blk_bn_backward(*args(2, None, dsl.ptr)) != 0 and b"go together" in lib.idb_last_error()
    aout = MC.Guarded(2 * 64)
    assert lib.idb_blk_affine(dev.c.data_ptr(), dev.aff.data_ptr(), None, None, dev.id_aff.data_ptr(), 2, 64, aout.ptr, MC.stream()) != 0
    assert b"without the identity" in lib.idb_last_error()
    img, pout = MC.dev(np.zeros((1, 3, 129, 1)), F32), MC.Guarded(129 * 4)
    assert lib.idb_blk_pack_images(img.data_ptr(), 1, 129, 1, pout.ptr, MC.stream()) != 0 and b"h and w in 1..128" in lib.idb_last_error()
    torch.cuda.synchronize()
    assert lib.idb_launch_count() == before
    for name, b in (("out", out), ("d_weight", dw), ("wgrad workspace", ws), ("g_c", gc), ("d_gamma", dgam), ("d_beta", dbeta), ("d_slope", dsl),
                    ("bn workspace", bws), ("affine out", aout), ("pack out", pout)):
        assert b.untouched(name), f"{name}: a refused call wrote to it"


def test_summary():
    W.show()
