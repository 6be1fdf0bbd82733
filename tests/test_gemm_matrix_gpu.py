"""Every accepted (case, tile id, feature combination) of idb_gemm against a float64 reference, element by element (tests/gemm_matrix.py).

Each case's inputs are rounded to the operand dtype once; the reference is computed once per case in float64 on the device (matmul for
linear cases, im2col + matmul for convs, the epilogue in float64) and reused for every tile and feature.  Only combinations that
gemm_matrix.classify() accepts are launched; every output buffer is filled with NaN first, so an element a kernel does not write fails.

Side outputs have their own checks: gn_partials and row statistics against float64 sums of the ROUNDED output (fp32 summation bound),
out2 bit-equal to fma(out, scale, shift) of the rounded output, the fused GroupNorm against a float64 GroupNorm(+SiLU) then the conv
(plus one operand rounding per normalised element: the kernel multiplies the rounded operand bits idb_groupnorm would write).

Bound constants gemm_matrix.C_R = C_A = 1, measured on MI355X (test_family_summary prints one line per family and feature):
  - operand-dtype outputs: worst err / bound 0.995 (bf16) and 0.990 (f16) in every family — the output rounding itself (half an ulp
    just above a power of two), so C_R cannot go lower;
  - fp32 outputs (the accumulation alone): worst 0.106 (bf16 operands) / 0.133 (f16), so C_A = 1 leaves a factor 7 of margin;
  - fused GroupNorm: worst 0.57 / 0.50 with its operand-rounding term;
  - large-grid plans (sampled rows): worst 0.995 / 0.990.
The whole file runs in about 12 s on one MI355X (about 34,000 launched combinations over both dtypes)."""
import ctypes as C
import math
import os
import sys
from collections import defaultdict

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_matrix as GM  # noqa: E402
from faceposegenerator_amd import _lib as L  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = {"bf16": (L.IDB_BF16, torch.bfloat16), "f16": (L.IDB_F16, torch.float16)}

_SUMMARY = defaultdict(lambda: [0, 0, 0.0])      # (dtype, family) -> [runs, refusals, worst ratio]
_FEAT_WORST = defaultdict(float)                  # (dtype, feature) -> worst ratio


def _gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def _im2col(case, xs):
    """xs: float64 NHWC source tensors -> A [M][K] in the kernel's K order ([segment][tap][channel])."""
    cols = []
    for (ch, taps, ih, iw, up), x in zip(case.srcs, xs):
        t = x.permute(0, 3, 1, 2)
        if up:
            t = t.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)
        if taps == 9:
            if case.pad_mode == 1:
                u = F.unfold(F.pad(t, (0, 2, 0, 2)), 3, padding=0, stride=case.stride)
            else:
                u = F.unfold(t, 3, padding=1, stride=case.stride)
            u = u.reshape(case.batch, ch, 9, case.out_h, case.out_w)
            cols.append(u.permute(0, 3, 4, 2, 1).reshape(case.M, 9 * ch))
        else:
            if t.shape[2] != case.out_h or t.shape[3] != case.out_w:      # stride-2 1x1 source on the input grid
                t = t[:, :, ::2, ::2]
            cols.append(t.permute(0, 2, 3, 1).reshape(case.M, ch))
    return torch.cat(cols, dim=1)


class CaseData:
    """Device inputs of one case in one dtype, and the float64 references derived from them (computed lazily, once)."""

    def __init__(self, lib, case, dt, tdt, seed):
        self.lib, self.case, self.dt, self.tdt = lib, case, dt, tdt
        g = torch.Generator(device=DEV).manual_seed(seed)
        rnd = lambda *s: torch.randn(*s, generator=g, device=DEV)
        M, K, n = case.M, case.K, case.n
        self.srcs = [(rnd(case.batch, ih, iw, ch) + 0.25).to(tdt) for ch, taps, ih, iw, up in case.srcs]
        self.wg = (rnd(2, n, K) * K ** -0.5).to(tdt)                      # two matrices back to back: w_groups
        self.w = self.wg[0]
        self.w_tiled = torch.empty(lib.idb_tiled_weight_bytes(n, K) // 2, dtype=tdt, device=DEV)
        L.check(lib.idb_tile_weight(self.w.data_ptr(), self.w_tiled.data_ptr(), n, K, dt, None), "idb_tile_weight")
        self.bias = rnd(n)
        self.sbias = rnd(case.batch, n)
        self.res = rnd(M, n).to(tdt)
        self.slope = 0.05 + 0.4 * torch.rand(n, generator=g, device=DEV)
        self.out2_scale, self.out2_shift = 0.5 + torch.rand(n, generator=g, device=DEV), rnd(n)
        self.ln_v = rnd(n)
        self.gn_gamma, self.gn_beta = 1.0 + 0.3 * rnd(512), 0.2 * rnd(512)
        self.counters = torch.zeros(GM.COUNTERS, dtype=torch.int32, device=DEV)
        self.ws = torch.empty(0, dtype=torch.uint8, device=DEV)
        self._acc = {}
        self.ptrs = {f"src{i}": s.data_ptr() for i, s in enumerate(self.srcs)}
        self.ptrs.update(w=self.w.data_ptr(), w_tiled=self.w_tiled.data_ptr(), bias=self.bias.data_ptr(), sbias=self.sbias.data_ptr(),
                         res=self.res.data_ptr(), slope=self.slope.data_ptr(), out2_scale=self.out2_scale.data_ptr(),
                         out2_shift=self.out2_shift.data_ptr(), ln_v=self.ln_v.data_ptr(), gn_gamma=self.gn_gamma.data_ptr(),
                         gn_beta=self.gn_beta.data_ptr(), counters=self.counters.data_ptr())
        if len(case.srcs) == 1 and case.srcs[0][1] == 1:
            x = self.srcs[0].double().reshape(M, K)
            h = K // 2
            st = torch.stack([torch.stack([x[:, :h].sum(1), (x[:, :h] ** 2).sum(1)], 1),
                              torch.stack([x[:, h:].sum(1), (x[:, h:] ** 2).sum(1)], 1)], 1)
            self.ln_stats = st.float().contiguous()                        # [M][2 tiles][2]
            self.ln_u = self.w.double().sum(1).float()
            self.ptrs.update(ln_stats=self.ln_stats.data_ptr(), ln_u=self.ln_u.data_ptr())

    # ---- references ---------------------------------------------------------------------------------------------------------
    def gn_inputs(self, nsrc, silu):
        """float64 GroupNorm(32)(+SiLU) of the first nsrc sources' channel concatenation, and the partials handed to the kernel."""
        key = ("gnx", nsrc, silu)
        if key not in self._acc:
            case = self.case
            xs = [s.double() for s in self.srcs[:nsrc]]
            x = torch.cat(xs, dim=3)                                       # [B][H][W][cn]
            B, cn, G, hw = case.batch, x.shape[3], GM.GN_GROUPS, case.hw
            ch = GM.gn_chunks(case)
            xg = x.reshape(B, ch, hw // ch, G, cn // G)
            part = torch.stack([xg.sum(dim=(2, 4)), (xg * xg).sum(dim=(2, 4))], dim=-1).float().contiguous()   # [B][chunks][G][2]
            p = part.double().sum(1)                                       # [B][G][2] from the fp32 partials the kernel reads
            cnt = hw * (cn // G)
            mean = p[..., 0] / cnt
            var = (p[..., 1] / cnt - mean * mean).clamp_min(0)
            rstd = 1.0 / torch.sqrt(var + 1e-5)
            k = (rstd[:, :, None] * torch.ones(cn // G, dtype=torch.float64, device=DEV)).reshape(B, cn)
            mm = (mean[:, :, None] * torch.ones(cn // G, dtype=torch.float64, device=DEV)).reshape(B, cn)
            y = (x - mm[:, None, None, :]) * k[:, None, None, :] * self.gn_gamma[:cn].double() + self.gn_beta[:cn].double()
            if silu:
                y = y * torch.sigmoid(y)
            outs, c0 = [], 0
            for s in xs:
                outs.append(y[..., c0:c0 + s.shape[3]])
                c0 += s.shape[3]
            self._acc[key] = (outs, part)
        return self._acc[key]

    def acc(self, which="raw", group=0):
        """(A W^T, |A| |W|^T, A) in float64 for A = the raw sources ('raw') or with the GroupNorm applied ((nsrc, silu))."""
        key = (which, group)
        if key not in self._acc:
            xs = [s.double() for s in self.srcs]
            if which != "raw":
                nsrc, silu = which
                xs[:nsrc] = self.gn_inputs(nsrc, silu)[0]
            A = _im2col(self.case, xs)
            W = self.wg[group].double()
            self._acc[key] = (A @ W.t(), A.abs() @ W.abs().t(), A)
        return self._acc[key]

    # ---- one combination ----------------------------------------------------------------------------------------------------
    def run(self, tile, feat, verdict):
        case, f, lib = self.case, GM.FEATURES[feat], self.lib
        M, n = case.M, case.n
        bm, bn = GM.tile_dims(verdict.tile)
        ncols = n // 2 if "geglu" in f else n
        odt = torch.float32 if "f32" in f else self.tdt
        bufs = {"out": torch.full((M, ncols), float("nan"), dtype=odt, device=DEV)}
        ptrs = dict(self.ptrs, out=bufs["out"].data_ptr(), out32=bufs["out"].data_ptr())
        if "out2" in f:
            bufs["out2"] = torch.full((M, n), float("nan"), dtype=self.tdt, device=DEV)
            ptrs["out2"] = bufs["out2"].data_ptr()
        if "gnp" in f:
            bufs["gnp"] = torch.full((case.batch, case.hw // 64, GM.GN_GROUPS, 2), float("nan"), device=DEV)
            ptrs["gnp"] = bufs["gnp"].data_ptr()
        nt = (n + bn - 1) // bn
        assert verdict.row_tiles in (0, nt), (verdict.row_tiles, nt)
        if "rows" in f:
            bufs["rows"] = torch.full((M, nt, 2), float("nan"), device=DEV)
            ptrs["rows"] = bufs["rows"].data_ptr()
        gn_key = None
        if "gn" in f:
            gn_key = (2 if "gn2" in f else 1, "nosilu" not in f)
            ptrs["gn_part"] = self.gn_inputs(*gn_key)[1].data_ptr()
        d = GM.make_desc(case, self.dt, tile, feat, ptrs, bm)
        tt, sk = C.c_int32(), C.c_int32()
        assert lib.idb_gemm_plan(C.byref(d), C.byref(tt), C.byref(sk), None) == 0 and (tt.value, sk.value) == (verdict.tile, verdict.split_k)
        need = lib.idb_gemm_workspace_bytes(C.byref(d))
        if need > self.ws.numel():
            self.ws = torch.empty(need, dtype=torch.uint8, device=DEV)
        rc = lib.idb_gemm(C.byref(d), C.c_void_p(self.ws.data_ptr() if need else None), need, None)
        L.check(rc, f"idb_gemm {case.name} tile {tile} {feat}")
        out = bufs["out"]
        # ---- reference ----
        K = case.K
        acc, absp, A = self.acc(gn_key or "raw")
        extra = None
        if gn_key:                                  # one operand rounding of every normalised element
            u_op = GM.UNIT[self.dt]
            extra = u_op * absp
        if "wgroups" in f:
            acc2, absp2, _ = self.acc(gn_key or "raw", 1)
            sel = ((torch.arange(M, device=DEV) // bm) % 2 == 1)[:, None]
            acc, absp = torch.where(sel, acc2, acc), torch.where(sel, absp2, absp)
        if "ln" in f:
            st = self.ln_stats.double().sum(1)
            mean = st[:, 0] / K
            var = (st[:, 1] / K - mean * mean).clamp_min(0)
            rstd = (1.0 / torch.sqrt(var + 1e-5))[:, None]
            wabs = self.w.double().abs().sum(1)
            v = rstd * (acc - mean[:, None] * self.ln_u.double()) + self.ln_v.double()
            a = rstd * (absp + mean.abs()[:, None] * wabs) + self.ln_v.double().abs()
        else:
            scale = 0.5 if "f32" in f else 1.0
            v = acc * scale + self.bias.double()
            a = absp * scale + self.bias.double().abs()
        if "sb" in f:
            sb = self.sbias.double()[torch.arange(M, device=DEV) // case.hw]
            v, a = v + sb, a + sb.abs()
        if "gelu" in f:
            v, a = _gelu(v), 1.13 * a
        if "prelu" in f:
            v = torch.where(v >= 0, v, v * self.slope.double())
        if "relu" in f:
            v = v.clamp_min(0)
        if "geglu" in f:
            perm = torch.arange(n)
            blk, t = perm // 32, perm % 32
            perm = torch.where(t < 16, 16 * blk + t, n // 2 + 16 * blk + (t - 16)).to(DEV)
            vs, as_ = torch.empty_like(v), torch.empty_like(a)
            vs[:, perm], as_[:, perm] = v, a
            val, gate, av, ag = vs[:, :n // 2], vs[:, n // 2:], as_[:, :n // 2], as_[:, n // 2:]
            v = val * _gelu(gate)
            a = av * _gelu(gate).abs() + 1.13 * val.abs() * ag + av * ag
            assert extra is None                    # the fused GroupNorm is never planned with GEGLU
        if "res" in f:
            r = self.res.double()
            v, a = v + r, a + r.abs()
        odt_id = L.IDB_F32 if "f32" in f else self.dt
        what = f"{case.name} {self.tdt} tile {tile}->{verdict.tile} sk {verdict.split_k} {feat}"
        worst = GM.check(out, v, a, odt_id, K, what, extra)
        ro = out.double()
        if "out2" in f:
            want = (ro * self.out2_scale.double() + self.out2_shift.double()).float().to(self.tdt)
            assert torch.equal(bufs["out2"].view(torch.int16), want.view(torch.int16)), f"{what}: out2 is not the affine of the rounded out"
        if "gnp" in f:
            G, cpg = GM.GN_GROUPS, n // GM.GN_GROUPS
            x = ro.reshape(case.batch, case.hw // 64, 64, G, cpg)
            cnt = 64 * cpg
            want = torch.stack([x.sum(dim=(2, 4)), (x * x).sum(dim=(2, 4))], dim=-1)
            bnd = torch.stack([GM.sum_bound(x.abs().sum(dim=(2, 4)), cnt), GM.sum_bound((x * x).sum(dim=(2, 4)), cnt)], dim=-1)
            got = bufs["gnp"].double()
            r = ((got - want).abs() / bnd.clamp_min(1e-30)).nan_to_num(math.inf)
            assert r.max().item() <= 1.0, f"{what}: gn_partials off by {r.max().item():.3g} x the summation bound"
            worst = max(worst, r.max().item())
        if "rows" in f:
            want = torch.zeros(M, nt, 2, dtype=torch.float64, device=DEV)
            bnd = torch.zeros_like(want)
            for j in range(nt):
                x = ro[:, j * bn:(j + 1) * bn]
                want[:, j, 0], want[:, j, 1] = x.sum(1), (x * x).sum(1)
                bnd[:, j, 0], bnd[:, j, 1] = GM.sum_bound(x.abs().sum(1), x.shape[1]), GM.sum_bound((x * x).sum(1), x.shape[1])
            r = ((bufs["rows"].double() - want).abs() / bnd.clamp_min(1e-30)).nan_to_num(math.inf)
            assert r.max().item() <= 1.0, f"{what}: row statistics off by {r.max().item():.3g} x the summation bound"
            worst = max(worst, r.max().item())
        return worst


def _tag(case):
    return case.name


@pytest.mark.parametrize("dtname", list(DTYPES))
@pytest.mark.parametrize("case", GM.CASES, ids=_tag)
def test_gemm_matrix(lib, dtname, case):
    dt, tdt = DTYPES[dtname]
    data = CaseData(lib, case, dt, tdt, seed=1000 + GM.CASES.index(case))
    failures = []
    for feat in GM.FEATURES:
        if not GM.applicable(case, feat):
            continue
        for tile in range(110):
            v = GM.classify(lib, case, dt, tile, feat)
            if not v.accepted:
                if tile in GM.VARIANT_IDS:
                    _SUMMARY[(dtname, GM.family_of(tile))][1] += 1
                continue
            key = (dtname, GM.family_of(v.tile))
            try:
                worst = data.run(tile, feat, v)
            except AssertionError as e:
                failures.append(str(e))
                continue
            s = _SUMMARY[key]
            s[0] += 1
            s[2] = max(s[2], worst)
            _FEAT_WORST[(dtname, feat)] = max(_FEAT_WORST[(dtname, feat)], worst)
    torch.cuda.synchronize()
    assert not failures, f"{len(failures)} failing combinations:\n" + "\n".join(failures[:30])


def test_family_summary():
    """One line per (dtype, family): combinations run, refused, worst err / bound ratio.  Every family must have run."""
    if not _SUMMARY:
        pytest.skip("the matrix did not run in this session")
    for (dtname, fam), (runs, refused, worst) in sorted(_SUMMARY.items()):
        print(f"gemm matrix {dtname:4s} {fam:12s} run {runs:5d}  refused {refused:5d}  worst err/bound {worst:.3f}")
    for (dtname, feat), worst in sorted(_FEAT_WORST.items()):
        print(f"gemm matrix {dtname:4s} feature {feat:15s} worst err/bound {worst:.3f}")
    for dtname in DTYPES:
        for fam in GM.FAMILIES.values():
            assert _SUMMARY[(dtname, fam)][0] > 0, (dtname, fam)


# ------------------------------------------------------------------------------------------------------------------------------------
# large-grid plans: the SD-2.1 layer shapes of test_plan_table_cpu.py at B_eff 2 and 128 on the planner's own tile (tile = 0), checked on
# sampled rows (first and last row of every M tile, the rows around every image boundary, 256 random rows) against float64
# ------------------------------------------------------------------------------------------------------------------------------------
from test_plan_table_cpu import CONVS, LINEARS  # noqa: E402

_BIG = [("conv", c) for c in CONVS] + [("lin", l) for l in LINEARS]


def _rows_im2col(batch, oh, ow, stride, srcs, xs, rows):
    """im2col rows `rows` of a conv ([segment][tap][channel] K order, zero padding 1, nearest-2x upsampling) in float64."""
    hw = oh * ow
    b, p = rows // hw, rows % hw
    oy, ox = p // ow, p % ow
    cols = []
    for (ch, taps, ih, iw, up), x in zip(srcs, xs):
        if taps == 9:
            ky = torch.arange(3, device=DEV).repeat_interleave(3)
            kx = torch.arange(3, device=DEV).repeat(3)
            ly, lx = oy[:, None] * stride + ky[None] - 1, ox[:, None] * stride + kx[None] - 1
            lh, lw = ih << up, iw << up
            valid = (ly >= 0) & (ly < lh) & (lx >= 0) & (lx < lw)
            v = x[b[:, None], ly.clamp(0, lh - 1) >> up, lx.clamp(0, lw - 1) >> up].double() * valid[..., None]
            cols.append(v.reshape(len(rows), 9 * ch))
        else:
            cols.append(x[b, oy, ox].double())
    return torch.cat(cols, dim=1)


@pytest.mark.parametrize("dtname", list(DTYPES))
@pytest.mark.parametrize("beff", [2, 128])
@pytest.mark.parametrize("shape", _BIG, ids=lambda s: s[1][0])
def test_large_grid_plans_on_sampled_rows(lib, dtname, beff, shape):
    dt, tdt = DTYPES[dtname]
    kind, spec = shape
    g = torch.Generator(device=DEV).manual_seed(7)
    if kind == "conv":
        name, oh, src_spec, n, stride = spec
        ow, batch, geglu = oh, beff, 0
        srcs = [(c, taps, (oh * stride) >> up if taps == 9 else oh, (oh * stride) >> up if taps == 9 else oh, up) for c, taps, up in src_spec]
    else:
        name, rows, k, n, geglu = spec
        oh = ow = 1
        batch = beff * rows
        stride, srcs = 1, [(k, 1, 1, 1, 0)]
    M, K = batch * oh * ow, sum(c * t for c, t, *_ in srcs)
    xs = [torch.randn(batch, ih, iw, c, generator=g, device=DEV).to(tdt) for c, taps, ih, iw, up in srcs]
    w = (torch.randn(n, K, generator=g, device=DEV) * K ** -0.5).to(tdt)
    bias = torch.randn(n, generator=g, device=DEV)
    ncols = n // 2 if geglu else n
    out = torch.full((M, ncols), float("nan"), dtype=tdt, device=DEV)
    d = L.GemmDesc()
    d.dtype, d.batch, d.out_h, d.out_w, d.stride, d.n, d.nsrc = dt, batch, oh, ow, stride, n, len(srcs)
    for i, ((c, taps, ih, iw, up), x) in enumerate(zip(srcs, xs)):
        d.src[i].ptr, d.src[i].channels, d.src[i].taps, d.src[i].in_h, d.src[i].in_w, d.src[i].upsample = x.data_ptr(), c, taps, ih, iw, up
    d.w, d.bias, d.out, d.out_dtype, d.out_ld, d.geglu = w.data_ptr(), bias.data_ptr(), out.data_ptr(), dt, ncols, geglu
    # the features the engine asks for on such a layer: the time-embedding bias on a resnet conv1, the residual of attention / FF
    # outputs, the GroupNorm statistics of a conv output wherever the plan emits them without an extra launch
    sbias = res = gnp = None
    if kind == "conv" and len(srcs) == 1 and stride == 1 and not srcs[0][4]:
        sbias = torch.randn(batch, n, generator=g, device=DEV)
        d.sample_bias, d.sample_bias_ld = sbias.data_ptr(), n
    if kind == "lin" and (name.startswith("out_") or name.startswith("ffout_")):
        res = torch.randn(M, n, generator=g, device=DEV).to(tdt)
        d.residual = res.data_ptr()
    if kind == "conv" and oh * ow % 64 == 0 and oh * ow <= 4096 and lib.idb_gemm_emits_gn_partials(C.byref(d), GM.GN_GROUPS) > 0:
        gnp = torch.full((batch, oh * ow // 64, GM.GN_GROUPS, 2), float("nan"), device=DEV)
        d.gn_partials, d.gn_groups = gnp.data_ptr(), GM.GN_GROUPS
    t, sk = C.c_int32(), C.c_int32()
    assert lib.idb_gemm_plan(C.byref(d), C.byref(t), C.byref(sk), None) == 0
    need = lib.idb_gemm_workspace_bytes(C.byref(d))
    ws = torch.empty(max(need, 1), dtype=torch.uint8, device=DEV)
    L.check(lib.idb_gemm(C.byref(d), C.c_void_p(ws.data_ptr() if need else None), need, None), f"idb_gemm {name}")
    # sampled rows
    bm, _ = GM.tile_dims(t.value)
    starts = torch.arange(0, M, bm, device=DEV)
    hw = oh * ow
    bounds = torch.arange(hw, M, hw, device=DEV) if hw > 1 else torch.empty(0, dtype=torch.long, device=DEV)
    gen = torch.Generator(device=DEV).manual_seed(11)
    rows = torch.cat([starts, (starts + bm - 1).clamp_max(M - 1), bounds - 1, bounds, torch.randint(0, M, (256,), generator=gen, device=DEV)])
    rows = torch.unique(rows)
    if kind == "conv":
        A = _rows_im2col(batch, oh, ow, stride, srcs, xs, rows)
    else:
        A = xs[0].reshape(M, K)[rows].double()
    W = w.double()
    acc, absp = A @ W.t(), A.abs() @ W.abs().t()
    v, a = acc + bias.double(), absp + bias.double().abs()
    if sbias is not None:
        sbr = sbias.double()[rows // hw]
        v, a = v + sbr, a + sbr.abs()
    if geglu:
        perm = torch.arange(n)
        blk, tt = perm // 32, perm % 32
        perm = torch.where(tt < 16, 16 * blk + tt, n // 2 + 16 * blk + (tt - 16)).to(DEV)
        vs, as_ = torch.empty_like(v), torch.empty_like(a)
        vs[:, perm], as_[:, perm] = v, a
        val, gate, av, ag = vs[:, :n // 2], vs[:, n // 2:], as_[:, :n // 2], as_[:, n // 2:]
        v, a = val * _gelu(gate), av * _gelu(gate).abs() + 1.13 * val.abs() * ag + av * ag
    if res is not None:
        r = res[rows].double()
        v, a = v + r, a + r.abs()
    what = f"{name} B_eff {beff} {dtname} tile {t.value} sk {sk.value}"
    worst = GM.check(out[rows], v, a, dt, K, what)
    assert not torch.isnan(out).any().item(), f"{what}: unwritten output elements"
    if gnp is not None:
        G, cpg = GM.GN_GROUPS, n // GM.GN_GROUPS
        x = out.double().reshape(batch, hw // 64, 64, G, cpg)
        want = torch.stack([x.sum(dim=(2, 4)), (x * x).sum(dim=(2, 4))], dim=-1)
        bnd = torch.stack([GM.sum_bound(x.abs().sum(dim=(2, 4)), 64 * cpg), GM.sum_bound((x * x).sum(dim=(2, 4)), 64 * cpg)], dim=-1)
        r = ((gnp.double() - want).abs() / bnd.clamp_min(1e-30)).nan_to_num(math.inf)
        assert r.max().item() <= 1.0, f"{what}: gn_partials off by {r.max().item():.3g} x the summation bound"
    key = (dtname, "grid:" + GM.family_of(t.value))
    s = _SUMMARY_BIG[key]
    s[0] += 1
    s[1] = max(s[1], worst)


_SUMMARY_BIG = defaultdict(lambda: [0, 0.0])


def test_large_grid_summary():
    for (dtname, fam), (runs, worst) in sorted(_SUMMARY_BIG.items()):
        print(f"gemm large grids {dtname:4s} {fam:17s} run {runs:3d}  worst err/bound {worst:.3f}")
