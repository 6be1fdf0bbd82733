"""The test matrix of the trunk's kernels one C entry at a time (csrc/idb_block.hip: idb_blk_conv_forward / _dgrad / _wgrad,
idb_blk_bn_forward / _backward, idb_blk_affine, idb_blk_pack_images, idb_sgd_clip_step_table).  Shared by test_block_matrix_cpu.py
(plans through the library's host-only queries, references, emulations, teeth, argument checks) and test_block_matrix_gpu.py (launch
+ compare): the cases, the input recipes (integer hashing, no RNG), the float64 references, numpy emulations of the kernels'
arithmetic in the kernels' order, injectable defects and the element-wise criteria.  numpy plus the CPU pieces of frblock_oracle.py.

Why one entry at a time.  test_frblock_gpu.py drives whole blocks: 64 or 128 channels (one column tile), square maps, at most 3
statistic slices, and every stage inherits the error bounds of the stages in front of it.  Here every input is an exact fp32 value, so
every inherited term of the bounds below is 0 and what is left is the entry's own arithmetic; the cases are the smallest that reach a
second and third column tile, non-square maps, unequal and empty stride-parity classes, the slice caps and the ragged last slices.

Criteria.  u = 2^-24, v = 2^-53, SECOND = 1 + 2^-10 (frblock_oracle.py); none is measured.
  conv forward   a = prelu(fma(x, sc, sh)) is formed in the operand load: against its double evaluation it carries one rounding, one
                 more under the slope (`_recompute_bound`; 0 without the affine pair).  `_conv_bound`: (K + 2) u sum |a||w| +
                 sum ea |w|, K = taps cin.
  conv dgrad     `_dgrad_bound` with a gradient error of 0: (taps cout + 2) u sum |g||w|.  An input pixel that no tap reaches has the
                 bound 0, that is equality, and its bits must be +0.
  conv wgrad     `_wgrad_bound` with a gradient error of 0 and the recomputed activation's ea: (M + 2) u sum |g||a| + sum |g| ea.
  load path      conv_forward(x, affine, slope) against conv_forward(idb_blk_affine(x, affine, slope), NULL, NULL), and the same for
                 wgrad: bit for bit (act4 is one function and the MFMA order does not depend on where the operand came from).
  bn forward     `_stat_bound` with ec = 0: |d mean| <= (R + 4) v spread, d var, d invstd, d sc, d sh from it; `_running_bound`.  The
                 reference takes mean and variance of x - x[0] in float64 (an exact difference of fp32 values) and adds x[0] back, so
                 that a channel with a large offset and a tiny spread is not lost in the reference itself.  `stat` is stored in double:
                 the mean's bound gets v |mean| for that one rounding (the oracle's term is relative to the spread alone, and 1e4 + m
                 cannot be stored to within 257 v 1e-2), carried into sh and the running mean.  In eval mode the mean is the running
                 mean itself: bound 0.
  bn backward    `_bn_backward_bound` with eg = eadd = 0.  `stat` and `affine` are the test's own arrays, the same on both sides; the
                 affine pairs are exact binary fractions, so y = fma(c, sc, sh) is exact in double and the planted y == 0 and
                 y == +-2^-126 are what they are called.
  affine         `_act_bound` with no inherited term: u |y| (+ the slope's rounding); with an identity (e3 + eid) SECOND + u |out| as
                 block_forward forms it.
  bit-equal      idb_blk_pack_images (a copy, the fourth channel +0), the exact zeros of dgrad, a repeat of any call, dgrad whatever
                 affine and slope the descriptor carries (it reads neither).
  sgd table      frtail_oracle.sgd_step / sgd_bound.

The emulations (fp32 fma chains for the products, double sums in the kernel's slice, thread-group, lane and butterfly order for the
statistics) must meet every bound at err / bound <= 0.5.  Bounds asked WHOLE of the emulation (<= 1), because the quantity is a
double-precision value rounded once to fp32 and a correctly rounded value attains u |value|: sc and sh, the running statistics,
d beta / d gamma / d slope, g_c and the affine outputs (attained shares are printed by test_summary of the CPU file: up to 0.99).

DEFECTS lists what is injected into the emulations; DEFECT_CASES names the case each must fail.  There is no harmless defect."""
import math
from functools import lru_cache

import numpy as np

import frblock_oracle as BO
import frtail_oracle as TO
from matrix_common import F32, F64, GUARD, NAN32, check, describe, fma32  # noqa: F401  (re-exported to the two test files)

U32, U64, SECOND = TO.U32, TO.U64, TO.SECOND
TM, TK, FILL, MAX_WSLICES, MAX_SSLICES = 128, 32, 256, 64, 1024


def _q(a):
    """Values rounded to fp32, held in float64."""
    return np.asarray(a, F64).astype(F32).astype(F64)


def _align(b):
    return (b + 255) & ~255


# ------------------------------------------------------------------------------------------------------------------------------------
# convolutions
# ------------------------------------------------------------------------------------------------------------------------------------
# (B, H, W, cin, cout, k, stride)
CONV_CASES = ((2, 3, 5, 192, 256, 3, 1), (2, 3, 5, 256, 192, 3, 2), (2, 6, 7, 192, 64, 3, 2), (2, 5, 4, 128, 192, 1, 2),
              (3, 7, 6, 64, 128, 1, 1), (2, 1, 5, 64, 64, 3, 2), (2, 5, 1, 64, 128, 3, 2), (1, 1, 127, 64, 64, 3, 1),
              (1, 3, 43, 64, 64, 3, 1), (2, 57, 59, 64, 64, 3, 1), (1, 100, 101, 4, 64, 3, 1), (2, 5, 7, 4, 64, 3, 2))
CONV_MODES = ("prelu", "affine", "plain")          # affine + slope | affine only | neither


def conv_modes(case):
    return CONV_MODES if case[3] != 4 else ("plain",)      # the stem's conv reads the packed images as they are


def conv_geo(case):
    B, H, W, cin, cout, k, s = case
    pad = 1 if k == 3 else 0
    Ho, Wo = (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1
    return dict(B=B, H=H, W=W, cin=cin, cout=cout, k=k, s=s, pad=pad, Ho=Ho, Wo=Wo, taps=k * k, K=k * k * cin, Mo=B * Ho * Wo)


def col_tile(ch):
    """The column-tile rule: 128 columns when the channel count is a multiple of 128, else 64."""
    return 128 if ch % 128 == 0 else 64


def class_dims(g, py, px):
    s = g["s"]
    return ((g["H"] - py + s - 1) // s if py < g["H"] else 0), ((g["W"] - px + s - 1) // s if px < g["W"] else 0)


def conv_plan(case):
    """conv_plan of idb_block.hip restated: grids of the three kernels, the wgrad slicing and workspace."""
    g = conv_geo(case)
    s, Mo, K, cout = g["s"], g["Mo"], g["K"], g["cout"]
    hc, wc = class_dims(g, 0, 0)
    p = dict(fwd_row_tiles=-(-Mo // TM), fwd_col_tiles=cout // col_tile(cout), dgrad_row_tiles=-(-(g["B"] * hc * wc) // TM),
             dgrad_col_tiles=g["cin"] // col_tile(g["cin"]) if g["cin"] % 64 == 0 else 0, classes=s * s,
             class_rows=tuple(g["B"] * h * w for h, w in (class_dims(g, z // s, z % s) for z in range(s * s))),
             k_tiles=-(-K // TM), wgrad_col_tiles=cout // col_tile(cout))
    steps = -(-Mo // TK)
    ks = max(1, min(FILL // (p["k_tiles"] * p["wgrad_col_tiles"]), steps // 4, MAX_WSLICES))
    p["per"] = -(-steps // ks)
    p["slices"] = -(-steps // p["per"])
    p["last_slice_rows"] = Mo - (p["slices"] - 1) * p["per"] * TK
    p["bytes"] = _align(4 * p["slices"] * cout * K)
    return p


# what each case is in the matrix for: the figures of the plan it must have (asserted on the CPU, with the library's own queries)
CONV_REACHES = {
    CONV_CASES[0]: dict(fwd_col_tiles=2, wgrad_col_tiles=2, dgrad_col_tiles=3, k_tiles=14),            # K = 1728 = 13.5 tiles: ragged
    CONV_CASES[1]: dict(fwd_col_tiles=3, wgrad_col_tiles=3, dgrad_col_tiles=2, classes=4, class_rows=(12, 8, 6, 4)),
    CONV_CASES[2]: dict(classes=4, class_rows=(24, 18, 24, 18), dgrad_col_tiles=3),
    CONV_CASES[3]: dict(classes=4, class_rows=(12, 12, 8, 8), fwd_col_tiles=3),
    CONV_CASES[4]: dict(classes=1, fwd_col_tiles=1, k_tiles=1),
    CONV_CASES[5]: dict(classes=4, class_rows=(6, 4, 0, 0)),
    CONV_CASES[6]: dict(classes=4, class_rows=(6, 0, 4, 0)),
    CONV_CASES[7]: dict(fwd_row_tiles=1, dgrad_row_tiles=1),                                           # Mo = 127
    CONV_CASES[8]: dict(fwd_row_tiles=2, dgrad_row_tiles=2),                                           # Mo = 129
    CONV_CASES[9]: dict(fwd_row_tiles=53, dgrad_row_tiles=53, per=5, slices=43, last_slice_rows=6, k_tiles=5),
    CONV_CASES[10]: dict(per=5, slices=64, last_slice_rows=20, k_tiles=1, dgrad_col_tiles=0),
    CONV_CASES[11]: dict(dgrad_col_tiles=0, classes=4, k_tiles=1),
}
CONV_MO = {CONV_CASES[7]: 127, CONV_CASES[8]: 129, CONV_CASES[9]: 6726, CONV_CASES[10]: 10100}


@lru_cache(maxsize=None)
def conv_inputs(case):
    """x [B, H, W, cin], w [cout, k, k, cin], g [B, Ho, Wo, cout], affine [2, cin], slope [cin]: fp32 values in float64."""
    B, H, W, cin, cout, k, s = case
    g = conv_geo(case)
    salt = 7919 * (B + 3 * H + 5 * W) + 13 * cin + 7 * cout + 3 * k + s
    idx = np.arange(cin)
    scale = 0.5 + 1.5 * (TO._h(idx + 17, 97) / 96.0)
    shift = (TO._h(idx + 5, 61) - 30) / 20.0
    x = BO._u((B, H, W, cin), salt) * scale + shift
    w = BO._u((cout, k, k, cin), salt + 101) * np.sqrt(3.0 / g["K"])
    go = BO._u((B, g["Ho"], g["Wo"], cout), salt + 211, 513)
    sc = np.where(TO._h(idx + 3, 2) == 0, -1.0, 1.0) * (0.5 + TO._h(idx + 29, 65) / 64.0)
    sh = (TO._h(idx + 31, 41) - 20) / 16.0
    slope = 0.05 + 0.35 * TO._h(idx + 19, 71) / 70.0
    return tuple(_q(a) for a in (x, w, go, np.stack([sc, sh]), slope))


def conv_operands(case, mode):
    """(x, w, g, affine or None, slope or None) of a mode."""
    x, w, go, aff, sl = conv_inputs(case)
    return x, w, go, (aff if mode != "plain" else None), (sl if mode == "prelu" else None)


@lru_cache(maxsize=None)
def conv_reference(case, mode, op):
    """(float64 reference, per-element bound) of op in ("fwd", "dgrad", "wgrad")."""
    x, w, go, aff, sl = conv_operands(case, mode)
    s = case[6]
    if op == "dgrad":
        return BO.conv_dgrad(go, w, s, x.shape), BO._dgrad_bound(go, 0.0 * go, w, s, x.shape)
    a = BO.act(x, aff, sl) if aff is not None else x
    ea = BO._recompute_bound(x, aff, sl) if aff is not None else 0.0 * x
    if op == "fwd":
        return BO.conv_fwd(a, w, s), BO._conv_bound(a, ea, w, s)
    return BO.conv_wgrad(go, a, w.shape, s), BO._wgrad_bound(go, 0.0 * go, a, ea, w.shape, s)


def no_tap_mask(case):
    """[H, W] True where no tap of the convolution reaches the input pixel: dgrad must write an exact +0 there."""
    g = conv_geo(case)
    m = np.ones((g["H"], g["W"]), bool)
    for oy in range(g["Ho"]):
        for ox in range(g["Wo"]):
            for ky in range(g["k"]):
                for kx in range(g["k"]):
                    y, x = oy * g["s"] - g["pad"] + ky, ox * g["s"] - g["pad"] + kx
                    if 0 <= y < g["H"] and 0 <= x < g["W"]:
                        m[y, x] = False
    return m


# ---- emulations: fp32 fma chains in the kernels' index arithmetic ---------------------------------------------------------------------
def act32(x, aff, sl):
    """act4: fma(x, sc, sh) rounded once, then the slope's product on the non-positive side."""
    if aff is None:
        return x.astype(F32)
    y = fma32(x.astype(F32), np.broadcast_to(aff[0].astype(F32), x.shape), np.broadcast_to(aff[1].astype(F32), x.shape)).reshape(x.shape)
    return y if sl is None else np.where(y > 0, y, sl.astype(F32) * y).astype(F32)


def _step(acc, a_col, b_row):
    """acc[i, j] = fl32(a_col[i] b_row[j] + acc[i, j]): the product is exact in float64."""
    return (a_col.astype(F64)[:, None] * b_row.astype(F64)[None, :] + acc).astype(F32)


def _patches(case, a, padval, defect):
    """The forward's and wgrad's operand rows: per tap, [Mo, cin] with the kernel's row decomposition."""
    g = conv_geo(case)
    m = np.arange(g["Mo"])
    b = m // (g["Ho"] * g["Wo"])
    rem = m - b * (g["Ho"] * g["Wo"])
    oy = rem // (g["Ho"] if defect == "rows_by_ho" else g["Wo"])
    ox = rem - oy * g["Wo"]
    for tap in range(g["taps"]):
        ky, kx = tap // g["k"], tap % g["k"]
        iy, ix = oy * g["s"] - g["pad"] + ky, ox * g["s"] - g["pad"] + kx
        ok = (iy >= 0) & (iy < g["H"]) & (ix >= 0) & (ix < g["W"])
        yield tap, np.where(ok[:, None], a[b, np.clip(iy, 0, g["H"] - 1), np.clip(ix, 0, g["W"] - 1)], padval)


def _operand(case, mode, defect):
    x, w, go, aff, sl = conv_operands(case, mode)
    a = act32(x, aff, sl)
    padval = act32(np.zeros((1, case[3])), aff, sl) if defect == "pad_act0" else np.zeros((1, case[3]), F32)
    return a, padval, w.astype(F32), go.astype(F32)


def emulate_conv_fwd(case, mode, defect=None):
    g = conv_geo(case)
    a, padval, w, _ = _operand(case, mode, defect)
    out = np.full((g["Mo"], g["cout"]), np.nan, F32)
    tile = col_tile(g["cout"])
    pats = list(_patches(case, a, padval, defect))
    for n0 in range(0, g["cout"], tile):
        acc = np.zeros((g["Mo"], tile), F32)
        for tap, av in pats:
            wt = w[n0:n0 + tile, tap // g["k"], tap % g["k"]]
            for ci in range(g["cin"]):
                acc = _step(acc, av[:, ci], wt[:, ci])
        dst = 0 if defect == "fwd_n0" else n0
        out[:, dst:dst + tile] = acc
    return out.reshape(g["B"], g["Ho"], g["Wo"], g["cout"])


def _c_rem(v, s):
    return int(math.fmod(v, s))      # C's %: the sign of the dividend


def emulate_conv_dgrad(case, defect=None):
    g = conv_geo(case)
    _, w, go, _, _ = conv_operands(case, "plain")
    w, go = w.astype(F32), go.astype(F32)
    s, pad, k = g["s"], g["pad"], g["k"]
    gi = np.full((g["B"], g["H"], g["W"], g["cin"]), np.nan, F32)
    tile = col_tile(g["cin"])
    for py in range(s):
        for px in range(s):
            Hc, Wc = class_dims(g, py, px)
            if defect == "class_floor":
                Hc, Wc = max(g["H"] - py, 0) // s, max(g["W"] - px, 0) // s
            Mc = g["B"] * Hc * Wc
            if Mc == 0:
                continue
            if defect == "parity_c_rem":
                reach = lambda v: _c_rem(v, s) != 1      # noqa: E731  (-1 % 2 is -1 in C: an odd negative passes)
            else:
                reach = lambda v: v % s == 0             # noqa: E731
            taps = [(ky, kx) for ky in range(k) for kx in range(k) if reach(py + pad - ky) and reach(px + pad - kx)]
            if not taps and defect == "notap_untouched":
                continue
            m = np.arange(Mc)
            b = m // (Hc * Wc)
            rem = m - b * (Hc * Wc)
            yc = rem // Wc
            xc = rem - yc * Wc
            for n0 in range(0, g["cin"], tile):
                acc = np.zeros((Mc, tile), F32)
                for ky, kx in taps:
                    ny, nx = py + s * yc + pad - ky, px + s * xc + pad - kx
                    oy, ox = np.abs(ny) // s, np.abs(nx) // s          # C's truncation; the negative ones are refused below
                    ok = (ny >= 0) & (nx >= 0) & (oy < g["Ho"]) & (ox < g["Wo"])
                    gv = np.where(ok[:, None], go[b, np.clip(oy, 0, g["Ho"] - 1), np.clip(ox, 0, g["Wo"] - 1)], F32(0))
                    for co in range(g["cout"]):
                        acc = _step(acc, gv[:, co], w[co, ky, kx, n0:n0 + tile])
                dst = 0 if defect == "dgrad_n0" else n0
                gi[b, py + s * yc, px + s * xc, dst:dst + tile] = acc
    return gi


def emulate_conv_wgrad(case, mode, defect=None):
    g, p = conv_geo(case), conv_plan(case)
    a, padval, _, go = _operand(case, mode, defect)
    A = np.zeros((g["Mo"], g["K"]), F32)
    for tap, av in _patches(case, a, padval, defect):
        A[:, tap * g["cin"]:(tap + 1) * g["cin"]] = av
    G = go.reshape(g["Mo"], g["cout"])
    part = np.zeros((p["slices"], g["cout"], g["K"]), F32)
    for z in range(p["slices"]):
        mfirst = z * p["per"] * TK
        mlast = min(g["Mo"], mfirst + p["per"] * TK)
        if defect == "ragged_stage":
            mlast = mfirst + (mlast - mfirst) // TK * TK
        acc = part[z]
        for m in range(mfirst, mlast):
            acc = _step(acc, G[m], A[m])
        part[z] = acc
    total = np.zeros((g["cout"], g["K"]), F64)
    for z in range(min(p["slices"], 32) if defect == "slices_past_32" else p["slices"]):
        total = total + part[z]
    dw = total.astype(F32)
    if defect == "wgrad_j0":
        tile, moved = col_tile(g["cout"]), np.full_like(dw, np.nan)
        moved[:tile] = dw[-tile:]
        dw = moved
    return dw.reshape(g["cout"], g["k"], g["k"], g["cin"])


# ------------------------------------------------------------------------------------------------------------------------------------
# BatchNorm forward / backward and the affine kernel
# ------------------------------------------------------------------------------------------------------------------------------------
BN_ROWS = (2, 255, 256, 257, 16385, 33275, 262145, 307193)
BN_CAP_ROWS = (262145, 307193)                      # above 1024 slices of 256 rows: ch == 64 only (79 MB per array at the larger)
BN_CH = (64, 192)
# rows -> (rows per slice, slices, rows of the last slice)
BN_PLAN = {2: (2, 1, 2), 255: (255, 1, 255), 256: (256, 1, 256), 257: (129, 2, 128), 16385: (253, 65, 193), 33275: (256, 130, 251),
           262145: (257, 1021, 5), 307193: (300, 1024, 293)}
EPS, MOMENTUM = BO.EPS, BO.MOMENTUM
OFFSET_CH, CONST_CH, INF_CH = 5, 9, 11


def bn_cases():
    return [(r, ch) for r in BN_ROWS for ch in BN_CH if ch == 64 or r not in BN_CAP_ROWS]


def bn_plan(rows, ch):
    ss = min(-(-rows // 256), MAX_SSLICES)
    per = -(-rows // ss)
    slices = -(-rows // per)
    return dict(per=per, slices=slices, last=rows - (slices - 1) * per, bytes=_align(8 * 3 * slices * ch) + _align(8 * 2 * ch))


@lru_cache(maxsize=4)
def bn_inputs(rows, ch, plant=None):
    """x [rows, ch] and the parameters {weight, bias, running_mean, running_var} under the key "bn".  Channel OFFSET_CH: offset about
    1e4, spread about 1e-2 (ten units in the last place of fp32 there).  plant "const": channel CONST_CH constant (for eps == 0);
    "inf": one +inf in channel INF_CH."""
    idx = np.arange(ch)
    scale = 0.5 + 1.5 * (TO._h(idx + 17, 97) / 96.0)
    shift = (TO._h(idx + 5, 61) - 30) / 20.0
    x = BO._u((rows, ch), 1000003 + 31 * rows + ch) * scale + shift
    x[:, OFFSET_CH] = 1e4 + 1e-2 * BO._u((rows,), 77 + rows)
    if plant == "const":
        x[:, CONST_CH] = 1.25
    if plant == "inf":
        x[rows // 2, INF_CH] = np.inf
    prm = {}
    BO._bn_params(prm, "bn", ch, 7, big_shift=True)
    x = _q(x)
    x.setflags(write=False)
    return x, BO._f32(prm)


def bn_forward_reference(x, prm, training=True, eps=EPS, momentum=MOMENTUM):
    """-> (values, bounds): dicts of mean, invstd (double), sc, sh, running_mean, running_var (fp32)."""
    gam, beta, rm, rv = (prm[f"bn.{k}"] for k in ("weight", "bias", "running_mean", "running_var"))
    R = x.shape[0]
    with np.errstate(all="ignore"):
        if training:
            st, _, var, _ = BO.bn_forward(x - x[0], prm, "bn", True, eps, momentum)
            mean, inv = x[0] + st[0], st[1]
            run_m, run_v = (1 - momentum) * rm + momentum * mean, (1 - momentum) * rv + momentum * var * (R / (R - 1.0))
        else:
            mean, inv, run_m, run_v = rm, 1.0 / np.sqrt(rv + eps), rm, rv
        sc = gam * inv
        sh = beta - mean * sc
        stat, aff = np.stack([mean, inv]), np.stack([sc, sh])
        em, ev, ei, esc, esh = BO._stat_bound(x, 0.0, stat, prm, "bn", aff, training)
        if training:
            em = em + U64 * np.abs(mean)                      # the stored double
            esh = esh + np.abs(sc) * U64 * np.abs(mean)
        val = dict(mean=mean, invstd=inv, sc=sc, sh=sh, running_mean=run_m, running_var=run_v)
        bound = dict(mean=em, invstd=ei, sc=esc, sh=esh, running_mean=0.0 * rm, running_var=0.0 * rv)
        if training:
            rb = BO._running_bound({"bn.running_mean": run_m, "bn.running_var": run_v}, "bn", em, ev, R, momentum)
            bound.update(running_mean=rb["bn.running_mean"], running_var=rb["bn.running_var"])
    return val, bound


def ordered_sums(terms, rows, per, slices, defect=None):
    """Column sums of [rows, ch] float64 arrays in the kernels' order: per slice four thread groups (rows first + g, + 4, ...) added
    ((0 + 1) + 2) + 3; per channel lane l of a wave takes slices l, l + 64, ... ascending; the xor butterfly 32, 16, ..., 1."""
    if defect == "per_256":
        per = 256
        slices = min(-(-rows // 256), MAX_SSLICES)
    if defect == "tail_dropped":
        slices = max(rows // per, 1)
    out = []
    for t in terms:
        ch = t.shape[1]
        n = slices * per
        t = t[:n] if n <= rows else np.concatenate([t, np.zeros((n - rows, ch))])      # s + 0.0 == s
        t = t.reshape(slices, per, ch)
        grp = []
        for g in range(4):
            s = np.zeros((slices, ch))
            for r in range(g, per, 4):
                s = s + t[:, r]
            grp.append(s)
        part = ((grp[0] + grp[1]) + grp[2]) + grp[3]
        lanes = np.zeros((64, ch))
        for i in range(slices if defect != "merge_first_pass" else min(slices, 64)):
            lanes[i % 64] += part[i]
        for o in (32, 16, 8, 4, 2, 1):
            lanes = lanes + lanes[np.arange(64) ^ o]
        out.append(lanes[0])
    return out


def emulate_bn_forward(x, prm, training=True, eps=EPS, momentum=MOMENTUM, defect=None):
    gam, beta, rm, rv = (prm[f"bn.{k}"] for k in ("weight", "bias", "running_mean", "running_var"))
    rows, ch = x.shape
    p = bn_plan(rows, ch)
    with np.errstate(all="ignore"):
        if training:
            x0 = x[0] if defect != "no_shift" else np.zeros(ch)
            d = (x.astype(F32) - x[0].astype(F32)).astype(F64) if defect == "shift_fp32" else x - x0
            s1, s2 = ordered_sums([d, d * d], rows, p["per"], p["slices"], defect)
            n = float(rows)
            m = s1 / n
            mean = x0 + m
            var = np.maximum((s2 - s1 * m) / n, 0.0)
            run_m = ((1.0 - momentum) * rm + momentum * mean).astype(F32)
            run_v = ((1.0 - momentum) * rv + momentum * (var * (n / (n - 1.0)))).astype(F32)
        else:
            mean, var, run_m, run_v = rm, rv, rm.astype(F32), rv.astype(F32)
        inv = 1.0 / np.sqrt(var + eps)
        sc = gam * inv
        bad = ~(np.abs(mean) <= 1.7e308) | ~(var <= 1.7e308)
        flags = (int(bad.any()), int((~bad & (var + eps == 0.0)).any()))
        return dict(mean=mean, invstd=inv, sc=sc.astype(F32), sh=(beta - mean * sc).astype(F32), running_mean=run_m, running_var=run_v,
                    flags=flags)


# ---- backward and affine -------------------------------------------------------------------------------------------------------------
_SC = (2.0, -0.5, 1.5, 0.25)
_SH = (-1.0, 0.5, 0.0, 0.75)
Y0_CH, TINY_CH = 0, 1          # channel 0: sc 2, sh -1, c = 0.5 gives y == 0; channel 1: sc 2, sh 0, c = +-2^-127 gives y = +-2^-126


@lru_cache(maxsize=4)
def bnb_inputs(rows, ch):
    """c, g, add [rows, ch]; stat [2, ch] (any mean, invstd: the backward takes them as given); affine, id_affine [2, ch] of exact
    binary fractions; gamma, slope [ch].  Planted in rows 0 and 1: y == 0 twice (g of both signs), y == +2^-126 and -2^-126."""
    idx = np.arange(ch)
    c = BO._u((rows, ch), 500009 + 17 * rows + ch) * 2.0
    g = BO._u((rows, ch), 91 + rows, 513)
    add = BO._u((rows, ch), 291 + rows, 1025) * 0.5
    pick = TO._h(idx + 43, 4)
    sc, sh = np.asarray(_SC)[pick], np.asarray(_SH)[TO._h(idx + 47, 4)]
    sc[[Y0_CH, TINY_CH]], sh[[Y0_CH, TINY_CH]] = 2.0, (-1.0, 0.0)
    c[0, Y0_CH] = c[1, Y0_CH] = 0.5
    g[0, Y0_CH], g[1, Y0_CH] = 0.75, -0.625
    c[0, TINY_CH], c[1, TINY_CH] = 2.0 ** -127, -(2.0 ** -127)
    g[0, TINY_CH] = g[1, TINY_CH] = 0.5
    stat = np.stack([(TO._h(idx + 53, 41) - 20) / 32.0, 0.5 + 1.5 * TO._h(idx + 59, 97) / 96.0])
    id_aff = np.stack([np.asarray(_SC)[TO._h(idx + 61, 4)], np.asarray(_SH)[TO._h(idx + 67, 4)]])
    gamma = np.where(TO._h(idx + 71, 2) == 0, -1.0, 1.0) * (0.8 + 0.4 * TO._h(idx + 3, 101) / 100.0)
    slope = 0.05 + 0.35 * TO._h(idx + 19, 71) / 70.0
    out = dict(c=_q(c), g=_q(g), add=_q(add), stat=stat, affine=np.stack([sc, sh]), id_affine=id_aff, gamma=_q(gamma), slope=_q(slope))
    for a in out.values():
        a.setflags(write=False)
    return out


BNB_FORMS = ((False, False), (True, False), (False, True), (True, True))          # (slope, add)


def bn_backward_reference(rows, ch, with_slope, with_add):
    """-> (values, bounds): dicts of gc, gamma, beta and, under a slope, slope."""
    i = bnb_inputs(rows, ch)
    sl, add = (i["slope"] if with_slope else None), (i["add"] if with_add else None)
    gc, dgam, dbeta, dsl, r = BO.bn_backward(i["c"], i["g"], i["stat"], i["affine"], i["gamma"], sl, add)
    b = BO._bn_backward_bound(i["c"], i["g"], 0.0 * i["g"], i["stat"], i["affine"], i["gamma"], sl, add, None if add is None else 0.0 * add, r)
    val = dict(gc=gc, gamma=dgam, beta=dbeta)
    if with_slope:
        val["slope"] = dsl
    return val, {k: b[k] for k in val}


def emulate_bn_backward(rows, ch, with_slope, with_add, defect=None):
    i = bnb_inputs(rows, ch)
    p = bn_plan(rows, ch)
    c, g, mean, inv = i["c"], i["g"], i["stat"][0], i["stat"][1]
    y = fma32(c.astype(F32), np.broadcast_to(i["affine"][0].astype(F32), c.shape), np.broadcast_to(i["affine"][1].astype(F32), c.shape))
    y = y.reshape(c.shape)
    gy = g
    if with_slope:
        gy = np.where((y >= 0) if defect == "y0_takes_g" else (y > 0), g, i["slope"] * g)
    xh = (c - mean) * inv
    ym = np.where(y > 0, y, F32(0)) if defect == "s3_pos" else np.where(y < 0, y, F32(0))
    s1, s2, s3 = ordered_sums([gy, gy * xh, g * ym.astype(F64)], rows, p["per"], p["slices"], defect)
    v = i["gamma"] * inv * (gy - s1 / float(rows) - xh * (s2 / float(rows)))
    if with_add and defect != "add_skipped":
        v = v + i["add"]
    out = dict(gc=v.astype(F32), gamma=s2.astype(F32), beta=s1.astype(F32))
    if with_slope:
        out["slope"] = s3.astype(F32)
    return out


AFFINE_FORMS = tuple((sl, idn) for idn in ("none", "plain", "affine") for sl in (False, True))


def affine_reference(rows, ch, with_slope, identity):
    i = bnb_inputs(rows, ch)
    sl = i["slope"] if with_slope else None
    e = BO._act_bound(i["c"], 0.0, i["affine"], 0.0, 0.0, sl)
    out = BO.act(i["c"], i["affine"], sl)
    if identity == "none":
        return out, e
    idn = i["add"] if identity == "plain" else BO.act(i["add"], i["id_affine"])
    eid = 0.0 if identity == "plain" else BO._act_bound(i["add"], 0.0, i["id_affine"], 0.0, 0.0)
    out = out + idn
    return out, (e + eid) * SECOND + U32 * np.abs(out)


def emulate_affine(rows, ch, with_slope, identity, defect=None):
    i = bnb_inputs(rows, ch)
    sl = i["slope"] if with_slope else None
    v = act32(i["c"], i["affine"], sl)
    if identity == "none":
        return v
    d = i["add"].astype(F32)
    if identity == "affine":
        d = act32(i["add"], i["id_affine"], sl if defect == "prelu_on_identity" else None)
    elif defect == "prelu_on_identity" and sl is not None:
        d = np.where(d > 0, d, sl.astype(F32) * d).astype(F32)
    return (v + d).astype(F32)


# ------------------------------------------------------------------------------------------------------------------------------------
# pack and the table SGD
# ------------------------------------------------------------------------------------------------------------------------------------
PACK_SHAPES = ((1, 1, 1), (1, 3, 5), (2, 15, 17), (3, 16, 16))          # 510 pixels: a ragged second block; 768: three whole blocks


def pack_input(shape):
    b, h, w = shape
    return BO._u((b, 3, h, w), 4242 + b + 7 * h).astype(F32)


def pack_reference(shape):
    img = pack_input(shape)
    out = np.zeros(shape + (4,), F32)
    out[..., :3] = np.transpose(img, (0, 2, 3, 1))
    return out


def emulate_pack(shape, defect=None):
    b, h, w = shape
    img = pack_input(shape).reshape(-1)
    hw = w * w if defect == "hw_from_w" else h * w
    i = np.arange(b * h * w)
    bb = i // hw
    s = bb * 3 * hw + (i - bb * hw)
    out = np.zeros((b * h * w, 4), F32)
    for k in range(3):
        out[:, k] = np.take(img, s + k * hw, mode="wrap")      # a wrong hw leaves the image; the emulation wraps
    return out.reshape(b, h, w, 4)


SGD_COUNTS = (1, 1024)


def sgd_sizes(count):
    return tuple(1 + (37 * i) % 300 for i in range(count))


# ------------------------------------------------------------------------------------------------------------------------------------
# defects and the named case each must fail
# ------------------------------------------------------------------------------------------------------------------------------------
HARMLESS = ()
DEFECTS = ("fwd_n0", "dgrad_n0", "wgrad_j0", "rows_by_ho", "class_floor", "parity_c_rem", "notap_untouched", "ragged_stage",
           "slices_past_32", "pad_act0", "merge_first_pass", "tail_dropped", "shift_fp32", "no_shift", "per_256", "y0_takes_g", "s3_pos",
           "add_skipped", "prelu_on_identity", "hw_from_w")
DEFECT_CASES = {
    "fwd_n0": ("conv", "fwd", CONV_CASES[1], "affine"),
    "dgrad_n0": ("conv", "dgrad", CONV_CASES[0], "plain"),
    "wgrad_j0": ("conv", "wgrad", CONV_CASES[1], "plain"),
    "rows_by_ho": ("conv", "fwd", CONV_CASES[0], "plain"),
    "class_floor": ("conv", "dgrad", CONV_CASES[1], "plain"),
    "parity_c_rem": ("conv", "dgrad", CONV_CASES[2], "plain"),
    "notap_untouched": ("conv", "dgrad", CONV_CASES[3], "plain"),
    "ragged_stage": ("conv", "wgrad", CONV_CASES[11], "plain"),
    "slices_past_32": ("conv", "wgrad", CONV_CASES[10], "plain"),
    "pad_act0": ("conv", "fwd", CONV_CASES[0], "prelu"),
    "merge_first_pass": ("bn_fwd", 16385, 64),
    "tail_dropped": ("bn_fwd", 257, 192),
    "shift_fp32": ("bn_fwd", 257, 64),
    "no_shift": ("bn_fwd", 257, 64),
    "per_256": ("bn_fwd", 262145, 64),
    "y0_takes_g": ("bn_bwd", 2, 64, True, False),
    "s3_pos": ("bn_bwd", 255, 64, True, True),
    "add_skipped": ("bn_bwd", 257, 192, False, True),
    "prelu_on_identity": ("affine", 255, 64, True, "plain"),
    "hw_from_w": ("pack", (1, 3, 5)),
}


def judge_all(got, ref, bound):
    """check() over a dict of outputs: (all within bounds, the worst share)."""
    res = {k: check(np.asarray(got[k], F64).reshape(np.shape(ref[k])), ref[k], bound[k]) for k in ref}
    return all(r[0] for r in res.values()), res


def defect_fails(defect):
    """True when `defect`, injected into the emulation of its named case, violates that case's criterion."""
    kind, *key = DEFECT_CASES[defect]
    if kind == "conv":
        op, case, mode = key
        ref, bound = conv_reference(case, mode, op)
        emu = emulate_conv_dgrad(case, defect) if op == "dgrad" else (emulate_conv_fwd if op == "fwd" else emulate_conv_wgrad)(case, mode, defect)
        return not check(emu, ref, bound)[0]
    if kind == "bn_fwd":
        x, prm = bn_inputs(*key)
        ref, bound = bn_forward_reference(x, prm)
        emu = emulate_bn_forward(x, prm, defect=defect)
        return not judge_all(emu, ref, bound)[0]
    if kind == "bn_bwd":
        ref, bound = bn_backward_reference(*key)
        return not judge_all(emulate_bn_backward(*key, defect=defect), ref, bound)[0]
    if kind == "affine":
        ref, bound = affine_reference(*key)
        return not check(emulate_affine(*key, defect=defect), ref, bound)[0]
    return not np.array_equal(emulate_pack(key[0], defect).view(np.uint32), pack_reference(key[0]).view(np.uint32))
