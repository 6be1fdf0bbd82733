"""The test matrix of idb_groupnorm_bwd (csrc/idb_gnbwd.hip), shared by test_gnbwd_matrix_cpu.py (refusals, plan query, emulation, teeth)
and test_gnbwd_matrix_gpu.py (launch and compare): cases, input recipes, a float64 reference, a numpy emulation of the two kernels'
arithmetic with injectable defects, and a per-element criterion.  The harness is matrix_common's; the form is tblock_matrix.py's and
norm_matrix.py's (whose plan query and statistics depth this file reads for the forward's partials).

The statistics partials are an INPUT of the kernel.  The GPU file takes them from idb_groupnorm_stats on the device (`stat` = "device":
the forward's own pixel chunks), or builds them on the host in 64-pixel chunks, the layout idb_gemm's gn_partials have (`stat` = "hw64": a
chunk count that differs from the backward's own); the CPU emulation builds them on the host at the forward plan's chunk count.

Criterion.  u = 2^-24, g(k) = k u / (1 - k u), u_T = 2^-11 (f16) or 2^-8 (bf16), sub_T = 2^-25 for f16 (0 for bf16).  Every constant is 1 or
a count of roundings.  No element is excluded; an element whose bound is 0 must be exact.  Per (sample, group), n = hw cpg, S1 = mean|x|,
S2 = mean x^2, d = norm_matrix.gn_depth(the forward's plan), the longest chain of fp32 additions in the statistics:
    E_mean = d u S1 + u |mean|                                        norm_matrix's mean line, and the rounding of the mean to fp32
    r_rstd = (1/2) d u (S2 + 2 |mean| S1) / (var + eps) + 2 u          norm_matrix's rstd line (one-pass variance), relative; the double
                                                                      expression and its rounding to fp32
             (`constant_group`, `silu_special`, `integer`: the sums are exact in fp32 and both d-lines are dropped)
    E_xhat = |xhat| (r_rstd + 2 u) + rstd E_mean                      the subtraction and the product (tblock_matrix's line)
    E_y    = |gamma| E_xhat + 2 u (|xhat gamma| + |y|)                y = xhat gamma + beta
    SiLU'(y) = f = s (1 + y (1 - s)), s = 1 / (1 + exp(-y)):
    r_s    = (6 + |y|) u                                              v_exp_f32 (1 ulp = 2 u) on an argument rounded after the scaling by log2 e
                                                                      (|y| u), 1 + exp (u), v_rcp_f32 (1 ulp = 2 u), one u to spare
    E_f    = (1/2) E_y + |f| (r_s + u) + s [ |y| (s r_s + 2 u (1 - s)) + u |1 + y (1 - s)| ]
                                                                      sup |f'| = 1/2 (at y = 0); then 1 - s, its product with y, 1 + that, and
                                                                      the product with s, each rounded once
    E_d    = |dy| E_f + u |d|       (0 without SiLU)                  d = dy f
    E_g    = |gamma| E_d + u |g|                                      g = d gamma
    k      = ceil(chunk_len / rows per pass) + 8 + ceil(threads / 64) + 6 + 2       the backward's own chain: a thread's pixels, the fold of
                                                                      its 8 channels, the threads per lane, six exchanges; the product
                                                                      g xhat and the rounding of m to fp32 (the chunks merge in double)
    E_m1   = g(k) mean|g| + mean E_g
    E_m2   = g(k) mean|g xhat| + mean(E_g |xhat| + |g| E_xhat)
    E_core = rstd [E_g + E_m1 + |xhat| E_m2 + |m2| E_xhat + 4 u (|g| + |m1| + |xhat m2|)] + |core| (r_rstd + u)      tblock_matrix's line for
                                                                      core = rstd (g - m1 - xhat m2), with E_g for the recomputed g
    dx:  u_T |ref| + sub_T + (1 + u_T) (E_core + u (|core| + |add|))  the fp32 addition of `add`, then the one rounding to T
Recipes: `normal`; `offset` (|mean| / std = 16); `constant_group` (x constant per (sample, group): var is exactly 0, xhat = 0, rstd =
1 / sqrt(eps), dx = rstd (g - m1) + add: eps decides); `one_hot` (one nonzero dy per (sample, group)); `silu_special` (x constant per
group, so y = beta exactly, and beta at 0, +-10, 2.3994 (the extremum of SiLU') and -1.2785 (SiLU's minimum)); `integer` (eps = 3,
x = +-1 alternating by channel so mean = 0, var = 1, var + eps = 4 and rstd = 1/2; gamma = 1, no SiLU, dy = a s + k with s the sign of x and
a, k integers in -2 .. 2 per (sample, group): m1 = k, m2 = a / 2 and dx = 3/8 a s (+ add, an integer in -4 .. 4), exact in T.  Where it is
not 0 the bound is 0: the fp32 chain stays below half a spacing of T (asserted where the bound is built); where it is 0 the fp32 terms
alone remain).

No constant had to be raised for the emulation or for the device; DESIGN 4.19 has the device's figures."""
import ctypes as C
import math
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

import matrix_common as MC
import norm_matrix as NM

F32, F64, U = MC.F32, MC.F64, MC.U
THREADS, MAXCHUNKS = 256, 64
SHAPES = ((64, 0, 32), (320, 0, 32), (640, 0, 32), (1280, 0, 32), (640, 320, 32), (1280, 640, 32), (1280, 1280, 32), (8, 0, 4), (64, 0, 8))
HWS = (1, 7, 64, 100, 1024)
BATCHES = (1, 2, 3)
RECIPES = ("normal", "offset", "constant_group", "one_hot", "silu_special", "integer")
EXACT_SUMS = ("constant_group", "silu_special", "integer")
ADD_MODES = ("add", "none", "alias", "alias_dy")            # alias: dx0 is add; alias_dy: dx0 is dy (both need one source)
SPECIAL_Y = (0.0, 10.0, -10.0, 2.3994, -1.2785)


# ------------------------------------------------------------------------------------------------------------------------------------
# the plan: query and pure-Python statement
# ------------------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Plan:
    sw: int
    slices: int
    chunks: int
    chunk_len: int
    apply_blocks: int


def plan(lib, c0, c1, batch, hw, groups) -> Tuple[int, Plan]:
    o = [C.c_int32(-1) for _ in range(5)]
    rc = lib.idb_groupnorm_bwd_plan(c0, c1, batch, hw, groups, *[C.byref(v) for v in o])
    return rc, Plan(*[v.value for v in o])


def _ceil(a, b):
    return -(-a // b)


def py_plan(c0, c1, batch, hw, groups) -> Plan:
    """The geometry rules of idb_gnbwd.hip, restated: idb_groupnorm's two-launch geometry without its large-tensor rule."""
    c = c0 + c1
    cpg = c // groups
    sw = math.lcm(cpg, 8)
    while sw // 8 < 8 and c % (sw * 2) == 0:
        sw *= 2
    pr, slices = THREADS // (sw // 8), c // sw
    chunks = max(1, min(_ceil(1024, batch * slices), _ceil(hw, 2 * pr), MAXCHUNKS))
    ppb = max(_ceil(hw, _ceil(2048, batch * slices)), 2 * pr)
    return Plan(sw, slices, chunks, _ceil(hw, chunks), _ceil(hw, ppb))


def py_supported(c0, c1, batch, hw, groups) -> bool:
    if min(batch, hw, groups, c0) <= 0 or c1 < 0 or c0 % 8 or c1 % 8 or (c0 + c1) % groups or (c0 + c1) // groups < 2:
        return False
    c, cpg = c0 + c1, (c0 + c1) // groups
    sw = math.lcm(cpg, 8)
    while sw // 8 < 8 and c % (sw * 2) == 0:
        sw *= 2
    return sw // 8 <= THREADS and sw // cpg <= 64 and batch <= 65535 and c // sw <= 65535


def depth(p: Plan) -> int:
    pr = THREADS // (p.sw // 8)
    return _ceil(p.chunk_len, pr) + 8 + _ceil(p.sw // 8 * pr, 64) + 6 + 2


# ------------------------------------------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    recipe: str
    c0: int
    c1: int
    groups: int
    batch: int
    hw: int
    silu: int = 1
    add: str = "add"
    stat: str = "device"

    @property
    def name(self) -> str:
        return f"{self.recipe}_{self.c0}p{self.c1}_g{self.groups}_b{self.batch}_hw{self.hw}_s{self.silu}_{self.add}_{self.stat}"

    @property
    def c(self):
        return self.c0 + self.c1

    @property
    def cpg(self):
        return self.c // self.groups

    @property
    def eps(self) -> float:
        return 3.0 if self.recipe == "integer" else 1e-5

    @property
    def stat_chunks(self) -> Optional[int]:
        return self.hw // 64 if self.stat == "hw64" else None


def _mk(recipe, c0, c1, g, b, hw, silu, add, stat="device") -> Case:
    if c1 and add in ("alias", "alias_dy"):
        add = "add"
    if recipe == "integer":
        silu = 0
    if recipe == "silu_special":
        silu = 1
    return Case(recipe, c0, c1, g, b, hw, silu, add, stat)


TEETH = _mk("normal", 640, 320, 32, 2, 100, 1, "add")                   # three ragged chunks, 120-channel slices that straddle x0 | x1
TEETH_CPG10 = _mk("normal", 320, 0, 32, 2, 100, 1, "alias")             # 8-channel vectors that straddle groups
TEETH_SPECIAL = _mk("silu_special", 640, 320, 32, 2, 100, 1, "add")
TEETH_CONST = _mk("constant_group", 640, 320, 32, 2, 100, 1, "add")


def cases() -> List[Case]:
    """Every (c0, c1, groups) with every hw and every batch on `normal` (9 x 5 x 3 = 135 shapes: the batch decides the pixel chunks and the
    pixel blocks of a shape), the SiLU and the add mode cycling;
    the other recipes on the shapes that tell: a ragged last chunk (640 + 320 at hw 100: chunks of 34, 34, 32 pixels), one pixel, two
    sources with the widest slice (120 channels), cpg 2 (four groups per vector); 64-pixel statistics chunks (16 against the backward's own
    21) at 640 x 1024."""
    cs = [TEETH, TEETH_CPG10, TEETH_SPECIAL, TEETH_CONST]
    for i, (c0, c1, g) in enumerate(SHAPES):
        for j, hw in enumerate(HWS):
            for k, b in enumerate(BATCHES):
                cs.append(_mk("normal", c0, c1, g, b, hw, (i + j + k) % 2, ADD_MODES[(i + 2 * j + k) % 4]))
    cs.append(_mk("normal", 640, 0, 32, 2, 1024, 1, "add", "hw64"))
    cs.append(_mk("normal", 64, 0, 32, 3, 64, 0, "alias_dy", "hw64"))
    for r, recipe in enumerate(RECIPES[1:]):
        cs += [_mk(recipe, 640, 320, 32, 2, 100, 1, "add"), _mk(recipe, 320, 0, 32, 3, 1, r % 2, "none"),
               _mk(recipe, 1280, 640, 32, 1, 64, 1, "add"), _mk(recipe, 64, 0, 32, 2, 7, 1, "alias"), _mk(recipe, 8, 0, 4, 2, 7, r % 2, "alias_dy"),
               _mk(recipe, 320, 0, 32, 1, 1024, 1, "add")]
    return list(dict.fromkeys(cs))


# ------------------------------------------------------------------------------------------------------------------------------------
# inputs and the float64 reference
# ------------------------------------------------------------------------------------------------------------------------------------
def inputs(case: Case, dt: str, seed: int = 81) -> Dict[str, Optional[np.ndarray]]:
    """x, dy, add [batch][hw][c] as float64 holding T values (add None in mode `none`), gamma, beta as float64 holding fp32 values."""
    rng = np.random.default_rng(seed + 7 * case.batch + 13 * case.hw + case.c + 100000 * case.c1)
    b, hw, c, cpg, G = case.batch, case.hw, case.c, case.cpg, case.groups
    rt = lambda v: MC.round_T(np.asarray(v, F32), dt).astype(F64)       # noqa: E731
    shape = (b, hw, c)
    gamma = (1.0 + 0.2 * rng.standard_normal(c)).astype(F32).astype(F64)
    beta = (0.3 * rng.standard_normal(c)).astype(F32).astype(F64)
    x, dy, add = rt(rng.standard_normal(shape) * 2 + 0.5), rt(rng.standard_normal(shape)), rt(rng.standard_normal(shape))
    grp = np.arange(c) // cpg
    const = ((grp[None, None, :] * 5 + np.arange(b)[:, None, None] * 3) % 13 - 6).astype(F64) / 2
    if case.recipe == "offset":
        x = rt(16.0 + rng.standard_normal(shape))
    elif case.recipe == "constant_group":
        x = np.broadcast_to(const, shape).copy()
    elif case.recipe == "one_hot":
        dy = np.zeros((b, hw, G, cpg))
        pick = rng.integers(0, hw * cpg, (b, G))
        dy[np.arange(b)[:, None], pick // cpg, np.arange(G)[None, :], pick % cpg] = 1.0
        dy = dy.reshape(shape)
    elif case.recipe == "silu_special":
        x = np.broadcast_to(const, shape).copy()
        beta = np.resize(np.array(SPECIAL_Y), c).astype(F32).astype(F64)
    elif case.recipe == "integer":
        s = np.where(np.arange(c) % 2 == 0, 1.0, -1.0)
        a = np.repeat(rng.integers(-2, 3, (b, 1, G)).astype(F64), cpg, axis=2)
        k = np.repeat(rng.integers(-2, 3, (b, 1, G)).astype(F64), cpg, axis=2)
        x, gamma, beta = np.broadcast_to(s, shape).copy(), np.ones(c), np.zeros(c)
        dy = np.broadcast_to(a * s + k, shape).copy()
        add = rng.integers(-4, 5, shape).astype(F64)
    return dict(x=x, dy=dy, add=None if case.add == "none" else add, gamma=gamma, beta=beta)


def host_partials(x: np.ndarray, groups: int, chunks: int) -> np.ndarray:
    """{sum, sum of squares} per (sample, pixel chunk, group) in chunks of ceil(hw / chunks) pixels: float64 sums rounded to fp32."""
    b, hw, c = x.shape
    cl = _ceil(hw, chunks)
    xp = np.zeros((b, chunks * cl, c))
    xp[:, :hw] = x
    xg = xp.reshape(b, chunks, cl, groups, c // groups)
    return np.stack([xg.sum(axis=(2, 4)), (xg * xg).sum(axis=(2, 4))], -1).astype(F32)


def eps32(eps: float) -> float:
    return float(F32(eps))


def _sig(y):
    return 1.0 / (1.0 + np.exp(-y))


def reference(case: Case, inp) -> Dict[str, np.ndarray]:
    b, hw, c, G, cpg = case.batch, case.hw, case.c, case.groups, case.cpg
    x, dy, add, gamma, beta = (inp[k] for k in ("x", "dy", "add", "gamma", "beta"))
    grp = lambda v: v.reshape(b, hw, G, cpg)                                      # noqa: E731
    gmean = lambda v: np.broadcast_to(grp(v).mean(axis=(1, 3), keepdims=True), (b, hw, G, cpg)).reshape(b, hw, c)      # noqa: E731
    mean = gmean(x)
    var = gmean((x - mean) ** 2)
    rstd = 1.0 / np.sqrt(var + eps32(case.eps))
    xhat = (x - mean) * rstd
    y = xhat * gamma + beta
    s = _sig(y)
    f = s * (1.0 + y * (1.0 - s)) if case.silu else np.ones_like(y)
    d = dy * f
    g = d * gamma
    m1, m2 = gmean(g), gmean(g * xhat)
    core = rstd * (g - m1 - xhat * m2)
    return dict(mean=mean, var=var, rstd=rstd, xhat=xhat, y=y, s=s, f=f, d=d, g=g, m1=m1, m2=m2, core=core, dx=core + (0.0 if add is None else add),
                s1=gmean(np.abs(x)), s2=gmean(x * x), gmean=gmean)


def bound(case: Case, ref, inp, dt: str, stat_depth: int, own: Plan) -> np.ndarray:
    """The criterion of the module docstring.  stat_depth: norm_matrix.gn_depth of the forward's plan; own: the backward's plan."""
    g_ = MC.gamma
    x, dy, add, gamma = inp["x"], inp["dy"], inp["add"], np.abs(inp["gamma"])
    mean, var, rstd, xhat, y, s, f, d, g, m1, m2, core = (ref[k] for k in ("mean", "var", "rstd", "xhat", "y", "s", "f", "d", "g", "m1", "m2", "core"))
    gm = ref["gmean"]
    eps = eps32(case.eps)
    ds = 0 if case.recipe in EXACT_SUMS else stat_depth
    e_mean = ds * U * ref["s1"] + U * np.abs(mean)
    r_rstd = 0.5 * ds * U * (ref["s2"] + 2 * np.abs(mean) * ref["s1"]) / (var + eps) + 2 * U
    e_xhat = np.abs(xhat) * (r_rstd + 2 * U) + rstd * e_mean
    if case.silu:
        e_y = gamma * e_xhat + 2 * U * (np.abs(xhat * gamma) + np.abs(y))
        r_s = (6 + np.abs(y)) * U
        e_f = 0.5 * e_y + np.abs(f) * (r_s + U) + s * (np.abs(y) * (s * r_s + 2 * U * (1 - s)) + U * np.abs(1 + y * (1 - s)))
        e_d = np.abs(dy) * e_f + U * np.abs(d)
    else:
        e_d = 0.0
    e_g = gamma * e_d + U * np.abs(g)
    k = depth(own)
    e_m1 = g_(k) * gm(np.abs(g)) + gm(e_g)
    e_m2 = g_(k) * gm(np.abs(g * xhat)) + gm(e_g * np.abs(xhat) + np.abs(g) * e_xhat)
    e_core = rstd * (e_g + e_m1 + np.abs(xhat) * e_m2 + np.abs(m2) * e_xhat + 4 * U * (np.abs(g) + np.abs(m1) + np.abs(xhat * m2))) \
        + np.abs(core) * (r_rstd + U)
    f32_terms = e_core + U * (np.abs(core) + (0.0 if add is None else np.abs(add)))
    if case.recipe == "integer":
        nz = ref["dx"] != 0
        assert (f32_terms[nz] < 0.5 * MC.U_T[dt] * np.abs(ref["dx"][nz])).all()
        return np.where(nz, 0.0, f32_terms)
    return MC.U_T[dt] * np.abs(ref["dx"]) + MC.SUB_T[dt] + (1 + MC.U_T[dt]) * f32_terms


# ------------------------------------------------------------------------------------------------------------------------------------
# the emulation of the two kernels, with injectable defects
# ------------------------------------------------------------------------------------------------------------------------------------
DEFECTS = ("no_add", "silu_grad_is_sigmoid", "no_beta", "no_m2", "count_hw", "count_full_chunks", "last_chunk_dropped", "stale_partial",
           "group_off_by_one", "neighbour_gamma", "x1_stride", "dx1_at_dx0_offset", "no_eps")
# the case each defect must fail, in both dtypes
DEFECT_CASE = {"no_add": TEETH, "silu_grad_is_sigmoid": TEETH_SPECIAL, "no_beta": TEETH_SPECIAL, "no_m2": TEETH, "count_hw": TEETH,
               "count_full_chunks": TEETH, "last_chunk_dropped": TEETH, "stale_partial": TEETH, "group_off_by_one": TEETH_CPG10,
               "neighbour_gamma": TEETH, "x1_stride": TEETH, "dx1_at_dx0_offset": TEETH, "no_eps": TEETH_CONST}
_LANES = np.arange(64)


def _butterfly(v: np.ndarray, stages) -> np.ndarray:
    """__shfl_xor tree over the last axis in fp32."""
    for o in stages:
        v = (v + v[..., np.arange(v.shape[-1]) ^ o]).astype(F32)
    return v


def emulate_forward_stats(partial: np.ndarray, hw: int, cpg: int, eps: float, no_eps: bool = False) -> Tuple[np.ndarray, np.ndarray]:
    """gn_apply_kernel's expressions: lane sub of 8 sums the chunks sub, sub + 8, ... in fp32, a three-stage exchange, then mean, variance
    and rstd in double, stored as fp32.  partial fp32 [batch][chunks][groups][2] -> (mean, rstd) fp32 [batch][groups]."""
    b, n, G, _ = partial.shape
    pp = np.zeros((b, 64, G, 2), F32)
    pp[:, :n] = partial
    pp = pp.reshape(b, 8, 8, G, 2)                       # [u][sub]
    acc = np.zeros((b, 8, G, 2), F32)
    for u in range(8):
        acc = (acc + pp[:, u]).astype(F32)
    tot = _butterfly(np.moveaxis(acc, 1, -1), (1, 2, 4))[..., 0].astype(F64)       # [b][G][2]
    cnt = float(hw) * cpg
    mean = tot[..., 0] / cnt
    var = np.maximum(tot[..., 1] / cnt - mean * mean, 0.0)
    with np.errstate(divide="ignore"):
        rstd = 1.0 / np.sqrt(var + (0.0 if no_eps else eps32(eps)))
    return mean.astype(F32), rstd.astype(F32)


def _elementwise(case: Case, inp, mean, rstd, sw: int, defect):
    """xhat and g per element in fp32 (products and sums rounded separately; a contracted FMA on the device differs by less than the
    criterion's roundings)."""
    b, hw, c, cpg, G = case.batch, case.hw, case.c, case.cpg, case.groups
    x = inp["x"].astype(F32)
    if defect == "x1_stride" and case.c1:
        flat = x[..., case.c0:].reshape(-1)
        idx = (np.arange(b * hw)[:, None] * case.c0 + np.arange(case.c1)[None, :]) % flat.size
        x = np.concatenate([x[..., :case.c0], flat[idx].reshape(b, hw, case.c1)], -1)
    gm, bt = inp["gamma"].astype(F32), inp["beta"].astype(F32)
    if defect == "neighbour_gamma":
        gm, bt = np.roll(gm, -sw), np.roll(bt, -sw)
    ex = lambda v: np.repeat(v, cpg, axis=1)[:, None, :]                 # noqa: E731  [b][G] -> [b][1][c]
    xh = ((x - ex(mean)).astype(F32) * ex(rstd)).astype(F32)
    d = inp["dy"].astype(F32)
    if case.silu:
        y = (xh * gm).astype(F32)
        if defect != "no_beta":
            y = (y + bt).astype(F32)
        with np.errstate(over="ignore"):
            s = (F32(1.0) / (F32(1.0) + np.exp(-y).astype(F32)).astype(F32)).astype(F32)
        f = s if defect == "silu_grad_is_sigmoid" else (s * (F32(1.0) + (y * (F32(1.0) - s)).astype(F32)).astype(F32)).astype(F32)
        d = (d * f).astype(F32)
    return xh, (d * gm).astype(F32), ex(rstd)


def _chunk_sums(vals: np.ndarray, case: Case, p: Plan, defect) -> np.ndarray:
    """gnb_sums_kernel's order for one of the two sums: vals fp32 [batch][hw][c] -> fp32 [batch][chunks][groups].  A thread (row, column)
    adds the pixels row, row + PR, ... of its chunk per channel; folds its 8 channels into the groups they belong to, in channel order; per
    group, lane l of 64 adds the threads l, l + 64, ... and a six-stage exchange follows.  Pixels past the chunk and threads whose vector does
    not touch the group add an exact 0."""
    b, hw, c, cpg, G = case.batch, case.hw, case.c, case.cpg, case.groups
    cols = p.sw // 8
    pr = THREADS // cols
    n, cl = p.chunks, p.chunk_len
    kk = _ceil(cl, pr)
    buf = np.zeros((b, n * cl, c), F32)
    buf[:, :hw] = vals[:, :min(hw, n * cl)]
    buf = buf.reshape(b, n, cl, c)
    pad = np.zeros((b, n, kk * pr, c), F32)
    pad[:, :, :cl] = buf
    pad = pad.reshape(b, n, kk, pr, c)
    thr = np.zeros((b, n, pr, c), F32)
    for k in range(kk):
        thr = (thr + pad[:, :, k]).astype(F32)
    ch = np.arange(c)
    vec, grp_of = ch // 8, ch // cpg
    if defect == "group_off_by_one":
        straddles = (vec * 8) // cpg != (vec * 8 + 7) // cpg
        grp_of = np.where(straddles, np.minimum((ch + 1) // cpg, (vec * 8) // cpg + 3), grp_of)
    gps = p.sw // cpg
    nact = cols * pr
    m64 = _ceil(nact, 64)
    out = np.zeros((b, n, G), F32)
    for ga in range(G):
        sl = ga // gps
        mine = np.flatnonzero((grp_of == ga) & (ch // p.sw == sl))
        w = np.zeros((b, n, pr, cols), F32)
        for v in np.unique(vec[mine]):
            acc = np.zeros((b, n, pr), F32)
            for e in mine[vec[mine] == v]:
                acc = (acc + thr[..., e]).astype(F32)
            w[..., v - sl * cols] = acc
        lanes = np.zeros((b, n, m64 * 64), F32)
        lanes[..., :nact] = w.reshape(b, n, nact)
        lanes = lanes.reshape(b, n, m64, 64)
        acc = np.zeros((b, n, 64), F32)
        for i in range(m64):
            acc = (acc + lanes[:, :, i]).astype(F32)
        out[..., ga] = _butterfly(acc, (32, 16, 8, 4, 2, 1))[..., 0]
    return out


def emulate_sums(case: Case, inp, stat: np.ndarray, p: Plan, defect=None) -> Tuple[np.ndarray, np.ndarray]:
    mean, rstd = emulate_forward_stats(stat, case.hw, case.cpg, case.eps, defect == "no_eps")
    with np.errstate(invalid="ignore", over="ignore"):
        xh, g, _ = _elementwise(case, inp, mean, rstd, p.sw, defect)
        return _chunk_sums(g, case, p, defect), _chunk_sums((g * xh).astype(F32), case, p, defect)


def emulate(case: Case, inp, stat: np.ndarray, p: Plan, dt: str, defect: Optional[str] = None, stale=None):
    """One idb_groupnorm_bwd call under plan p on the statistics partials `stat`: (dx0 [batch][hw][c0], dx1 [batch][hw][c1] or None) as
    float64 holders of T values; an element a defect leaves unwritten is NaN.  stale: the (sum g, sum g xhat) partials an earlier launch
    left in the workspace (stale_partial)."""
    assert defect is None or defect in DEFECTS
    b, hw, c, cpg, G = case.batch, case.hw, case.c, case.cpg, case.groups
    mean, rstd = emulate_forward_stats(stat, hw, cpg, case.eps, defect == "no_eps")
    with np.errstate(invalid="ignore", over="ignore"):
        xh, g, rs = _elementwise(case, inp, mean, rstd, p.sw, defect)
        s1, s2 = _chunk_sums(g, case, p, defect), _chunk_sums((g * xh).astype(F32), case, p, defect)
        if defect == "stale_partial" and stale is not None and p.chunks > 1:
            s1, s2 = s1.copy(), s2.copy()
            s1[:, 1], s2[:, 1] = stale[0][:, 1], stale[1][:, 1]
        if defect == "last_chunk_dropped" and p.chunks > 1:
            s1, s2 = s1[:, :-1], s2[:, :-1]
        cnt = float(hw) * cpg
        if defect == "count_hw":
            cnt = float(hw)
        if defect == "count_full_chunks":
            cnt = float(p.chunks * p.chunk_len) * cpg
        ex = lambda v: np.repeat(v, cpg, axis=1)[:, None, :]                 # noqa: E731
        m1 = ex((s1.astype(F64).sum(1) / cnt).astype(F32))
        m2 = ex((s2.astype(F64).sum(1) / cnt).astype(F32))
        if defect == "no_m2":
            m2 = np.zeros_like(m2)
        r = (rs * ((g - m1).astype(F32) - (xh * m2).astype(F32)).astype(F32)).astype(F32)
        if inp["add"] is not None and defect != "no_add":
            r = (r + inp["add"].astype(F32)).astype(F32)
        out = MC.round_T(r, dt).astype(F64)
    dx0 = out[..., :case.c0].copy()
    if not case.c1:
        return dx0, None
    dx1 = out[..., case.c0:].copy()
    if defect == "dx1_at_dx0_offset":
        flat = np.full(b * hw * case.c1, np.nan)
        idx = np.arange(b * hw)[:, None] * case.c0 + np.arange(case.c1)[None, :]
        ok = idx < flat.size
        flat[idx[ok]] = dx1.reshape(b * hw, case.c1)[ok]
        dx1 = flat.reshape(b, hw, case.c1)
    return dx0, dx1


def judge(case: Case, ref, bnd, dx0, dx1):
    """matrix_common.check of both outputs against the reference: (ok, worst err / bound)."""
    r0 = MC.check(dx0, ref["dx"][..., :case.c0], bnd[..., :case.c0])
    if dx1 is None:
        return r0[0], r0[1], MC.describe(case.name + " dx0", r0)
    r1 = MC.check(dx1, ref["dx"][..., case.c0:], bnd[..., case.c0:])
    worst = r0 if r0[1] >= r1[1] else r1
    return r0[0] and r1[0], max(r0[1], r1[1]), MC.describe(case.name + (" dx0" if worst is r0 else " dx1"), worst)


# ------------------------------------------------------------------------------------------------------------------------------------
# the device side (GPU file)
# ------------------------------------------------------------------------------------------------------------------------------------
def forward_plan(lib, case: Case) -> NM.Plan:
    rc, p = NM.plan(lib, case.c0, case.c1, case.batch, case.hw, case.groups)
    assert rc == 0
    return p


def run(lib, case: Case, inp, dt: str):
    """idb_groupnorm_bwd on guarded buffers: (return code, dx0 Guarded, dx1 Guarded or None, the stat partials as the kernel read them
    (fp32 [batch][chunks][groups][2]), the workspace Guarded).  Every input that is not an output is checked to be unchanged."""
    b, hw, c0, c1, G = case.batch, case.hw, case.c0, case.c1, case.groups
    bits = lambda a: MC.to_bits(np.asarray(a, F32), dt)                 # noqa: E731
    xb = bits(inp["x"])
    x0 = MC.dev(np.ascontiguousarray(xb[..., :c0]))
    x1 = MC.dev(np.ascontiguousarray(xb[..., c0:])) if c1 else None
    gm, bt = MC.dev(inp["gamma"], F32), MC.dev(inp["beta"], F32)
    if case.stat == "device":
        part = torch.full((b * MAXCHUNKS * G * 2,), float("nan"), dtype=torch.float32, device=MC.DEV)
        chunks = C.c_int32()
        rc = lib.idb_groupnorm_stats(x0.data_ptr(), c0, MC.ptr(x1), c1, b, hw, G, part.data_ptr(), part.numel() * 4, C.byref(chunks), MC.IDB[dt], MC.stream())
        assert rc == 0, lib.idb_last_error()
        sc = chunks.value
    else:
        sc = case.stat_chunks
        part = MC.dev(host_partials(inp["x"], G, sc), F32)
    n0, n1 = b * hw * c0, b * hw * c1
    dyb = MC.Guarded(n0 + n1, 2, init=bits(inp["dy"]))
    addb = None if inp["add"] is None else MC.Guarded(n0 + n1, 2, init=bits(inp["add"]))
    dx0 = addb if case.add == "alias" else dyb if case.add == "alias_dy" else MC.Guarded(n0, 2)
    dx1 = MC.Guarded(n1, 2) if c1 else None
    need = lib.idb_groupnorm_bwd_workspace_bytes(b, hw, G)
    assert need == b * MAXCHUNKS * G * 8
    ws = MC.Guarded(need // 4, 4)
    rc = lib.idb_groupnorm_bwd(x0.data_ptr(), c0, MC.ptr(x1), c1, part.data_ptr(), sc, dyb.ptr, None if addb is None else addb.ptr, gm.data_ptr(),
                               bt.data_ptr(), case.eps, case.silu, dx0.ptr, None if dx1 is None else dx1.ptr, b, hw, G, MC.IDB[dt], ws.ptr, need,
                               MC.stream())
    torch.cuda.synchronize()
    if dyb is not dx0:
        MC.same_bits(f"{case.name}: dy is an input", dyb.raw("dy"), bits(inp["dy"]).reshape(-1))
    if addb is not None and addb is not dx0:
        MC.same_bits(f"{case.name}: add is an input", addb.raw("add"), bits(inp["add"]).reshape(-1))
    stat = part.cpu().numpy()[:b * sc * G * 2].reshape(b, sc, G, 2)
    return rc, dx0, dx1, stat, ws
