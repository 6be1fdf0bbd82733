"""The test matrix of the transformer block's training kernels (csrc/idb_tblock.hip: idb_layernorm_bwd, idb_geglu_fwd, idb_geglu_bwd)
and of the AdamW step (csrc/idb_adamw.hip: idb_adamw_clip_step_table), shared by test_tblock_matrix_cpu.py (refusals, emulation, teeth)
and test_tblock_matrix_gpu.py (launch and compare): cases, input recipes, float64 references, a numpy emulation of each kernel's
arithmetic with injectable defects, per-element criteria.  The harness is matrix_common's; the form is attn_bwd_matrix.py's.

Notation.  u = 2^-24 (fp32), g(n) = n u / (1 - n u), u_T = 2^-11 (f16) or 2^-8 (bf16), sub_T = 2^-25 for f16 (0 for bf16).  Every
constant is 1 or a count of roundings, but for the one published approximation error (Abramowitz & Stegun 7.1.26).  No element is
excluded; an element whose bound is 0 must be exact.

idb_layernorm_bwd.  One wave per row: lane l holds the 8-vectors l, l + 64, l + 128 of the row; a row sum is the lane's chain of 8 NCH
additions, six exchange levels, and the division by c: k = 8 NCH + 7 roundings on any term.
    E_mean = g(k) mean|x|                                            the row mean
    E_var  = 2 E_mean mean|d| + E_mean^2 + g(k + 3) var               d = x - mean rounded, squared, summed (biased variance over c)
    r_rstd = E_var / (2 (var + eps)) + 3 u                            the division and + eps (two roundings, halved by the root), rsqrtf (1 ulp)
    E_xhat = |xhat| (r_rstd + 2 u) + rstd E_mean                      the subtraction and the product
    E_mg   = g(k + 1) mean|g|                                         g = dy gamma rounded once, then the row mean
    E_mgx  = g(k + 2) mean|g xhat| + mean(|g| E_xhat)
    E_core = rstd [E_mg + |xhat| E_mgx + |mgx| E_xhat + 4 u (|g| + |mg| + |xhat mgx|)] + |core| (r_rstd + u)
             core = rstd (g - mg - xhat mgx): the product g, the product xhat mgx, two subtractions (4 roundings of terms bounded by the
             three magnitudes), the product with rstd
    dx:  u_T |ref| + sub_T + (1 + u_T) (E_core + u (|core| + |add|))  the fp32 addition of `add`, then the one rounding to T
Structured recipes: `const_row` (x constant: mean is exact, xhat = 0 exactly, rstd = 1 / sqrt(eps), dx = rstd (g - mean g));
`one_hot` (one nonzero dy per row); `integer` (eps = 3, x = +-1 alternating so mean = 0, var = 1, var + eps = 4 and rstd = 1/2;
g = a s + q + k with s the sign of x, q = (b, b, -b, -b) per quad, a and k per row, b per quad integers in -2 .. 2: mean g = k, mean(g xhat) = a / 2
and dx = 3/8 a s + q / 2 (+ add) is a multiple of 1/8 below 8, exact in T.  Where it is not 0 the bound is 0: a one-ulp rsqrtf and the fp32
chain stay below half a spacing of T (asserted where the bound is built), so the rounding returns the exact value; where it is 0 the fp32 terms alone remain).

idb_geglu_fwd / idb_geglu_bwd.  Phi' = the device's cumulative normal (A&S 7.1.26 in fp32), z = |gate| / sqrt 2.
    E_cdf = 7.5e-8 + u (1 + (8 + z^2) erfc(z))      the published error of the erf approximation, halved (Phi = 1/2 (1 + erf)); the fp32
                                                    chain on erfc': z, 1 + p z, rcp (1 ulp), five FMAs, the product with t and with the
                                                    exponential (16 roundings, halved), __expf's argument error z^2 u; the final 1 - x/2
    E_pdf = u (3 + z^2) phi(gate)                   the same exponential, one product
    out    = value gate Phi:        u_T |ref| + sub_T + (1 + u_T) (|value gate| E_cdf + 2 u |ref|)
    dvalue = dout gate Phi:         the same with dout for value
    dgate  = dout value (Phi + gate phi):   u_T |ref| + sub_T + (1 + u_T) |dout value| (E_cdf + |gate| E_pdf + 3 u (Phi + |gate| phi))
sub_T applies where the reference is not 0: a product with an exact 0 factor is 0 on the device (`one_hot`: one nonzero dout per row).
`special` puts the gates at 0, +-10 (the tails: gelu' -> 0 and 1), at the minimum of GELU (-0.7518), and at +-1, +-3.

idb_adamw_clip_step_table.  The oracle is torch.optim.AdamW + clip_grad_norm_ on float64 CPU copies of the same fp32 states, stepped once
from identical states.  The device evaluates the same expressions in double and rounds each state once: w, m, v within ONE fp32 ulp of the
float64 result rounded to fp32 (the two double evaluations differ by a few 2^-53, which moves the rounded value by at most one ulp and
only next to a tie).  total_norm: a double sum of N squares in another order and a root: |norm| (N + 8) 2^-53.  A non-finite gradient:
every state bit-unchanged and skipped = 1."""
import math
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

import matrix_common as MC

F32, F64, U = MC.F32, MC.F64, MC.U
LN_C = (8, 64, 72, 320, 640, 1280, 1536)        # 640: the two-vector-per-lane instance (512 < c <= 1024), which the others leave out
LN_ROWS = (1, 3, 5, 70)
LN_RECIPES = ("normal", "offset", "const_row", "one_hot", "integer")
GEGLU_INNER = (8, 256, 1280, 5120)
GEGLU_ROWS = (1, 3, 70)
GEGLU_RECIPES = ("normal", "special", "one_hot")
GEGLU_BLOCK = 256                       # 8-vectors per workgroup


# ------------------------------------------------------------------------------------------------------------------------------------
# idb_layernorm_bwd
# ------------------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class LnCase:
    rows: int
    c: int
    recipe: str
    add: str = "add"                 # "none", "add" (a buffer of its own), "alias" (dx is add)

    @property
    def name(self) -> str:
        return f"ln_{self.recipe}_r{self.rows}_c{self.c}_{self.add}"

    @property
    def eps(self) -> float:
        return 3.0 if self.recipe == "integer" else 1e-5

    @property
    def nch(self) -> int:
        return (self.c // 8 + 63) // 64


def ln_cases() -> List[LnCase]:
    """Every c with every row count on `normal` (the add mode cycling); every recipe on the shapes that tell: c = 72 (a ragged last lane
    group), 8 (below one wave of vectors), 1536 (the maximum), rows 5 (a partial workgroup after a full one)."""
    modes = ("add", "none", "alias")
    cs = [LnCase(r, c, "normal", modes[(i + j) % 3]) for i, c in enumerate(LN_C) for j, r in enumerate(LN_ROWS)]
    for recipe in LN_RECIPES[1:]:
        cs += [LnCase(5, 72, recipe, "add"), LnCase(3, 8, recipe, "none"), LnCase(5, 1536, recipe, "alias"), LnCase(70, 320, recipe, "add")]
    return cs


def ln_inputs(case: LnCase, dt: str, seed: int = 71):
    """(x, dy, add or None, gamma): float64 arrays holding T values (gamma: fp32 values)."""
    rng = np.random.default_rng(seed + 1000 * case.rows + case.c)
    r, c = case.rows, case.c
    rt = lambda v: MC.round_T(v.astype(F32), dt).astype(F64)       # noqa: E731
    gamma = (1.0 + 0.5 * rng.standard_normal(c)).astype(F32).astype(F64)
    x, dy, add = rt(rng.standard_normal((r, c))), rt(rng.standard_normal((r, c))), rt(rng.standard_normal((r, c)))
    if case.recipe == "offset":
        x = rt(16.0 + rng.standard_normal((r, c)))
    elif case.recipe == "const_row":
        x = np.broadcast_to(rng.integers(-3, 4, (r, 1)).astype(F64) + 0.5, (r, c)).copy()
    elif case.recipe == "one_hot":
        dy = np.zeros((r, c))
        dy[np.arange(r), rng.integers(0, c, r)] = 1.0
    elif case.recipe == "integer":
        s = np.where(np.arange(c) % 2 == 0, 1.0, -1.0)
        a, k = rng.integers(-2, 3, (r, 1)).astype(F64), rng.integers(-2, 3, (r, 1)).astype(F64)
        b = np.repeat(rng.integers(-2, 3, (r, c // 4)).astype(F64), 4, axis=1) * np.tile([1.0, 1.0, -1.0, -1.0], c // 4)
        x, gamma = np.broadcast_to(s, (r, c)).copy(), np.ones(c)
        dy, add = a * s + b + k, rng.integers(-4, 5, (r, c)).astype(F64)
    return x, dy, (None if case.add == "none" else add), gamma


def ln_reference(case: LnCase, x, dy, add, gamma) -> Dict[str, np.ndarray]:
    c, eps = case.c, case.eps
    mean = x.mean(-1, keepdims=True)
    d = x - mean
    var = (d * d).mean(-1, keepdims=True)
    rstd = 1.0 / np.sqrt(var + eps)
    xhat, g = d * rstd, dy * gamma
    mg, mgx = g.mean(-1, keepdims=True), (g * xhat).mean(-1, keepdims=True)
    core = rstd * (g - mg - xhat * mgx)
    return dict(mean=mean, d=d, var=var, rstd=rstd, xhat=xhat, g=g, mg=mg, mgx=mgx, core=core, dx=core + (0.0 if add is None else add),
                absx=np.abs(x).mean(-1, keepdims=True), absd=np.abs(d).mean(-1, keepdims=True), absg=np.abs(g).mean(-1, keepdims=True),
                absgx=np.abs(g * xhat).mean(-1, keepdims=True), c=c)


def ln_expected(case: LnCase, ref, x, dy, add, gamma) -> np.ndarray:
    return ref["dx"]


def ln_bound(case: LnCase, ref, add, dt: str) -> np.ndarray:
    k = 8 * case.nch + 7
    g_ = MC.gamma
    e_mean = g_(k) * ref["absx"]
    e_var = 2 * e_mean * ref["absd"] + e_mean ** 2 + g_(k + 3) * ref["var"]
    r_rstd = e_var / (2 * (ref["var"] + case.eps)) + 3 * U
    rstd, xhat, g, mg, mgx, core = (ref[n] for n in ("rstd", "xhat", "g", "mg", "mgx", "core"))
    e_xhat = np.abs(xhat) * (r_rstd + 2 * U) + rstd * e_mean
    e_mg = g_(k + 1) * ref["absg"]
    e_mgx = g_(k + 2) * ref["absgx"] + (np.abs(g) * e_xhat).mean(-1, keepdims=True)
    e_core = rstd * (e_mg + np.abs(xhat) * e_mgx + np.abs(mgx) * e_xhat + 4 * U * (np.abs(g) + np.abs(mg) + np.abs(xhat * mgx))) \
        + np.abs(core) * (r_rstd + U)
    f32_terms = e_core + U * (np.abs(core) + (0.0 if add is None else np.abs(add)))
    full = MC.U_T[dt] * np.abs(ref["dx"]) + MC.SUB_T[dt] + (1 + MC.U_T[dt]) * f32_terms
    if case.recipe == "integer":
        assert (f32_terms[ref["dx"] != 0] < 0.5 * MC.U_T[dt] * np.abs(ref["dx"][ref["dx"] != 0])).all()
        return np.where(ref["dx"] != 0, 0.0, f32_terms)
    return full


LN_DEFECTS = ("no_mean_g", "padded_count", "clamped_summed", "gamma_after_means", "var_c_minus_1", "no_add", "skip_partial_workgroup")


def _wave_sum(vals: np.ndarray, nch: int, clamped: bool = False) -> np.ndarray:
    """The kernel's row sum in fp32: vals [rows][c] -> [rows][1].  Lane l adds its vectors l, l + 64, ... element by element, then the six
    xor exchanges.  Lanes past the row add 0; `clamped`: they add the row's last vector (the copy their clamped load returned)."""
    r, c = vals.shape
    ct = c // 8
    v = np.zeros((r, nch * 64, 8), F32)
    v[:, :ct] = vals.astype(F32).reshape(r, ct, 8)
    if clamped:
        v[:, ct:] = v[:, ct - 1:ct]
    v = v.reshape(r, nch, 64, 8)
    acc = np.zeros((r, 64), F32)
    for i in range(nch):
        for e in range(8):
            acc = (acc + v[:, i, :, e]).astype(F32)
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        acc = (acc + acc[:, lanes ^ o]).astype(F32)
    return acc[:, :1]


def ln_emulate(case: LnCase, x, dy, add, gamma, dt: str, defect: Optional[str] = None) -> np.ndarray:
    """fp32 arithmetic in the kernel's order (products and sums rounded separately; a contracted FMA on the device differs by less than
    the criteria's roundings), the result rounded once to T.  An element a defect leaves unwritten is NaN."""
    assert defect is None or defect in LN_DEFECTS
    f = lambda v: np.asarray(v, F32)                                # noqa: E731
    c, nch = case.c, case.nch
    cnt = F32(nch * 512 if defect == "padded_count" else c)
    clamped = defect == "clamped_summed"
    xv, dyv, gm = f(x), f(dy), f(gamma)
    mean = _wave_sum(xv, nch, clamped) / cnt
    d = xv - mean
    var = _wave_sum(d * d, nch, clamped) / (F32(c - 1) if defect == "var_c_minus_1" else cnt)
    rstd = (F32(1.0) / np.sqrt((var + F32(case.eps)).astype(F64))).astype(F32)
    xhat = d * rstd
    g = dyv if defect == "gamma_after_means" else dyv * gm
    mg = _wave_sum(g, nch, clamped) / cnt
    mgx = _wave_sum(g * xhat, nch, clamped) / cnt
    if defect == "no_mean_g":
        mg = np.zeros_like(mg)
    core = rstd * (g - mg - xhat * mgx)
    if defect == "gamma_after_means":
        core = core * gm
    if add is not None and defect != "no_add":
        core = core + f(add)
    out = MC.round_T(core, dt).astype(F64)
    if defect == "skip_partial_workgroup" and case.rows % 4:
        out[case.rows // 4 * 4:] = np.nan
    return out


# ------------------------------------------------------------------------------------------------------------------------------------
# idb_geglu_fwd / idb_geglu_bwd
# ------------------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class GegluCase:
    rows: int
    inner: int
    recipe: str
    pad: int = 0                     # extra elements per row of hg beyond 2 inner

    @property
    def name(self) -> str:
        return f"geglu_{self.recipe}_r{self.rows}_i{self.inner}_p{self.pad}"

    @property
    def ld(self) -> int:
        return 2 * self.inner + self.pad


def geglu_cases() -> List[GegluCase]:
    cs = [GegluCase(r, i, GEGLU_RECIPES[(a + b) % 3], pad=8 * ((a + b) % 2)) for a, i in enumerate(GEGLU_INNER) for b, r in enumerate(GEGLU_ROWS)]
    # every recipe at a total below one workgroup, at a tail after full workgroups, and at an exact multiple
    for recipe in GEGLU_RECIPES:
        cs += [GegluCase(3, 8, recipe), GegluCase(3, 1280, recipe, pad=16), GegluCase(1, 256 * 8, recipe)]
    return list(dict.fromkeys(cs))


SPECIAL_GATES = (0.0, 10.0, -10.0, -0.7518, -3.0, 3.0, -1.0, 1.0)


def geglu_inputs(case: GegluCase, dt: str, seed: int = 72):
    """(value, gate, dout): float64 arrays [rows][inner] holding T values."""
    rng = np.random.default_rng(seed + 1000 * case.rows + case.inner)
    r, n = case.rows, case.inner
    rt = lambda v: MC.round_T(np.asarray(v, F32), dt).astype(F64)       # noqa: E731
    value, gate, dout = rt(rng.standard_normal((r, n))), rt(2.0 * rng.standard_normal((r, n))), rt(rng.standard_normal((r, n)))
    if case.recipe == "special":
        gate = rt(np.broadcast_to(np.resize(np.array(SPECIAL_GATES), n), (r, n)))
    if case.recipe == "one_hot":
        dout = np.zeros((r, n))
        dout[np.arange(r), rng.integers(0, n, r)] = 1.0
    return value, gate, dout


def _phi(gate):
    t = torch.from_numpy(np.ascontiguousarray(gate, F64))
    cdf = 0.5 * torch.erfc(-t / math.sqrt(2.0))
    return cdf.numpy(), np.exp(-0.5 * gate * gate) / math.sqrt(2.0 * math.pi)


def geglu_reference(value, gate, dout) -> Dict[str, np.ndarray]:
    cdf, pdf = _phi(gate)
    return dict(out=value * gate * cdf, dvalue=dout * gate * cdf, dgate=dout * value * (cdf + gate * pdf), cdf=cdf, pdf=pdf)


def geglu_bound(ref, value, gate, dout, dt: str) -> Dict[str, np.ndarray]:
    z2 = 0.5 * gate * gate
    erfc = torch.erfc(torch.from_numpy(np.sqrt(z2))).numpy()
    e_cdf = 7.5e-8 + U * (1 + (8 + z2) * erfc)
    e_pdf = U * (3 + z2) * ref["pdf"]
    ut = MC.U_T[dt]
    b = {}
    for name, lead in (("out", value), ("dvalue", dout)):
        b[name] = ut * np.abs(ref[name]) + MC.SUB_T[dt] * (ref[name] != 0) + (1 + ut) * (np.abs(lead * gate) * e_cdf + 2 * U * np.abs(ref[name]))
    b["dgate"] = ut * np.abs(ref["dgate"]) + MC.SUB_T[dt] * (ref["dgate"] != 0) \
        + (1 + ut) * np.abs(dout * value) * (e_cdf + np.abs(gate) * e_pdf + 3 * U * (ref["cdf"] + np.abs(gate) * ref["pdf"]))
    return b


GEGLU_DEFECTS = ("halves_swapped", "tanh_gelu", "no_gate_pdf", "tail_block_unprocessed")


def _cdf_pdf32(x: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """gelu_erf_f's cumulative normal in fp32, operation by operation (the reciprocal and the exponential correctly rounded where the
    device's are within an ulp), and the density from the same exponential."""
    x = x.astype(F32)
    z = (np.abs(x) * F32(0.70710678118654752)).astype(F32)
    t = (F32(1.0) / (F32(1.0) + F32(0.3275911) * z)).astype(F32)
    poly = np.full_like(t, F32(1.061405429))
    for coef in (-1.453152027, 1.421413741, -0.284496736, 0.254829592):
        poly = MC.fma32(poly, t, np.full_like(t, F32(coef))).reshape(t.shape)
    e = np.exp((-(z * z)).astype(F32)).astype(F32)
    erfc_z = (poly * t).astype(F32) * e
    cdf = np.where(x >= 0, F32(1.0) - F32(0.5) * erfc_z, F32(0.5) * erfc_z).astype(F32)
    return cdf, (F32(0.3989422804014327) * e).astype(F32)


def geglu_emulate(case: GegluCase, value, gate, dout, dt: str, defect: Optional[str] = None) -> Dict[str, np.ndarray]:
    """{out, dvalue, dgate} as float64 holders of T values; an element a defect leaves unwritten is NaN."""
    assert defect is None or defect in GEGLU_DEFECTS
    v, gt, do = (np.asarray(a, F32) for a in (value, gate, dout))
    if defect == "halves_swapped":
        v, gt = gt, v
    cdf, pdf = _cdf_pdf32(gt)
    if defect == "tanh_gelu":        # 0.5 (1 + tanh(sqrt(2 / pi) (x + 0.044715 x^3))) for Phi, and its derivative's density term
        g64 = gt.astype(F64)
        inner_ = math.sqrt(2.0 / math.pi) * (g64 + 0.044715 * g64 ** 3)
        cdf64 = 0.5 * (1.0 + np.tanh(inner_))
        cdf = cdf64.astype(F32)
        pdf = (0.5 * (1.0 - np.tanh(inner_) ** 2) * math.sqrt(2.0 / math.pi) * (1.0 + 3 * 0.044715 * g64 ** 2)).astype(F32)
    gelu = (gt * cdf).astype(F32)
    slope = cdf if defect == "no_gate_pdf" else (cdf + (gt * pdf).astype(F32)).astype(F32)
    res = {"out": MC.round_T(v * gelu, dt).astype(F64), "dvalue": MC.round_T(do * gelu, dt).astype(F64),
           "dgate": MC.round_T(((do * v).astype(F32) * slope).astype(F32), dt).astype(F64)}
    if defect == "tail_block_unprocessed":
        vpr = case.inner // 8
        done = case.rows * vpr // GEGLU_BLOCK * GEGLU_BLOCK * 8
        for k in res:
            flat = res[k].reshape(-1)
            flat[done:] = np.nan
    return res


# ------------------------------------------------------------------------------------------------------------------------------------
# idb_adamw_clip_step_table
# ------------------------------------------------------------------------------------------------------------------------------------
ADAMW_NUMEL = (1, 4, 255, 4097, 320 * 4)


@dataclass(frozen=True)
class AdamCase:
    name: str
    tensors: int
    step: int = 1
    lr: float = 1e-2
    beta1: float = 0.9
    beta2: float = 0.999
    eps: float = 1e-8
    wd: float = 1e-2
    max_norm: float = 1.0
    inv_scale: float = 1.0
    grad_scale: float = 1.0          # the gradients' size: small keeps the norm below max_norm (clipping inactive)
    poison: Optional[str] = None     # "inf" / "nan": one gradient element

    @property
    def numel(self) -> Tuple[int, ...]:
        return tuple(ADAMW_NUMEL[i % len(ADAMW_NUMEL)] for i in range(self.tensors))


def adam_cases() -> List[AdamCase]:
    return [
        AdamCase("one_tensor_step1", 1),
        AdamCase("three_step1_clipped", 3),
        AdamCase("three_step2_clipped", 3, step=2),
        AdamCase("sixteen_step1_unclipped", 16, grad_scale=1e-3),
        AdamCase("sixteen_step2_scaled", 16, step=2, inv_scale=1.0 / 65536.0, grad_scale=65536.0),
        AdamCase("sixteen_large_step", 16, step=100000, eps=1e-6),
        AdamCase("three_no_decay", 3, step=2, wd=0.0),
        AdamCase("three_unclipped_scaled", 3, step=2, inv_scale=1.0 / 1024.0, grad_scale=1.0),
        AdamCase("three_inf", 3, step=2, poison="inf"),
        AdamCase("sixteen_nan", 16, step=1, poison="nan"),
    ]


def adam_inputs(case: AdamCase, seed: int = 73):
    """Lists of fp32 arrays (w, g, m, v) per tensor.  Step 1 starts from zero moments, as the optimiser does."""
    rng = np.random.default_rng(seed + case.tensors + 7 * case.step)
    w = [(0.1 * rng.standard_normal(n)).astype(F32) for n in case.numel]
    g = [(case.grad_scale * 0.5 * rng.standard_normal(n)).astype(F32) for n in case.numel]
    if case.step == 1:
        m, v = [np.zeros(n, F32) for n in case.numel], [np.zeros(n, F32) for n in case.numel]
    else:
        m = [(0.01 * rng.standard_normal(n)).astype(F32) for n in case.numel]
        v = [(1e-4 * rng.random(n)).astype(F32) for n in case.numel]
    if case.poison:
        g[-1][g[-1].size // 2] = np.inf if case.poison == "inf" else np.nan
    return w, g, m, v


def adam_oracle(case: AdamCase, w, g, m, v):
    """torch.optim.AdamW + clip_grad_norm_ on float64 copies, one step from the given states: (w, m, v as float64 lists, norm, skipped).
    A non-finite norm skips the step (GradScaler.step): the states come back as they were."""
    params = [torch.nn.Parameter(torch.from_numpy(a.astype(F64))) for a in w]
    for p, a in zip(params, g):
        p.grad = torch.from_numpy(a.astype(F64)) * case.inv_scale                      # GradScaler.unscale_
    opt = torch.optim.AdamW(params, lr=case.lr, betas=(case.beta1, case.beta2), eps=case.eps, weight_decay=case.wd, amsgrad=False, foreach=False)
    for p, mi, vi in zip(params, m, v):
        opt.state[p] = {"step": torch.tensor(float(case.step - 1)), "exp_avg": torch.from_numpy(mi.astype(F64)),
                        "exp_avg_sq": torch.from_numpy(vi.astype(F64))}
    norm = float(torch.nn.utils.clip_grad_norm_(params, case.max_norm))
    if not math.isfinite(norm):
        return [a.astype(F64) for a in w], [a.astype(F64) for a in m], [a.astype(F64) for a in v], norm, True
    opt.step()
    return ([p.detach().numpy() for p in params], [opt.state[p]["exp_avg"].numpy() for p in params],
            [opt.state[p]["exp_avg_sq"].numpy() for p in params], norm, False)


def adam_norm_bound(case: AdamCase, norm: float) -> float:
    return abs(norm) * (sum(case.numel) + 8) * 2.0 ** -53


ADAM_DEFECTS = ("bias_step_minus_1", "coupled_decay", "eps_inside_root", "clip_after_moments", "skip_still_decays")


def adam_emulate(case: AdamCase, w, g, m, v, defect: Optional[str] = None):
    """The step kernel's expressions in float64, each state rounded once to fp32: (w, m, v lists of fp32, norm, skipped)."""
    assert defect is None or defect in ADAM_DEFECTS
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        norm = case.inv_scale * math.sqrt(sum(float((a.astype(F64) ** 2).sum()) for a in g))
        decay = 1.0 - case.lr * case.wd
        if not math.isfinite(norm):
            if defect == "skip_still_decays":
                return [(a.astype(F64) * decay).astype(F32) for a in w], m, v, norm, True
            return w, m, v, norm, True
        coef = min(1.0, case.max_norm / (norm + 1e-6))
        step = case.step - 1 if defect == "bias_step_minus_1" else case.step
        bc1, bc2 = F64(1.0 - case.beta1 ** step), F64(1.0 - case.beta2 ** step)          # numpy scalars: a zero divides to inf, as on the device
        wo, mo, vo = [], [], []
        for wi, gi, mi, vi in zip(w, g, m, v):
            wi, mi, vi = wi.astype(F64), mi.astype(F64), vi.astype(F64)
            gh = case.inv_scale * gi.astype(F64) * (1.0 if defect == "clip_after_moments" else coef)
            if defect == "coupled_decay":
                gh, dec = gh + case.wd * wi, 1.0
            else:
                dec = decay
            mn = case.beta1 * mi + (1 - case.beta1) * gh
            vn = case.beta2 * vi + (1 - case.beta2) * gh * gh
            denom = np.sqrt(vn / bc2 + case.eps) if defect == "eps_inside_root" else np.sqrt(vn) / math.sqrt(bc2) + case.eps
            upd = (case.lr / bc1) * mn / denom * (coef if defect == "clip_after_moments" else 1.0)
            wo.append((wi * dec - upd).astype(F32)), mo.append(mn.astype(F32)), vo.append(vn.astype(F32))
    return wo, mo, vo, norm, False


def adam_verdict(what: str, got: List[np.ndarray], want64: List[np.ndarray]) -> Tuple[bool, float, str]:
    """Every tensor within one fp32 ulp of the float64 result rounded to fp32: (ok, worst err / ulp, where)."""
    worst, where, ok = 0.0, "", True
    for i, (a, b) in enumerate(zip(got, want64)):
        want = b.astype(F32).astype(F64)
        res = MC.check(a.astype(F64), want, MC.ulp32(want))
        ok &= res[0]
        if res[1] >= worst:
            worst, where = res[1], f"{what}[{i}]{res[2]}"
    return ok, worst, where


# ------------------------------------------------------------------------------------------------------------------------------------
# the device side (GPU file)
# ------------------------------------------------------------------------------------------------------------------------------------
def ln_run(lib, case: LnCase, x, dy, add, gamma, dt: str):
    """idb_layernorm_bwd on guarded buffers: (return code, the dx Guarded).  `alias`: dx is the add buffer itself."""
    bits = lambda a: MC.to_bits(np.asarray(a, F32), dt)                 # noqa: E731
    n = case.rows * case.c
    xb, dyb = MC.dev(bits(x)), MC.dev(bits(dy))
    gm = MC.dev(gamma, F32)
    addb = None if add is None else MC.Guarded(n, 2, init=bits(add))
    dx = addb if case.add == "alias" else MC.Guarded(n, 2)
    rc = lib.idb_layernorm_bwd(xb.data_ptr(), dyb.data_ptr(), None if addb is None else addb.ptr, gm.data_ptr(), dx.ptr, case.rows, case.c, case.eps,
                               MC.IDB[dt], MC.stream())
    torch.cuda.synchronize()
    if addb is not None and addb is not dx:
        MC.same_bits(f"{case.name}: add is an input", addb.raw("add"), bits(add).reshape(-1))
    return rc, dx


def geglu_pack(case: GegluCase, value, gate, dt: str) -> np.ndarray:
    """hg [rows][ld] as 16-bit patterns: value, gate, then NaN padding."""
    hg = np.full((case.rows, case.ld), MC.NAN16, np.uint16)
    hg[:, :case.inner] = MC.to_bits(np.asarray(value, F32), dt)
    hg[:, case.inner:2 * case.inner] = MC.to_bits(np.asarray(gate, F32), dt)
    return hg


def geglu_run(lib, case: GegluCase, value, gate, dout, dt: str):
    """Both kernels on guarded outputs: (rc fwd, rc bwd, out Guarded, dhg Guarded)."""
    hg = MC.dev(geglu_pack(case, value, gate, dt))
    do = MC.dev(MC.to_bits(np.asarray(dout, F32), dt))
    n = case.rows * case.inner
    out, dhg = MC.Guarded(n, 2), MC.Guarded(2 * n, 2)
    rc1 = lib.idb_geglu_fwd(hg.data_ptr(), case.ld, out.ptr, case.rows, case.inner, MC.IDB[dt], MC.stream())
    rc2 = lib.idb_geglu_bwd(hg.data_ptr(), case.ld, do.data_ptr(), dhg.ptr, case.rows, case.inner, MC.IDB[dt], MC.stream())
    torch.cuda.synchronize()
    return rc1, rc2, out, dhg


class AdamDevice:
    """One case's states in guarded fp32 buffers and the device tables."""

    def __init__(self, case: AdamCase, w, g, m, v):
        self.case = case
        self.w, self.m, self.v = ([MC.Guarded(a.size, 4, init=a) for a in lst] for lst in (w, m, v))
        self.g = [MC.dev(a, F32) for a in g]
        table = lambda ptrs: torch.tensor(ptrs, dtype=torch.int64, device=MC.DEV)       # noqa: E731
        self.tables = [table([b.ptr for b in self.w]), table([t.data_ptr() for t in self.g]), table([b.ptr for b in self.m]),
                       table([b.ptr for b in self.v]), table(list(case.numel))]
        self.norm, self.skipped = MC.Guarded(1, 8), MC.Guarded(1, 4)

    def run(self, lib):
        cs = self.case
        need = lib.idb_adamw_clip_table_workspace_bytes(cs.tensors)
        assert need == 8 * 1024 * cs.tensors
        self.ws = MC.Guarded(need // 8, 8)
        rc = lib.idb_adamw_clip_step_table(cs.tensors, *[t.data_ptr() for t in self.tables], cs.lr, cs.beta1, cs.beta2, cs.eps, cs.wd, cs.max_norm,
                                           cs.inv_scale, cs.step, self.norm.ptr, self.skipped.ptr, self.ws.ptr, need, MC.stream())
        torch.cuda.synchronize()
        return rc

    def results(self):
        self.ws.raw("workspace")
        get = lambda lst, n: [b.f32(n).copy() for b in lst]                # noqa: E731
        return (get(self.w, "w"), get(self.m, "m"), get(self.v, "v"), float(self.norm.f64("total_norm")[0]),
                int(self.skipped.raw("skipped").view(np.int32)[0]))
