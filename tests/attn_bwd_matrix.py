"""The test matrix of the training attention (idb_attention_fwd_train, idb_attention_bwd) and of idb_lora_grad, shared by
test_attn_bwd_matrix_cpu.py (plans, refusals, emulation, teeth) and test_attn_bwd_matrix_gpu.py (launch and compare): cases, input
recipes, float64 references, a plain emulation of the kernels' arithmetic contract with injectable defects, per-element criteria.
The structure is attn_matrix.py's; its reference and bound serve the forward's `out` unchanged.

Block sizes are never constants here: key blocks, the query chunk of form 1 and the launches come from idb_attention_bwd_plan, the
32-row query slice and the lora chunking from the header's constants as _lib mirrors them.

Notation.  u = unit roundoff of the operand dtype T (2^-8 bf16, 2^-11 f16), w = 2^-24 (fp32), sub = 2^-25 for f16 (below 2^-14 f16 is
spaced 2^-24, so a rounding there errs by up to 2^-25 absolutely; 0 for bf16).  s = scale Q K^T, sabs = scale |Q| |K|^T,
P = exp(s - lse), out = P V, delta = rowsum(dout o out), dabs = rowsum(|dout| o |out|), dP = dout V^T, dPabs = |dout| |V|^T,
dS = P o (dP - delta).  The backward is handed out rounded to T and lse rounded to fp32 (what the forward stores); its reference is the
float64 gradient of the UNROUNDED problem, so the rounding of out and lse count as errors (the delta and lse terms).

lse (forward), per row:   |lse - ref| <= w (8 max_j sabs + sqrt(n_kv) + 4 + 3 |lse|)
    the 64-term fp32 score (random-sign growth sqrt(64) = 8 on terms bounded by sabs), the running sum over n_kv terms, exp2 and log
    (2 ulp each), the final fma.

P as the kernels recompute it, relative error   E_P = w (11 (|lse| + sabs) + 3)
    lse rounded to fp32, -lse / scale rounded, the product with scale log2(e) rounded (3 roundings of a quantity bounded by |lse| + sabs),
    the 64-term accumulation on top of the initial accumulator (8), exp2 and the rounded constant (3).

dS as it enters the second products, absolute error
    E_dS = |dS| (u + w + E_P)                       its rounding to T, the fp32 product, P's own error
         + sub                                      f16 subnormal results
         + P [(u + 8 w) dabs + 8 w (|delta| + dPabs)]
                                                    delta from the ROUNDED out (u dabs) summed in fp32 (8 w dabs), and the 64-term dP chain
                                                    on top of -delta

dV = P^T dout:    u |dV| + sub                      the single rounding of the result
                + (u + E_P) o P ^T |dout|           every P_ij rounded to T (relative u) before the product, and its own error
                + n_q sub max|dout|                 f16: P_ij below 2^-14
                + sqrt(n_q) w P^T |dout|            fp32 accumulation over n_q terms (random-sign growth, as the forward's C_A term)
dQ = scale dS K:  u |dQ| + sub + scale E_dS |K| + sqrt(n_kv) w scale |dS| |K|
dK = scale dS^T Q:u |dK| + sub + scale E_dS^T |Q| + sqrt(n_q) w scale |dS|^T |Q|
Every constant not explained by a count of roundings is 1.  No element is excluded; an element whose bound is 0 must be exact.

Structured recipes (the gradients are known exactly, confirmed on the defect-free emulation by the CPU file):
    count     q = 0, small-integer dout: P is uniform.  dK is exactly 0 (bound 0: q = 0 annihilates every term).  With n_kv a power of two
              P = 1 / n_kv is exact in T, so dV = round_T(sum_i dout_i / n_kv) bit for bit: it catches the QUERY-side index defects (extra
              or missing query row, skipped first slice, a chunk's slab left out) that perturb a sum of n_q equal weights, and through dQ
              (every key weighs the same) the KEY-side ones (extra or missing key, skipped last tile).
    one_hot   query i = 64 x its dominant key (attn_matrix's recipe), integer v and dout: P is exactly one-hot, lse = 512 and
              lse / scale = 4096 exactly.  dV is the exact sum of the selecting queries' dout; out = v_j, so delta = dP on the selected
              key and dS, dQ, dK are exactly 0: it catches the rescaling defects (delta omitted, lse off by the scale factor).
    ones_dout n_q = 1 and dout = 1: dV_j = round_T(P_j), ONE rounding, so the separate P term is dropped (criterion u |dV| + E_P |dV|):
              a truncated P errs by up to 2 u and fails.
`normal` catches dK's missing scale; padding rows attended yield NaN or an overflow and fail as non-finite."""
import ctypes as C
import math
from dataclasses import dataclass, replace
from types import SimpleNamespace
from typing import Dict, List, Optional, Tuple

import torch

import attn_matrix as AM
import matrix_common as MC
from faceposegenerator_amd import _lib as L

UNIT, TDT, IDB_DT, rnd, trunc = AM.UNIT, AM.TDT, AM.IDB_DT, AM.rnd, AM.trunc
W32 = 2.0 ** -24
SUB = {"bf16": 0.0, "f16": 2.0 ** -25}
SLICE = L.IDB_ATTN_BWD_SLICE
F64 = torch.float64


# ------------------------------------------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    name: str
    form: int                        # the form this case was chosen for (asserted through idb_attention_bwd_plan)
    batch: int
    heads: int
    n_q: int
    n_kv: int
    recipes: Tuple[str, ...] = ("normal", "count")
    n_kv_alloc: int = 0
    layout: str = "sep"              # "qkv": one packed [q|k|v] buffer for the inputs and another for the gradients; "sep": separate, padded
    pad: int = 0                     # extra elements per row beyond the packed width ("sep": 8 + pad so that every stride differs)
    scale: float = 0.125
    poison: Optional[str] = None     # K/V rows n_kv .. n_kv_alloc-1: "nan" or "max"

    @property
    def alloc(self) -> int:
        return self.n_kv_alloc or self.n_kv

    @property
    def c(self) -> int:
        return self.heads * 64


def plan(lib, batch, heads, n_q, n_kv):
    """(return code, (form, key_block, query_rows, launches)) of idb_attention_bwd_plan."""
    o = [C.c_int32(-1) for _ in range(4)]
    rc = lib.idb_attention_bwd_plan(batch, heads, n_q, n_kv, *[C.byref(x) for x in o])
    return rc, tuple(x.value for x in o)


def case_plan(lib, case: Case):
    rc, p = plan(lib, case.batch, case.heads, case.n_q, case.n_kv)
    assert rc == 0, (case.name, rc)
    return p


def cases(lib) -> List[Case]:
    """The smallest shapes at which each thing can go wrong, sized from the plan query."""
    _, (_, kb, _, _) = plan(lib, 1, 1, 1, 1)
    full = L.IDB_ATTN_BWD_FULL_GRID
    S = SLICE
    cs = [
        # key blocks of the key-owning kernel (and 64-key tiles of the query-owning one): short by one, exactly full, three ragged
        Case("kb_short", 0, 1, 1, S, kb - 1),
        Case("kb_full", 0, 1, 2, S, kb, recipes=("normal", "count", "one_hot")),
        Case("kb_three_ragged", 0, 1, 1, 2 * S, 2 * kb + 37, recipes=("normal", "peaked", "one_hot")),
        # query slices: one, two, three with a ragged last one (form 0 needs at most two slices, or a full grid)
        Case("slice_one", 0, 1, 1, S, 64),
        Case("slice_one_ragged", 0, 2, 1, S - 5, 64, recipes=("normal", "count", "one_hot")),
        Case("slice_two_ragged", 0, 1, 2, 2 * S - 1, 64),
        Case("slice_three_ragged_full_grid", 0, 2, full // 2, 2 * S + 7, 16, recipes=("normal",)),
        # the two degenerate sizes
        Case("one_query", 0, 1, 2, 1, 70, recipes=("normal", "ones_dout")),
        Case("one_query_long", 0, 1, 1, 1, 2 * kb + 1, recipes=("ones_dout",)),
        Case("one_key", 0, 2, 1, 40, 1, recipes=("normal",)),
        # cross-attention: 77 keys in 80 allocated rows, the padding poisoned; many queries -> form 1
        Case("cross77_nan", 1, 2, 2, 3 * S + 3, 77, n_kv_alloc=80, poison="nan", recipes=("normal", "peaked")),
        Case("cross77_max", 1, 1, 5, 2 * S + 1, 77, n_kv_alloc=80, poison="max", recipes=("normal", "one_hot")),
        Case("cross77_form0", 0, 1, 1, 2 * S, 77, n_kv_alloc=80, poison="nan"),
        # form 1: chunks with a ragged last one, more than one key block, and the packed layout
        Case("chunks_ragged", 1, 1, 1, 7 * S + 9, 64, recipes=("normal", "count", "one_hot")),
        Case("chunks_two_key_blocks", 1, 1, 2, 4 * S, kb + 64, recipes=("normal", "count")),
        Case("packed_self", 1, 2, 2, 70, 70, layout="qkv", recipes=("normal", "peaked")),
        Case("packed_self_form0", 0, 1, 5, 2 * S, 2 * S, layout="qkv", recipes=("normal", "count", "one_hot")),
        Case("self_600", 1, 1, 1, 600, 600, layout="qkv", recipes=("normal",)),
        Case("scale_half", 0, 1, 1, 2 * S, 50, scale=0.5, pad=8, recipes=("normal",)),
    ]
    return cs + threshold_cases(lib)


def threshold_cases(lib) -> List[Case]:
    """Both sides of the plan's two thresholds, found with the plan query: the row count at which chunking starts (a small grid) and the
    grid size at which it stops (a row count that chunks on a small grid)."""
    out = []
    rows = next(n for n in range(1, 4096) if plan(lib, 1, 1, n, 16)[1][0] == 1)
    out += [Case(f"rows_{rows - 1}_form0", 0, 1, 1, rows - 1, 16, recipes=("normal",)), Case(f"rows_{rows}_form1", 1, 1, 1, rows, 16, recipes=("normal",))]
    heads = next(h for h in range(1, 4096) if plan(lib, 1, h, rows, 16)[1][0] == 0)
    out += [Case(f"grid_{heads - 1}_form1", 1, 1, heads - 1, rows, 16, recipes=("normal",)), Case(f"grid_{heads}_form0", 0, 1, heads, rows, 16, recipes=("normal",))]
    return out


# ------------------------------------------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------------------------------------------
@dataclass
class Inputs:
    q: torch.Tensor          # [batch][heads][n][64] float64 holding operand-dtype values
    k: torch.Tensor
    v: torch.Tensor
    dout: torch.Tensor
    exact_out: Optional[torch.Tensor] = None       # one_hot: the forward's exactly known output (attn_matrix's `exact`)


def make_inputs(case: Case, recipe: str, dtype: str, seed: int = 61) -> Inputs:
    g = torch.Generator().manual_seed(seed)
    b, h, nq, nk = case.batch, case.heads, case.n_q, case.n_kv
    fwd = {"normal": "normal", "peaked": "peaked", "count": "count", "one_hot": "one_hot", "ones_dout": "normal"}[recipe]
    a = AM.make_inputs(SimpleNamespace(batch=b, heads=h, n_q=nq, n_kv=nk, scale=case.scale, causal=False), fwd, dtype, seed)
    q, k, v = a.q, a.k, a.v
    if recipe == "count":            # the forward recipe's one-hot v would make dP sparse; a dense v exercises dQ
        v = rnd(torch.randn(b, h, nk, 64, generator=g, dtype=torch.float32).double(), dtype)
    if recipe in ("count", "one_hot"):
        dout = torch.randint(-4, 5, (b, h, nq, 64), generator=g).double()
    elif recipe == "ones_dout":
        assert nq == 1
        dout = torch.ones(b, h, nq, 64, dtype=F64)
    else:
        dout = rnd(torch.randn(b, h, nq, 64, generator=g, dtype=torch.float32).double(), dtype)
    return Inputs(q, k, v, dout, a.exact if recipe == "one_hot" else None)


# ------------------------------------------------------------------------------------------------------------------------------------
# float64 reference
# ------------------------------------------------------------------------------------------------------------------------------------
@dataclass
class Ref:
    fwd: AM.Ref              # attn_matrix's reference of `out`
    lse: torch.Tensor        # [b][h][n_q]
    p: torch.Tensor
    sabs: torch.Tensor
    ds: torch.Tensor
    delta: torch.Tensor
    dabs: torch.Tensor
    dpabs: torch.Tensor
    dq: torch.Tensor
    dk: torch.Tensor
    dv: torch.Tensor


def reference(inp: Inputs, case: Case) -> Ref:
    nk, sc = case.n_kv, case.scale
    q, k, v, do = inp.q, inp.k[..., :nk, :], inp.v[..., :nk, :], inp.dout
    s = (q @ k.transpose(-1, -2)) * sc
    lse = torch.logsumexp(s, -1)
    p = torch.exp(s - lse[..., None])
    out = p @ v
    delta = (do * out).sum(-1, keepdim=True)
    dp = do @ v.transpose(-1, -2)
    ds = p * (dp - delta)
    return Ref(AM.reference(q, k, v, nk, sc, False), lse, p, (q.abs() @ k.abs().transpose(-1, -2)) * sc, ds, delta,
               (do.abs() * out.abs()).sum(-1, keepdim=True), do.abs() @ v.abs().transpose(-1, -2),
               sc * (ds @ k), sc * (ds.transpose(-1, -2) @ q), p.transpose(-1, -2) @ do)


def saved(r: Ref, dtype: str) -> Tuple[torch.Tensor, torch.Tensor]:
    """What the backward is handed: out rounded to T, lse rounded to fp32 (float64 holders)."""
    return rnd(r.fwd.ref, dtype), r.lse.float().double()


def forward_criterion(inp: Inputs, r: Ref, n_kv: int, dtype: str) -> Tuple[torch.Tensor, torch.Tensor]:
    """(expected out, bound) by attn_matrix's own criterion: bit-equality with the known output for one_hot (the float64 P V carries
    weights of e^-190 where the kernel's are 0), its full bound otherwise (`count` here has a dense v, not the forward recipe's)."""
    if inp.exact_out is not None:
        return inp.exact_out, AM.bound(r.fwd, n_kv, dtype, "one_hot")
    return r.fwd.ref, AM.bound(r.fwd, n_kv, dtype, "normal")


def lse_bound(r: Ref, n_kv: int) -> torch.Tensor:
    return W32 * (8 * r.sabs.amax(-1) + math.sqrt(n_kv) + 4 + 3 * r.lse.abs())


# ------------------------------------------------------------------------------------------------------------------------------------
# the emulation of the backward's arithmetic contract, with defects
# ------------------------------------------------------------------------------------------------------------------------------------
DEFECTS = ("extra_key", "missing_key", "extra_query", "missing_query", "skip_first_slice", "skip_last_tile", "no_delta", "lse_unscaled",
           "p_trunc", "dk_no_scale", "slab_left_out", "pad_attended")


def emulate(inp: Inputs, out_t, lse32, case: Case, dtype: str, query_rows: int, defect: Optional[str] = None, pad_value: float = math.nan):
    """delta from the rounded out; P = exp(s - lse) in float64; P rounded (to nearest even) to T for dV; dS = P (dP - delta) rounded to T
    for dQ and dK; each gradient rounded once.  Returns (dq, dk, dv); an element a defect leaves unwritten is NaN.  `query_rows` is the
    plan's chunk (slab_left_out drops the last chunk)."""
    assert defect is None or defect in DEFECTS
    nq, nk, sc = case.n_q, case.n_kv, case.scale
    q, k, v, do = inp.q, inp.k[..., :nk, :], inp.v[..., :nk, :], inp.dout
    if defect == "pad_attended":
        padrows = torch.full(k.shape[:-2] + (case.alloc - nk, 64), pad_value, dtype=F64)
        k, v = torch.cat([k, padrows], -2), torch.cat([v, padrows], -2)
    if defect == "extra_key":        # a missed tail mask reads, after the clamp, a copy of key n_kv - 1
        k, v = torch.cat([k, k[..., -1:, :]], -2), torch.cat([v, v[..., -1:, :]], -2)
    if defect == "missing_key":
        k, v = k[..., :-1, :], v[..., :-1, :]
    delta = torch.zeros_like(lse32[..., None]) if defect == "no_delta" else (do * out_t).sum(-1, keepdim=True)
    s = (q @ k.transpose(-1, -2)) * sc
    p = torch.exp(s - (lse32 * sc if defect == "lse_unscaled" else lse32)[..., None])
    ds = rnd(p * (do @ v.transpose(-1, -2) - delta), dtype)
    pr = trunc(p, dtype) if defect == "p_trunc" else rnd(p, dtype)
    # the key-owning side: which query rows enter dK and dV
    rows = torch.ones(nq, dtype=torch.bool)
    if defect == "missing_query":
        rows[-1] = False
    if defect == "skip_first_slice" and nq > SLICE:
        rows[:SLICE] = False
    if defect == "slab_left_out" and nq > query_rows:
        rows[(nq - 1) // query_rows * query_rows:] = False
    qs, dos, dss, prs = q[..., rows, :], do[..., rows, :], ds[..., rows, :], pr[..., rows, :]
    if defect == "extra_query":      # a missed row mask reads a copy of the last query row
        qs, dos, dss, prs = (torch.cat([x, x[..., -1:, :]], -2) for x in (qs, dos, dss, prs))
    dk = rnd((1.0 if defect == "dk_no_scale" else sc) * (dss.transpose(-1, -2) @ qs), dtype)
    dv = rnd(prs.transpose(-1, -2) @ dos, dtype)
    # the query-owning side: which keys enter dQ
    dsq, kq = ds, k
    if defect == "skip_last_tile" and k.shape[-2] > AM_TILE:
        keep = (k.shape[-2] - 1) // AM_TILE * AM_TILE
        dsq, kq = ds[..., :keep], k[..., :keep, :]
    dq = rnd(sc * (dsq @ kq), dtype)
    if defect == "missing_query":
        dq[..., -1, :] = math.nan
    if defect == "missing_key":
        nanrow = torch.full(dk.shape[:-2] + (1, 64), math.nan, dtype=F64)
        dk, dv = torch.cat([dk, nanrow], -2), torch.cat([dv, nanrow], -2)
    return dq, dk[..., :nk, :], dv[..., :nk, :]


AM_TILE = 64                         # keys per tile of the query-owning kernels (only the skip_last_tile defect reads it)


# ------------------------------------------------------------------------------------------------------------------------------------
# criteria
# ------------------------------------------------------------------------------------------------------------------------------------
def _pow2(n: int) -> bool:
    return n & (n - 1) == 0


def expected(inp: Inputs, r: Ref, case: Case, recipe: str, dtype: str) -> Dict[str, torch.Tensor]:
    """The value every element is compared with: the float64 gradient, or its single rounding where the recipe makes it exact."""
    e = {"dq": r.dq, "dk": r.dk, "dv": r.dv}
    if recipe == "count":
        e["dk"] = torch.zeros_like(r.dk)
        if _pow2(case.n_kv):
            e["dv"] = rnd((inp.dout.sum(-2, keepdim=True) / case.n_kv).expand_as(r.dv), dtype)
    if recipe == "one_hot":
        e["dq"], e["dk"] = torch.zeros_like(r.dq), torch.zeros_like(r.dk)
        e["dv"] = rnd((r.p.round().transpose(-1, -2) @ inp.dout), dtype)
    return e


def bound(inp: Inputs, r: Ref, case: Case, recipe: str, dtype: str) -> Dict[str, torch.Tensor]:
    u, sub, nq, nk, sc = UNIT[dtype], SUB[dtype], case.n_q, case.n_kv, case.scale
    k, q, do = inp.k[..., :nk, :].abs(), inp.q.abs(), inp.dout.abs()
    e_p = W32 * (11 * (r.lse.abs()[..., None] + r.sabs) + 3)
    e_ds = r.ds.abs() * (u + W32 + e_p) + sub + r.p * ((u + 8 * W32) * r.dabs + 8 * W32 * (r.delta.abs() + r.dpabs))
    pt = r.p.transpose(-1, -2)
    p_term = (0.0 if recipe == "ones_dout" else u) + e_p
    b = {
        "dq": u * r.dq.abs() + sub + sc * (e_ds @ k) + math.sqrt(nk) * W32 * sc * (r.ds.abs() @ k),
        "dk": u * r.dk.abs() + sub + sc * (e_ds.transpose(-1, -2) @ q) + math.sqrt(nq) * W32 * sc * (r.ds.abs().transpose(-1, -2) @ q),
        "dv": u * r.dv.abs() + sub + (p_term * r.p).transpose(-1, -2) @ do + nq * sub * do.max() + math.sqrt(nq) * W32 * (pt @ do),
    }
    if recipe == "count":
        b["dk"] = torch.zeros_like(r.dk)
        if _pow2(nk):
            b["dv"] = torch.zeros_like(r.dv)
    if recipe == "one_hot":
        b = {n: torch.zeros_like(x) for n, x in b.items()}
    return b


# ------------------------------------------------------------------------------------------------------------------------------------
# the C ABI's layouts (GPU file)
# ------------------------------------------------------------------------------------------------------------------------------------
def _rows(x: torch.Tensor) -> torch.Tensor:
    b, h, n, d = x.shape
    return x.permute(0, 2, 1, 3).reshape(b * n, h * d)


def _unrows(x: torch.Tensor, b: int, h: int) -> torch.Tensor:
    return x.reshape(b, -1, h, 64).permute(0, 2, 1, 3)


class Device:
    """One (case, recipe, dtype) on the device: inputs with NaN in every element the ABI does not hand to a kernel (row padding) and
    the poison in K/V rows n_kv .. n_kv_alloc - 1; outputs NaN-filled between NaN guards (matrix_common.Guarded), so an unwritten
    element fails its criterion and a write outside the ABI's outputs (padding rows of dk / dv included) is seen."""

    def __init__(self, case: Case, inp: Inputs, dtype: str):
        self.case, self.dtype, t = case, dtype, TDT[dtype]
        b, c, nq, nk, na = case.batch, case.c, case.n_q, case.n_kv, case.alloc
        fill = {None: 0.0, "nan": math.nan, "max": torch.finfo(t).max}[case.poison]

        def kv_rows(x):
            full = torch.full((b, na, c), fill, dtype=F64)
            full[:, :nk] = _rows(x).reshape(b, nk, c)
            return full.reshape(b * na, c)

        q, k, v, do = _rows(inp.q), kv_rows(inp.k), kv_rows(inp.v), _rows(inp.dout)
        if case.layout == "qkv":
            assert nq == nk == na
            self.q_ld = self.kv_ld = self.dq_ld = self.dkv_ld = 3 * c + case.pad
            buf = torch.full((b * nq, self.q_ld), math.nan, dtype=t)
            buf[:, :c], buf[:, c:2 * c], buf[:, 2 * c:3 * c] = q.to(t), k.to(t), v.to(t)
            self.qkv = buf.to(MC.DEV)
            p = self.qkv.data_ptr()
            self.q_ptr, self.k_ptr, self.v_ptr = p, p + 2 * c, p + 4 * c
            self.grad = [MC.Guarded(b * nq * self.dq_ld, 2)]
            g = self.grad[0].ptr
            self.dq_ptr, self.dk_ptr, self.dv_ptr = g, g + 2 * c, g + 4 * c
        else:
            self.q_ld, self.kv_ld, self.dq_ld, self.dkv_ld = c + 8 + case.pad, c + 16 + case.pad, c + 24 + case.pad, c + 32 + case.pad

            def padded(x, ld):
                buf = torch.full((x.shape[0], ld), math.nan, dtype=t)
                buf[:, :c] = x.to(t)
                return buf.to(MC.DEV)

            self.qb, self.kb, self.vb = padded(q, self.q_ld), padded(k, self.kv_ld), padded(v, self.kv_ld)
            self.q_ptr, self.k_ptr, self.v_ptr = self.qb.data_ptr(), self.kb.data_ptr(), self.vb.data_ptr()
            self.grad = [MC.Guarded(b * nq * self.dq_ld, 2), MC.Guarded(b * na * self.dkv_ld, 2), MC.Guarded(b * na * self.dkv_ld, 2)]
            self.dq_ptr, self.dk_ptr, self.dv_ptr = (x.ptr for x in self.grad)
        self.out_ld = self.dout_ld = c + 40 + case.pad
        self.dout = torch.full((b * nq, self.dout_ld), math.nan, dtype=t)
        self.dout[:, :c] = do.to(t)
        self.dout = self.dout.to(MC.DEV)
        self.out = MC.Guarded(b * nq * self.out_ld, 2)
        self.lse = MC.Guarded(b * case.heads * nq, 4)

    def forward(self, lib):
        cs = self.case
        return lib.idb_attention_fwd_train(self.q_ptr, self.q_ld, self.k_ptr, self.v_ptr, self.kv_ld, self.out.ptr, self.out_ld, self.lse.ptr,
                                           cs.batch, cs.heads, cs.n_q, cs.n_kv, cs.alloc, cs.scale, IDB_DT[self.dtype], MC.stream())

    def forward_results(self):
        """(out [b][h][n_q][64], lse [b][h][n_q]) as float64; the padding columns of `out` must be untouched."""
        cs = self.case
        vals, bits = self.out.T("out", self.dtype)
        bits = bits.reshape(cs.batch * cs.n_q, self.out_ld)
        assert (bits[:, cs.c:] == MC.NAN16).all(), f"{cs.name}: forward wrote into the row padding of out"
        out = torch.from_numpy(vals.reshape(cs.batch * cs.n_q, self.out_ld)[:, :cs.c].copy()).double()
        return _unrows(out, cs.batch, cs.heads), torch.from_numpy(self.lse.f32("lse").copy()).double().reshape(cs.batch, cs.heads, cs.n_q)

    def backward(self, lib, out_t: torch.Tensor, lse32: torch.Tensor, workspace_bytes: Optional[int] = None):
        """idb_attention_bwd on the given saved tensors (float64 holders of T / fp32 values) into fresh NaN-filled gradients."""
        cs, t = self.case, TDT[self.dtype]
        ob = torch.full((cs.batch * cs.n_q, self.out_ld), math.nan, dtype=t)
        ob[:, :cs.c] = _rows(out_t).to(t)
        self.out_in, self.lse_in = ob.to(MC.DEV), lse32.float().contiguous().to(MC.DEV)
        need = lib.idb_attention_bwd_workspace_bytes(cs.batch, cs.heads, cs.n_q, cs.n_kv)
        assert need > 0 and need % 4 == 0
        self.ws = MC.Guarded(need // 4, 4)
        return lib.idb_attention_bwd(self.q_ptr, self.q_ld, self.k_ptr, self.v_ptr, self.kv_ld, self.out_in.data_ptr(), self.out_ld,
                                     self.dout.data_ptr(), self.dout_ld, self.lse_in.data_ptr(), self.dq_ptr, self.dq_ld, self.dk_ptr, self.dv_ptr,
                                     self.dkv_ld, self.ws.ptr, need if workspace_bytes is None else workspace_bytes, cs.batch, cs.heads, cs.n_q,
                                     cs.n_kv, cs.alloc, cs.scale, IDB_DT[self.dtype], MC.stream())

    def gradients(self):
        """({dq, dk, dv} as [b][h][n][64] float64, the raw 16-bit patterns of every gradient buffer); asserts the guards, the workspace's
        guards, and that every element outside the ABI's outputs (row padding, K/V padding rows) still holds the NaN pre-fill."""
        cs = self.case
        b, c, nq, nk, na = cs.batch, cs.c, cs.n_q, cs.n_kv, cs.alloc
        self.ws.raw("workspace")
        raws = [g.raw("gradient buffer") for g in self.grad]
        vals = [MC.from_bits(x, self.dtype) for x in raws]
        if cs.layout == "qkv":
            m = vals[0].reshape(b * nq, self.dq_ld)
            bits = raws[0].reshape(b * nq, self.dq_ld)
            assert (bits[:, 3 * c:] == MC.NAN16).all(), f"{cs.name}: a gradient's row padding was written"
            parts = [m[:, :c], m[:, c:2 * c], m[:, 2 * c:3 * c]]
        else:
            parts = []
            for i, (x, bts, rows, ld) in enumerate(zip(vals, raws, (b * nq, b * na, b * na), (self.dq_ld, self.dkv_ld, self.dkv_ld))):
                bts = bts.reshape(rows, ld)
                assert (bts[:, c:] == MC.NAN16).all(), f"{cs.name}: a gradient's row padding was written"
                if i > 0:
                    assert (bts.reshape(b, na, ld)[:, nk:] == MC.NAN16).all(), f"{cs.name}: rows n_kv .. n_kv_alloc-1 of dk / dv were written"
                parts.append(x.reshape(rows, ld)[:, :c])
            parts[1] = parts[1].reshape(b, na, c)[:, :nk].reshape(b * nk, c)
            parts[2] = parts[2].reshape(b, na, c)[:, :nk].reshape(b * nk, c)
        return {n: _unrows(torch.from_numpy(p.copy()).double(), b, cs.heads) for n, p in zip(("dq", "dk", "dv"), parts)}, raws


# ------------------------------------------------------------------------------------------------------------------------------------
# idb_lora_grad
# ------------------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class LoraCase:
    name: str
    m: int
    n_in: int
    n_out: int
    rank: int
    recipe: str = "normal"           # "normal", "b_zero" (upstream's initial state), "integer" (both gradients exact)
    sliced: bool = False             # dy is the middle third of a [m][3 out] buffer
    scale: float = 0.5


def lora_chunk_rows(m: int) -> int:
    cr, cap = L.IDB_LORA_GRAD_CHUNK_ROWS, L.IDB_LORA_GRAD_MAX_CHUNKS
    return cr if m <= cr * cap else -(-m // cap)


def lora_cases() -> List[LoraCase]:
    cr, cap = L.IDB_LORA_GRAD_CHUNK_ROWS, L.IDB_LORA_GRAD_MAX_CHUNKS
    return [
        LoraCase("one_row", 1, 64, 64, 4),
        LoraCase("chunk_minus", cr - 1, 64, 128, 1),
        LoraCase("chunk_exact", cr, 128, 64, 5),
        LoraCase("chunk_plus", cr + 1, 64, 128, 16, sliced=True),
        LoraCase("cap_exact", cr * cap, 64, 128, 4),
        LoraCase("cap_plus", cr * cap + 1, 128, 64, 4, sliced=True),
        LoraCase("b_zero", 3 * cr + 7, 128, 64, 4, recipe="b_zero", sliced=True),
        LoraCase("integer", 5 * cr + 3, 64, 128, 5, recipe="integer"),
        LoraCase("integer_r16", 2 * cr + 1, 128, 64, 16, recipe="integer", sliced=True),
        LoraCase("wide", 70, 640, 320, 4, sliced=True),
    ]


def lora_inputs(case: LoraCase, dtype: str, seed: int = 62):
    """(x [m][in], dy [m][out] as float64 holders of T values, lora_a [rank][in], lora_b [out][rank] as float64 holders of fp32 values)."""
    g = torch.Generator().manual_seed(seed)
    m, i, o, r = case.m, case.n_in, case.n_out, case.rank
    if case.recipe == "integer":     # every product and sum is an integer below 2^24: exact in fp32 in any order; scale is a power of two
        ri = lambda *s: torch.randint(-2, 3, s, generator=g).double()
        return ri(m, i), ri(m, o), ri(r, i), ri(o, r)
    x = rnd(torch.randn(m, i, generator=g, dtype=torch.float32).double(), dtype)
    dy = rnd(torch.randn(m, o, generator=g, dtype=torch.float32).double(), dtype)
    a = (torch.randn(r, i, generator=g, dtype=torch.float32) / math.sqrt(r)).double()
    b = torch.zeros(o, r, dtype=F64) if case.recipe == "b_zero" else torch.randn(o, r, generator=g, dtype=torch.float32).double() * 0.1
    return x, dy, a, b


def lora_reference(case: LoraCase, x, dy, a, b):
    """(da, db, bound da, bound db) in float64.  u = x A^T is a sum of in / 64 terms per lane and a 6-level exchange, t = dy B likewise
    over out: worst-case gamma(in / 64 + 6) |x| |A|^T; the sum over m takes chunk-rows fp32 FMAs per chunk (gamma(chunk rows)), the
    chunks merge in double (nothing), the scale and the final rounding to fp32 one w.  B = 0 gives t = 0, a bound of 0 and so da == 0."""
    s = case.scale
    u, t = x @ a.T, dy @ b
    da, db = s * (t.T @ x), s * (dy.T @ u)
    e_u = MC.gamma(case.n_in // 64 + 6) * (x.abs() @ a.abs().T)
    e_t = MC.gamma(case.n_out // 64 + 6) * (dy.abs() @ b.abs())
    gc = MC.gamma(lora_chunk_rows(case.m) + 2)
    bda = abs(s) * (e_t.T @ x.abs() + gc * (t.abs().T @ x.abs())) + W32 * da.abs()
    bdb = abs(s) * (dy.abs().T @ e_u + gc * (dy.abs().T @ u.abs())) + W32 * db.abs()
    if case.recipe == "integer":
        bda, bdb = torch.zeros_like(bda), torch.zeros_like(bdb)
    return da, db, bda, bdb


def lora_emulate(case: LoraCase, x, dy, a, b, defect: Optional[str] = None):
    """fp32 u and t, fp32 chunk sums, chunks merged in double: (da, db).  Defects: "chunk_left_out" (the last chunk), "no_scale",
    "swap" (u and t exchanged roles is impossible by shape; instead da built from u's first columns: wrong projection)."""
    s = 1.0 if defect == "no_scale" else case.scale
    u, t = (x @ a.T).float().double(), (dy @ b).float().double()
    cr = lora_chunk_rows(case.m)
    starts = list(range(0, case.m, cr))
    if defect == "chunk_left_out" and len(starts) > 1:
        starts = starts[:-1]
    da = sum((t[i:i + cr].T @ x[i:i + cr]).float().double() for i in starts)
    db = sum((dy[i:i + cr].T @ u[i:i + cr]).float().double() for i in starts)
    return (s * da).float().double(), (s * db).float().double()


class LoraDevice:
    def __init__(self, case: LoraCase, x, dy, a, b, dtype: str):
        self.case, t = case, TDT[dtype]
        self.x = x.to(t).to(MC.DEV)
        self.dy_ld = 3 * case.n_out if case.sliced else case.n_out
        buf = torch.full((case.m, self.dy_ld), math.nan, dtype=t)
        off = case.n_out if case.sliced else 0
        buf[:, off:off + case.n_out] = dy.to(t)
        self.dyb = buf.to(MC.DEV)
        self.dy_ptr = self.dyb.data_ptr() + 2 * off
        self.a, self.b = a.float().contiguous().to(MC.DEV), b.float().contiguous().to(MC.DEV)
        self.dtype = dtype

    def run(self, lib):
        cs = self.case
        self.da, self.db = MC.Guarded(cs.rank * cs.n_in, 4), MC.Guarded(cs.n_out * cs.rank, 4)
        need = lib.idb_lora_grad_workspace_bytes(cs.m, cs.n_in, cs.n_out, cs.rank)
        assert need > 0 and need % 4 == 0
        self.ws = MC.Guarded(need // 4, 4)
        rc = lib.idb_lora_grad(self.x.data_ptr(), cs.n_in, self.dy_ptr, self.dy_ld, self.a.data_ptr(), self.b.data_ptr(), self.da.ptr, self.db.ptr,
                               cs.m, cs.n_in, cs.n_out, cs.rank, cs.scale, self.ws.ptr, need, IDB_DT[self.dtype], MC.stream())
        return rc

    def results(self):
        cs = self.case
        self.ws.raw("workspace")
        da, db = self.da.f32("da").copy(), self.db.f32("db").copy()
        return (torch.from_numpy(da).double().reshape(cs.rank, cs.n_in), torch.from_numpy(db).double().reshape(cs.n_out, cs.rank), da, db)


def with_(case, **kw):
    return replace(case, **kw)
