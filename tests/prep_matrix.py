"""The test matrix of the load-time weight preparation and of the fp32 latent path in csrc/idb_misc.hip: idb_pack_conv_weight,
idb_pack_matrix, idb_pack_matrix_scaled, idb_lora_merge, idb_lora_merge_scaled, idb_tile_weight, idb_ln_fold_vectors, idb_cfg_ddpm_step,
idb_vae_sample, idb_postprocess, idb_cast_f32, idb_nhwc_to_nchw_f32, idb_f32_nhwc_to_nchw and idb_embed_tokens.  Shared by
test_prep_matrix_cpu.py (recipes, teeth, emulations, argument checks) and test_prep_matrix_gpu.py (launch + compare): cases at the smallest
shapes that can go wrong, input recipes from fixed seeds, float64 references written from the definitions, numpy float32 emulations of the
kernels' arithmetic, injectable defects and the element-wise criteria.  numpy only, no GPU.  The helpers (gamma, check, describe, to_bits,
from_bits, round_T, bf16_bits, fma32, U_T, SUB_T, GUARD, NAN32, NAN16) are matrix_common.py's; the emulations' fmaf (_fma), the keyed
generator (_rng) and the bound of a rounding to T (_t_bound) are stem_matrix.py's, whose recipes they were written for.

Every kernel but ln_fold_vectors runs one thread per element (tile_weight, embed_tokens: per 16-byte chunk / four features) in 256-thread
blocks, so every family has a single element, a total below 256 and a ragged second block (tile_weight's chunk count is a multiple of
128: one half block, one whole block, several).  ln_fold_vectors runs one wave per row, four rows per block.

Criteria, per element.  u = 2^-24, gamma_n = n u / (1 - n u), u_T and sub_T as in matrix_common.py.  Every count is read off the kernel.

  bit-equal      pack_conv_weight, pack_matrix, cast_f32: one rounding to nearest even of the fp32 source [1], against round_T.  Both
                 transposes (no arithmetic), tile_weight (a copy; the rows past n are zeros), postprocess, vae_sample's mean (a copy)
                 and logvar (fmaxf / fminf round nothing).
                 postprocess: v = x * 0.5 [exact] + 0.5 [1], two clamps [0]; u8 = trunc(clamp(v * 255 + 0.5)), the sum rounded once
                 (fused) or twice (unfused): post_fused_differs() finds on the CPU that both give the same byte for every fp32 v
                 within 4096 ulp of each threshold (k + 0.5) / 255, the only places where they could differ, so the reference is the
                 unfused definition in numpy float32 and the device must equal it whichever way the compiler went.
  set of two     pack_matrix_scaled, lora_merge_scaled with rank 0 (src * col_scale) and embed_tokens (tok + pos): ONE exact operation,
                 then the conversion to T.  The exact result is a float64 (a product of two fp32 values has 48 bits; the embed recipe
                 keeps the two exponents within 2^28 of each other, asserted on the CPU).  The stored bits must be the exact value
                 rounded to T (round_exact_T: to fp32 to odd, then to T, exact because 24 >= 11 + 2) or its fp32 rounding rounded
                 to T; nothing else passes.  Each scaled recipe plants operand pairs whose two roundings differ (twice_pairs), so the
                 summary can say which one a dtype produced.
  lora_merge     d = sum_k b a: one multiply [1] and at most `rank` additions [rank] on a term (or `rank` fmaf's, fewer); scale * d and
  (_scaled)      the addition to w [2, or one fmaf]; the column scale [1, scaled form].  n = rank + 3 (+ 1 scaled):
                     e = gamma_n (|w| + |scale| sum_k |b| |a|) |cs|,     bound = _t_bound(ref, e, dt) = e + max(u_T (|ref| + e), sub_T).
  ln_fold        L = ceil(cols / 64) elements per lane.  u: L additions in the lane [L], six shuffle additions [6]: gamma_(L + 6) sum |wq|,
                 wq being the 16-bit matrix the test hands in, against the float64 row sum of those rounded values.
                 v: a W term passes its multiply [1], at most L + rank additions in the lane, six shuffle additions and the bias
                 addition [L + rank + 7]; an adapter term passes a beta [1, L additions], scale * b [1], the product [1] and at most
                 rank + 7 additions.  n' = L + 8 without an adapter, L + rank + 10 with one:
                     gamma_n' (sum |w beta| + |scale| sum_j |b_j| sum |a_j beta| + |bias|).
  cfg_ddpm       float64 reference from the fp32 inputs and the six fp32 coefficients.  Longest path of one term: guidance
                 e = eu + g (ec - eu) [3, cfg only]; x0 = (x - sb e) / sa [3] or sa x - sb e [2]; prev = c_x0 x0 + c_x x [2];
                 + sigma noise [1].  n_x0 = 3 cfg + (2 if v-prediction else 3), n_prev = n_x0 + 2 + (1 with noise); the bound is
                 gamma_n A with A the same formula over absolute values and the division by |sa|.  Contracted multiply-adds round less.
  vae_sample     z = (mean + exp(0.5 logvar) noise) scale: 0.5 logvar exact, expf approximate, then a multiply, an addition and the
                 scale [3].  r = worst relative error of numpy's float32 exp against float64 on the case's inputs, allowance
                 a = max(3 r, 4 u) (3: device transcendentals against numpy's, the project's standing factor), E = |exp(.) noise|:
                     bound = |scale| (a E + gamma_3 (|mean| + (1 + a) E));      noise = NULL: z = mean scale [1], gamma_1 |mean scale|.

The unmodified emulations must meet every bounded criterion at err / bound <= 0.5 and every bit-equal one exactly
(test_prep_matrix_cpu.py); for lora_merge, which rounds to T, the half applies to e (e_scale), as in stem_matrix.py.  Two bounds are
sharp in the same sense as the rounding to T there, and are asked whole, not halved: vae_sample without noise (ONE rounding: the
correctly rounded product attains u |ref|, measured 0.97) and cfg_ddpm's x0 (a chain of two or three roundings after the guidance, in
which the last one acts on the whole result: a correctly rounded evaluation reaches (A + |x0|) / (n A) of gamma_n A, up to 1 for n = 2;
measured 0.89 at v-prediction without guidance).  The new latents, whose longest path is two to three roundings longer than most of
their terms', are held to the half.

The postprocess sweep holds 2^21 inputs.  "Every x whose v lies in a window" is not a finite-sized set worth launching: the window about
v = 0.5 (k = 127) alone is reached from every fp32 below 2^-12 in magnitude, 2 x 10^9 values.  The sweep therefore takes, for every v of
the 255 windows, the fp32 nearest 2 v - 1, keeps those whose v falls into a window, and fills up to 2^21 with the next fp32 values
about them; the CPU test asserts that every v of the windows that any x can reach (v >= 0.5: all of them) is reached.

DEFECTS lists what is injected into the emulations and DEFECT_CASES the named case each must fail; none is HARMLESS."""
from dataclasses import dataclass
from functools import lru_cache
from typing import Optional, Tuple

import numpy as np

from matrix_common import (DTYPES, F32, F64, GUARD, NAN16, NAN32, SUB_T, U, U_T, bf16_bits, check, describe, fma32, from_bits,  # noqa: F401
                           gamma, round_T, to_bits)                            # re-exported to the two test files
from stem_matrix import _fma, _rng, _t_bound

ELEMENT_LIMIT = 1 << 39               # idb_misc.hip below_2p39: blocks_for returns unsigned, 2^31 blocks of 256


# ------------------------------------------------------------------------------------------------------------------------------------
# roundings
# ------------------------------------------------------------------------------------------------------------------------------------
def f32_odd(x64) -> np.ndarray:
    """float64 -> fp32 rounded to odd: the neighbour with an odd last bit when the value is not an fp32."""
    x64 = np.asarray(x64, F64)
    f = x64.astype(F32)
    inexact = f.astype(F64) != x64
    even = (f.view(np.uint32) & 1) == 0
    toward = np.where(x64 > f.astype(F64), F32(np.inf), F32(-np.inf)).astype(F32)
    return np.where(inexact & even, np.nextafter(f, toward), f).astype(F32)


def round_exact_T(x64, dt) -> np.ndarray:
    """The 16 bits of the float64 value rounded ONCE to T."""
    return to_bits(f32_odd(x64), dt)


def admissible(x64, dt) -> Tuple[np.ndarray, np.ndarray]:
    """(bits of the exact value rounded once to T, bits of its fp32 rounding rounded to T)."""
    x64 = np.asarray(x64, F64)
    return round_exact_T(x64, dt), to_bits(x64.astype(F32), dt)


def member(bits, x64, dt):
    """(ok, index of the first element outside the admissible set or None, elements equal to the once / twice value where they differ)."""
    once, twice = admissible(x64, dt)
    bits = np.asarray(bits, np.uint16).reshape(once.shape)
    bad = np.argwhere((bits != once) & (bits != twice))
    sep = once != twice
    return bad.size == 0, (tuple(int(v) for v in bad[0]) if bad.size else None), int((sep & (bits == once)).sum()), int((sep & (bits == twice)).sum())


def trunc_bits(v, dt) -> np.ndarray:
    """fp32 -> T by truncation (the defect): the nearest value of T not larger in magnitude."""
    v = np.asarray(v, F32)
    b = to_bits(v, dt)
    over = np.abs(from_bits(b, dt).reshape(v.shape)) > np.abs(v)
    return np.where(over, b - np.uint16(1), b).astype(np.uint16)


def _to_T(v, dt, defect=None) -> np.ndarray:
    return trunc_bits(v, dt) if defect == "truncate" else to_bits(v, dt)


@lru_cache(maxsize=None)
def twice_pairs(dt: str, kind: str = "mul"):
    """Four fp32 pairs (a, b) whose exact product (kind "mul") or sum ("add") rounds to a different T once than through fp32: the fp32
    rounding lands on a tie of T that the exact value is not on.  Found by search, verified here."""
    out = []
    spacing = 2.0 * U_T[dt]                              # of T in [1, 2)
    j = 0
    while len(out) < 4:
        j += 1
        tie = 1.0 + spacing * (2 * (j % 5) + 0.5 + (j % 2))      # odd multiples of the half spacing
        if kind == "mul":
            a = F32(1.0 + 0.173 * j / (1 + 0.01 * j) % 0.9)
            b = F32(tie / float(a))
        else:
            a, b = F32(tie), F32((-1.0) ** j * 2.0 ** -(26 + j % 3))
        exact = float(a) * float(b) if kind == "mul" else float(a) + float(b)
        o, t = admissible(np.array([exact]), dt)
        if o[0] != t[0]:
            out.append((a, b))
    return np.array([p[0] for p in out], F32), np.array([p[1] for p in out], F32)


# ------------------------------------------------------------------------------------------------------------------------------------
# idb_pack_conv_weight
# ------------------------------------------------------------------------------------------------------------------------------------
PACK_CONV_SHAPES = ((1, 1, 1), (3, 5, 9), (5, 13, 4), (8, 64, 9), (2, 67, 1))          # (cout, cin, taps): 1, 135, 260, 4608, 134 elements


@lru_cache(maxsize=None)
def pack_conv_input(shape) -> np.ndarray:
    return _rng("pack_conv", shape).normal(size=shape).astype(F32)


def pack_conv_reference(shape, dt) -> np.ndarray:
    """uint16 [cout][taps][cin]."""
    return to_bits(pack_conv_input(shape).transpose(0, 2, 1), dt)


def emulate_pack_conv(shape, dt, defect=None) -> np.ndarray:
    src = pack_conv_input(shape)
    cout, cin, taps = shape
    v = src.reshape(cout, taps, cin) if defect == "conv_untransposed" else src.transpose(0, 2, 1)
    return _to_T(np.ascontiguousarray(v), dt, defect)


# ------------------------------------------------------------------------------------------------------------------------------------
# idb_pack_matrix, idb_pack_matrix_scaled
# ------------------------------------------------------------------------------------------------------------------------------------
PACK_MATRIX_SHAPES = ((1, 1, 0), (7, 37, 0), (32, 3, 1), (96, 5, 1), (64, 64, 1))       # (rows, cols, geglu): 1, 259, 96, 480, 4096 elements


def geglu_rows(rows: int, group: int = 16, gate_first: bool = False) -> np.ndarray:
    """Source row of every packed row, from the header's sentence: value rows and gate rows (the second half of the matrix) alternate
    in groups of 16."""
    half, out = rows // 2, []
    for g in range(half // group):
        value, gate = list(range(group * g, group * g + group)), list(range(half + group * g, half + group * g + group))
        out += gate + value if gate_first else value + gate
    return np.asarray(out, np.int64)


def _src_rows(rows, geglu, defect=None) -> np.ndarray:
    if not geglu:
        return np.arange(rows)
    return geglu_rows(rows, 32 if defect == "geglu_groups_32" else 16, defect == "geglu_halves_swapped")


@lru_cache(maxsize=None)
def matrix_inputs(shape, dt: Optional[str] = None):
    """(src fp32 [rows][cols], col_scale fp32 [cols], non-constant and of both signs).  With a dtype, the first columns hold the pairs of
    twice_pairs: col_scale[c] = b_c and every row's src[r][c] = a_c."""
    rows, cols = shape[:2]
    rng = _rng("matrix", shape[:2])
    src = rng.normal(size=(rows, cols)).astype(F32)
    cs = (rng.uniform(0.5, 1.5, size=cols) * np.where(np.arange(cols) % 3 == 1, -1.0, 1.0)).astype(F32)
    if dt is not None:
        a, b = twice_pairs(dt)
        k = min(cols, 4)
        src[:, :k], cs[:k] = a[:k], b[:k]
    return src, cs


def pack_matrix_reference(shape, dt) -> np.ndarray:
    rows, cols, geglu = shape
    return to_bits(matrix_inputs(shape)[0][_src_rows(rows, geglu)], dt)


def emulate_pack_matrix(shape, dt, defect=None) -> np.ndarray:
    rows, cols, geglu = shape
    return _to_T(matrix_inputs(shape)[0][_src_rows(rows, geglu, defect)], dt, defect)


def pack_scaled_exact(shape, dt) -> np.ndarray:
    """float64 [rows][cols]: the exact products."""
    rows, cols, geglu = shape
    src, cs = matrix_inputs(shape, dt)
    return src[_src_rows(rows, geglu)].astype(F64) * cs.astype(F64)


def emulate_pack_scaled(shape, dt, defect=None, fused=False) -> np.ndarray:
    rows, cols, geglu = shape
    src, cs = matrix_inputs(shape, dt)
    v = src[_src_rows(rows, geglu, defect)]
    s = cs[np.arange(rows) % cols][:, None] if defect == "cs_by_row" else cs[None]
    if fused and defect is None:
        return round_exact_T(v.astype(F64) * s.astype(F64), dt)
    return _to_T(v * s, dt, defect)


# ------------------------------------------------------------------------------------------------------------------------------------
# idb_lora_merge, idb_lora_merge_scaled
# ------------------------------------------------------------------------------------------------------------------------------------
LORA_SHAPES = ((1, 1, 1), (3, 21, 2), (7, 37, 4), (33, 64, 16), (5, 130, 3))          # (rows, cols, rank): 1, 63, 259, 2112, 650 elements
LORA_SCALES = (0.5, -1.75)


@dataclass(frozen=True)
class LoraCase:
    shape: Tuple[int, int, int]
    scale: float
    scaled: bool                      # idb_lora_merge_scaled
    rank0: bool = False               # scaled form with NULL adapters

    @property
    def rank(self):
        return 0 if self.rank0 else self.shape[2]

    @property
    def name(self):
        return "r{}_c{}_rank{}".format(self.shape[0], self.shape[1], self.rank) + f"_s{self.scale}_{'scaled' if self.scaled else 'plain'}"


def lora_cases():
    out = [LoraCase(s, sc, scaled) for s in LORA_SHAPES for sc in LORA_SCALES for scaled in (False, True)]
    return out + [LoraCase(s, LORA_SCALES[i % 2], True, True) for i, s in enumerate(LORA_SHAPES)]


@lru_cache(maxsize=None)
def lora_inputs(case: LoraCase, dt: Optional[str] = None):
    """(w [rows][cols], A [rank][cols], B [rows][rank], col_scale [cols]); rank 0 plants twice_pairs as matrix_inputs does."""
    rows, cols, rank = case.shape
    rng = _rng("lora", case.shape)
    w = rng.normal(size=(rows, cols)).astype(F32)
    a = rng.normal(size=(rank, cols)).astype(F32)
    b = (rng.normal(size=(rows, rank)) * 0.5).astype(F32)
    cs = (rng.uniform(0.5, 1.5, size=cols) * np.where(np.arange(cols) % 3 == 1, -1.0, 1.0)).astype(F32)
    if case.rank0 and dt is not None:
        pa, pb = twice_pairs(dt)
        k = min(cols, 4)
        w[:, :k], cs[:k] = pa[:k], pb[:k]
    return w, a, b, cs


def lora_roundings(case: LoraCase) -> int:
    return case.rank + 3 + (1 if case.scaled else 0)


def lora_reference(case: LoraCase, dt, e_scale=1.0):
    """(ref float64 [rows][cols], bound) for rank > 0; rank 0 is judged by `member` on lora_exact."""
    w, a, b, cs = (v.astype(F64) for v in lora_inputs(case, dt))
    s = float(F32(case.scale))
    c = cs if case.scaled else np.ones_like(cs)
    ref = (w + s * (b @ a)) * c
    mag = (np.abs(w) + abs(s) * (np.abs(b) @ np.abs(a))) * np.abs(c)
    return ref, _t_bound(ref, e_scale * gamma(lora_roundings(case)) * mag, dt)


def lora_exact(case: LoraCase, dt) -> np.ndarray:
    w, _, _, cs = lora_inputs(case, dt)
    return w.astype(F64) * cs.astype(F64)


def emulate_lora(case: LoraCase, dt, defect=None) -> np.ndarray:
    """uint16 [rows][cols]: d by fmaf's over ascending k from 0, fmaf(scale, d, w), the column scale, one rounding to T."""
    w, a, b, cs = lora_inputs(case, dt)
    rows, cols, rank = case.shape
    bm = b.reshape(-1)[(np.arange(rank)[None] * rows + np.arange(rows)[:, None])] if defect == "lora_b_transposed" else b
    d = np.zeros((rows, cols), F32)
    for k in range(case.rank):
        d = _fma(bm[:, k, None].astype(F64), a[None, k].astype(F64), d)
    v = fma32(F32(1.0 if defect == "lora_scale_dropped" else case.scale), d, w).reshape(rows, cols)
    if case.scaled:
        v = v * (cs[np.arange(rows) % cols][:, None] if defect == "cs_by_row" else cs[None])
    return _to_T(v.astype(F32), dt, defect)


# ------------------------------------------------------------------------------------------------------------------------------------
# idb_tile_weight
# ------------------------------------------------------------------------------------------------------------------------------------
TILE_SHAPES = ((1, 64), (16, 64), (17, 128), (3, 128), (250, 192))                    # (n, k): 128, 128, 512, 256, 6144 16-byte chunks


def tiled_bytes(n, k) -> int:
    return (n + 15) // 16 * 16 * k * 2


@lru_cache(maxsize=None)
def tile_input(shape) -> np.ndarray:
    """uint16 [n][k]: finite patterns of either dtype, every one distinct from the NaN pre-fill."""
    n, k = shape
    return _rng("tile", shape).integers(1, 0x7C00, size=(n, k)).astype(np.uint16)


def tile_reference(shape, defect=None) -> np.ndarray:
    """uint16 [ceil(n / 16)][k / 64][16][64], the rows past n zero (NAN16, the pre-fill, under the defect that leaves them alone)."""
    n, k = shape
    nb, kt = (n + 15) // 16, k // 64
    pad = np.full((nb * 16, k), NAN16 if defect == "tile_pad_unzeroed" else 0, np.uint16)
    pad[:n] = tile_input(shape)
    t = pad.reshape(nb, 16, kt, 64).transpose(0, 2, 1, 3)
    if defect == "tile_order_swapped":
        t = t.transpose(1, 0, 2, 3).reshape(nb, kt, 16, 64)
    return np.ascontiguousarray(t)


# ------------------------------------------------------------------------------------------------------------------------------------
# idb_ln_fold_vectors
# ------------------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class FoldCase:
    rows: int
    cols: int
    rank: int
    geglu: int
    bias: bool
    null_a: bool = False              # lora_a = NULL with rank > 0: the header says no adapter

    @property
    def name(self):
        return f"r{self.rows}_c{self.cols}_rank{self.rank}_{'geglu' if self.geglu else 'plain'}_{'bias' if self.bias else 'nobias'}" + ("_nullA" if self.null_a else "")

    @property
    def eff_rank(self):
        return 0 if self.null_a else self.rank


FOLD_CASES = (FoldCase(1, 1, 0, 0, True), FoldCase(5, 63, 0, 0, True), FoldCase(6, 65, 3, 0, True), FoldCase(32, 64, 0, 1, True),
              FoldCase(96, 200, 16, 1, True), FoldCase(7, 320, 4, 0, False), FoldCase(9, 70, 4, 0, True, True))
FOLD_SCALE = -1.75


@lru_cache(maxsize=None)
def fold_inputs(case: FoldCase, dt):
    """(w [rows][cols], A [rank][cols], B [rows][rank], wq fp32 [rows][cols] holding T values in PACKED row order, beta [cols], bias [rows])."""
    rng = _rng("fold", case.rows, case.cols, case.rank, case.geglu)
    w = rng.normal(size=(case.rows, case.cols)).astype(F32)
    a = rng.normal(size=(max(case.rank, 1), case.cols)).astype(F32)[:case.rank]
    b = (rng.normal(size=(case.rows, max(case.rank, 1))) * 0.5).astype(F32)[:, :case.rank]
    g = rng.uniform(0.5, 1.5, size=case.cols).astype(F32)
    beta = rng.normal(size=case.cols).astype(F32)
    bias = (rng.normal(size=case.rows) + 3.0).astype(F32)
    wq = w[_src_rows(case.rows, case.geglu)] * g[None]
    return w, a, b, (wq if dt is None else round_T(wq, dt)), beta, bias


def fold_unrounded(case: FoldCase) -> np.ndarray:
    """The fp32 matrix whose rounding to T is w_folded."""
    return fold_inputs(case, None)[3]


def fold_roundings(case: FoldCase) -> Tuple[int, int]:
    lanes = (case.cols + 63) // 64
    return lanes + 6, lanes + 8 + (case.eff_rank + 2 if case.eff_rank else 0)


def fold_reference(case: FoldCase, dt):
    """(u float64 [rows], its bound, v, its bound)."""
    w, a, b, wq, beta, bias = (x.astype(F64) for x in fold_inputs(case, dt))
    sr = _src_rows(case.rows, case.geglu)
    nu, nv = fold_roundings(case)
    u, bu = wq.sum(1), gamma(nu) * np.abs(wq).sum(1)
    v, mag = w[sr] @ beta, np.abs(w[sr]) @ np.abs(beta)
    if case.eff_rank:
        s = float(F32(FOLD_SCALE))
        v = v + s * (b[sr] @ (a @ beta))
        mag = mag + abs(s) * (np.abs(b[sr]) @ (np.abs(a) @ np.abs(beta)))
    if case.bias:
        v, mag = v + bias, mag + np.abs(bias)
    return u, bu, v, gamma(nv) * mag


def emulate_fold(case: FoldCase, dt, defect=None):
    """(u, v) fp32 [rows]: lane l sums columns l, l + 64, ... (fmaf for the W term), then per adapter row j its own a beta chain and
    fmaf(scale * b, ab, sv); the xor shuffle tree 32, 16, ... 1; lane 0 adds the bias."""
    w, a, b, wq, beta, bias = fold_inputs(case, dt)
    rows, cols = case.rows, case.cols
    sr = np.arange(rows) if defect == "v_row_r" else _src_rows(rows, case.geglu)
    usrc = fold_unrounded(case) if defect == "u_unrounded" else wq
    su, sv = np.zeros((rows, 64), F32), np.zeros((rows, 64), F32)
    ab = np.zeros((case.eff_rank, 64), F32)
    for base in range(0, cols, 64):
        idx = np.arange(base, min(base + 64, cols))
        ln = idx - base
        su[:, ln] = su[:, ln] + usrc[:, idx]
        sv[:, ln] = _fma(w[sr][:, idx].astype(F64), beta[None, idx].astype(F64), sv[:, ln])
        if case.eff_rank:
            ab[:, ln] = _fma(a[:, idx].astype(F64), beta[None, idx].astype(F64), ab[:, ln])
    for j in range(case.eff_rank):
        sb = (F32(FOLD_SCALE) * b[sr][:, j]).astype(F32)
        sv = _fma(sb[:, None].astype(F64), ab[None, j].astype(F64), sv)
    for o in (32, 16, 8, 4, 2, 1):
        su, sv = su + su[:, np.arange(64) ^ o], sv + sv[:, np.arange(64) ^ o]
    v = sv[:, 0] + (bias if case.bias and defect != "v_no_bias" else F32(0))
    return su[:, 0].astype(F32), v.astype(F32)


# ------------------------------------------------------------------------------------------------------------------------------------
# idb_cast_f32
# ------------------------------------------------------------------------------------------------------------------------------------
CAST_COUNTS = (1, 255, 257)


def _nb(v, k=1):
    """The fp32 k steps above (k > 0) or below v."""
    return (np.array([v], F32).view(np.int32) + np.int32(k)).view(F32)[0] if v > 0 else (np.array([v], F32).view(np.int32) - np.int32(k)).view(F32)[0]


@lru_cache(maxsize=None)
def cast_table() -> np.ndarray:
    """The edge values of both dtypes, each with its negative."""
    h = 2.0 ** -11                                    # half a spacing of f16 at 1
    vals = [1 + h, 1 + 3 * h, _nb(F32(1 + h)), _nb(F32(1 + h), -1), _nb(F32(1 + 3 * h)), _nb(F32(1 + 3 * h), -1),       # f16 ties to even both ways
            2.0 ** -24, 2.0 ** -25, _nb(F32(2.0 ** -25)), 3 * 2.0 ** -25, 2.0 ** -14, _nb(F32(2.0 ** -14)), _nb(F32(2.0 ** -14), -1),
            65504.0, 65519.996, 65520.0, _nb(F32(65520.0), -1), 70000.0,
            1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, _nb(F32(1 + 2.0 ** -8)), _nb(F32(1 + 2.0 ** -8), -1), _nb(F32(1 + 3 * 2.0 ** -8)), _nb(F32(1 + 3 * 2.0 ** -8), -1),
            float(from_bits(np.array([0x7F7F], np.uint16), "bf16")[0]), float(np.finfo(F32).max), _nb(F32(np.finfo(F32).max), -0x7FFF), _nb(F32(np.finfo(F32).max), -0x8000),
            float(np.finfo(F32).tiny), 1e-40, 1.4e-45, 2.0 ** -133, 2.0 ** -134, 3 * 2.0 ** -134,                     # fp32 subnormals; bf16's smallest, its tie
            0.0, np.inf, 1.0, 0.333333, 3.14159, 1000.123]
    v = np.array(vals, F32)
    return np.concatenate([v, -v, np.array([NAN32, NAN32 | 0x80000000, 0x7F800001], np.uint32).view(F32)])


def cast_input(count: int) -> np.ndarray:
    t = cast_table()
    return t[np.arange(count) % t.size]


def cast_reference(count, dt):
    """(uint16 bits, mask of the elements compared bit for bit: all but the NaNs, which must come out as NaNs)."""
    x = cast_input(count)
    with np.errstate(over="ignore"):
        return to_bits(x, dt), ~np.isnan(x)


# ------------------------------------------------------------------------------------------------------------------------------------
# idb_nhwc_to_nchw_f32, idb_f32_nhwc_to_nchw
# ------------------------------------------------------------------------------------------------------------------------------------
TRANSPOSE_SHAPES = ((1, 1, 1), (2, 3, 5), (3, 7, 4), (1, 257, 3))                     # (batch, hw, c): 1, 30, 84, 771 elements


@lru_cache(maxsize=None)
def transpose_input(shape, dt) -> np.ndarray:
    """[batch][hw][c]: fp32 values (dt "f32") or 16-bit patterns of finite values of T."""
    rng = _rng("transpose", shape, dt)
    if dt == "f32":
        return rng.normal(size=shape).astype(F32)
    return rng.integers(0, 0x7C00, size=shape).astype(np.uint16) | (rng.integers(0, 2, size=shape).astype(np.uint16) << np.uint16(15))


def transpose_reference(shape, dt, defect=None) -> np.ndarray:
    """fp32 [batch][c][hw]."""
    x = transpose_input(shape, dt)
    v = x if dt == "f32" else from_bits(x, dt).reshape(shape)
    b, hw, c = shape
    return np.ascontiguousarray(v.reshape(b, c, hw) if defect == "transpose_copy" else v.transpose(0, 2, 1))


# ------------------------------------------------------------------------------------------------------------------------------------
# idb_embed_tokens
# ------------------------------------------------------------------------------------------------------------------------------------
EMBED_SHAPES = ((1, 1, 4, 1), (2, 3, 8, 5), (3, 77, 12, 50))                          # (batch, n_tokens, dim, vocab): 1, 12, 693 threads


@lru_cache(maxsize=None)
def embed_inputs(shape, dt):
    """(ids int64 [batch * n_tokens] with 0, vocab - 1 and repeats; tok fp32 [vocab][dim]; pos fp32 [n_tokens][dim]).  Feature 0 of the
    first vocabulary and position rows holds a pair of twice_pairs(dt, "add")."""
    batch, n_tokens, dim, vocab = shape
    rng = _rng("embed", shape)
    ids = rng.integers(0, vocab, size=batch * n_tokens).astype(np.int64)
    ids[0] = 0
    ids[-1] = vocab - 1
    if ids.size > 2:
        ids[1] = ids[2] = vocab // 2
    sign = lambda s: np.where(rng.integers(0, 2, size=s) == 1, -1.0, 1.0)   # noqa: E731
    tok = (rng.uniform(0.25, 4.0, size=(vocab, dim)) * sign((vocab, dim))).astype(F32)
    pos = (rng.uniform(0.25, 4.0, size=(n_tokens, dim)) * sign((n_tokens, dim))).astype(F32)
    a, b = twice_pairs(dt, "add")
    tok[0, :4], pos[0, :4] = a, b
    return ids, tok, pos


def embed_exact(shape, dt, defect=None) -> np.ndarray:
    """float64 [batch * n_tokens][dim]: tok[id] + pos[row % n_tokens], exact (the exponents are within 2^28 of each other)."""
    ids, tok, pos = embed_inputs(shape, dt)
    batch, n_tokens, dim, vocab = shape
    rows = np.arange(batch * n_tokens)
    if defect == "pos_by_row":                            # the rows past the table are not the kernel's to read: NaN stands for them
        p = np.concatenate([pos.astype(F64), np.full(((batch - 1) * n_tokens, dim), np.nan)])[rows]
    else:
        p = pos.astype(F64)[rows % n_tokens]
    return tok.astype(F64)[ids] + p


def emulate_embed(shape, dt, defect=None) -> np.ndarray:
    with np.errstate(invalid="ignore"):
        return to_bits(embed_exact(shape, dt, defect).astype(F32), dt)


# ------------------------------------------------------------------------------------------------------------------------------------
# idb_postprocess
# ------------------------------------------------------------------------------------------------------------------------------------
POST_WINDOW = 4096                    # fp32 steps on each side of a threshold
POST_SWEEP = 1 << 21


@lru_cache(maxsize=None)
def post_window_v() -> np.ndarray:
    """Every fp32 v within POST_WINDOW steps of a threshold (k + 0.5) / 255, k = 0..254: 255 x 8193 values, ascending."""
    th = ((np.arange(255) + 0.5) / 255.0).astype(F32)
    bits = th.view(np.int32)[:, None] + np.arange(-POST_WINDOW, POST_WINDOW + 1, dtype=np.int32)[None]
    return bits.reshape(-1).view(F32)


def post_v(x) -> np.ndarray:
    """img01 of the definition, one fp32 operation at a time."""
    x = np.asarray(x, F32)
    with np.errstate(invalid="ignore"):
        return np.minimum(np.maximum(x * F32(0.5) + F32(0.5), F32(0)), F32(1)).astype(F32)


def post_u8(v, fused=False, defect=None) -> np.ndarray:
    """uint8 of img01 values: trunc(clamp(v * 255 + 0.5, 0, 255)), the sum rounded twice (the definition) or once (fused)."""
    v = np.asarray(v, F32)
    if defect == "u8_half_even":
        return np.clip(np.rint(v * F32(255)), 0, 255).astype(np.uint8)
    t = fma32(v, F32(255), F32(0.5)).reshape(v.shape) if fused else (v * F32(255)).astype(F32) + F32(0.5)
    return np.minimum(np.maximum(t, F32(0)), F32(255)).astype(np.uint8)


@lru_cache(maxsize=None)
def post_sweep_input() -> np.ndarray:
    """fp32 [2^21], see the module docstring."""
    v = post_window_v()
    x = np.unique((2.0 * v.astype(F64) - 1.0).astype(F32))
    lo, hi = v.reshape(255, -1)[:, 0], v.reshape(255, -1)[:, -1]
    def inside(xx):   # noqa: E306
        vv = post_v(xx)
        k = np.clip(np.searchsorted(lo, vv, side="right") - 1, 0, 254)
        return (vv >= lo[k]) & (vv <= hi[k])
    x = x[inside(x)]
    step = 1
    while x.size < POST_SWEEP:                            # the next fp32 values about them, while they still fall into a window
        more = np.concatenate([(x.view(np.int32) + np.int32(step)).view(F32), (x.view(np.int32) - np.int32(step)).view(F32)])
        more = np.setdiff1d(more[inside(more)], x)
        x = np.union1d(x, more[:POST_SWEEP - x.size])
        step += 1
    return np.ascontiguousarray(x[:POST_SWEEP], F32)


@lru_cache(maxsize=None)
def post_edge_input() -> np.ndarray:
    """fp32 [257]: -1, 1 and their neighbours, +-0, +-2, +-inf, the rest inside and outside [-1, 1]."""
    one = F32(1)
    head = [-1.0, 1.0, _nb(one), _nb(one, -1), -_nb(one), -_nb(one, -1), 0.0, -0.0, 2.0, -2.0, np.inf, -np.inf, 1.5, -1.5, 1e-30, -1e-30, 0.99999, -0.99999]
    rest = _rng("post_edge").uniform(-1.5, 1.5, size=257 - len(head))
    return np.concatenate([np.array(head, F32), rest.astype(F32)])


POST_CASES = {"edge257": post_edge_input, "one": lambda: np.array([0.2503], F32), "below256": lambda: post_edge_input()[:200].copy(),
              "sweep": post_sweep_input}


@lru_cache(maxsize=None)
def post_reference(name):
    """(img01 fp32, u8)."""
    v = post_v(POST_CASES[name]())
    return v, post_u8(v)


def post_fused_differs() -> int:
    """How many v of the windows get another byte from the fused sum than from the unfused one."""
    v = post_window_v()
    return int((post_u8(v, fused=True) != post_u8(v)).sum())


def emulate_post(name, defect=None, fused=False):
    x = POST_CASES[name]()
    with np.errstate(invalid="ignore"):
        v = (x * F32(0.5) + F32(0.5)).astype(F32) if defect == "clamp_left_out" else post_v(x)
        return v, post_u8(v, fused, defect)


# ------------------------------------------------------------------------------------------------------------------------------------
# idb_vae_sample
# ------------------------------------------------------------------------------------------------------------------------------------
VAE_SHAPES = ((1, 1, 1), (2, 3, 5), (3, 4, 80), (1, 4, 257))                          # (batch, channels, hw): 1, 30, 960, 1028 elements
VAE_SCALE = 0.18215
LOGVAR_EDGES = (-30.0, 20.0, -30.000002, 20.000002, -29.999998, 19.999998, -45.0, 31.0, -3.0, 0.5)


@lru_cache(maxsize=None)
def vae_inputs(shape):
    """(moments fp32 [batch][hw][2 channels], noise fp32 [batch][channels][hw])."""
    b, c, hw = shape
    rng = _rng("vae", shape)
    mean = rng.normal(size=(b, hw, c)).astype(F32)
    lv = rng.uniform(-12.0, 6.0, size=(b, hw, c)).astype(F32)
    flat = lv.reshape(-1)
    idx = np.arange(0, flat.size, 3)[:len(LOGVAR_EDGES) * 2]
    flat[idx] = np.array(LOGVAR_EDGES, F32)[np.arange(idx.size) % len(LOGVAR_EDGES)]
    return np.concatenate([mean, lv], axis=2), rng.normal(size=(b, c, hw)).astype(F32)


def _vae_split(shape, defect=None):
    """(mean, clamped logvar) fp32 NCHW, as the kernel reads them."""
    b, c, hw = shape
    m, _ = vae_inputs(shape)
    if defect == "vae_nchw_read":
        m = m.reshape(b, 2 * c, hw).transpose(0, 2, 1)
    mean, lv = m[:, :, :c], m[:, :, c:]
    if defect == "moment_halves_swapped":
        mean, lv = lv, mean
    mean, lv = mean.transpose(0, 2, 1), lv.transpose(0, 2, 1)
    if defect != "logvar_unclamped":
        lv = np.minimum(np.maximum(lv, F32(-30)), F32(20))
    return np.ascontiguousarray(mean, F32), np.ascontiguousarray(lv, F32)


def vae_allowance(shape) -> Tuple[float, float]:
    """(max(3 r, 4 u), r): r the worst relative error of numpy's float32 exp on the case's clamped 0.5 logvar."""
    _, lv = _vae_split(shape)
    h = lv * F32(0.5)
    ref = np.exp(h.astype(F64))
    r = float((np.abs(np.exp(h).astype(F64) - ref) / ref).max())
    return max(3.0 * r, 4.0 * U), r


def vae_reference(shape, with_noise: bool):
    """(latents float64 NCHW, bound, mean fp32, logvar fp32)."""
    mean, lv = _vae_split(shape)
    s = float(F32(VAE_SCALE))
    if not with_noise:
        ref = mean.astype(F64) * s
        return ref, gamma(1) * np.abs(ref), mean, lv
    noise = vae_inputs(shape)[1].astype(F64)
    allow, _ = vae_allowance(shape)
    e = np.exp(0.5 * lv.astype(F64)) * noise
    ref = (mean.astype(F64) + e) * s
    return ref, abs(s) * (allow * np.abs(e) + gamma(3) * (np.abs(mean.astype(F64)) + (1.0 + allow) * np.abs(e))), mean, lv


def emulate_vae(shape, with_noise: bool, defect=None):
    """(latents, mean, logvar) fp32 NCHW."""
    mean, lv = _vae_split(shape, defect)
    z = mean
    if with_noise:
        with np.errstate(over="ignore"):
            z = (mean + (np.exp(lv if defect == "exp_full_logvar" else lv * F32(0.5)) * vae_inputs(shape)[1]).astype(F32)).astype(F32)
    return (z * F32(VAE_SCALE)).astype(F32), mean, lv


# ------------------------------------------------------------------------------------------------------------------------------------
# idb_cfg_ddpm_step
# ------------------------------------------------------------------------------------------------------------------------------------
CFG_SHAPES = ((1, 1, 1), (2, 3, 5), (2, 4, 64), (1, 4, 257))                          # (batch, C, hw): 1, 30, 512, 1028 elements
CFG_TIMESTEPS = (999, 500, 1, 0)
GUIDANCE = (0.0, 1.0, 5.0, 7.5)


@lru_cache(maxsize=None)
def ddpm_coefficients(t: int) -> Tuple[float, float, float, float, float]:
    """(sqrt(abar_t), sqrt(1 - abar_t), c_x0, c_x, sigma) of DDPMScheduler.step between t and t - 1 in float64: the scaled-linear
    schedule (betas = linspace(sqrt(0.00085), sqrt(0.012), 1000)^2), fixed_small variance, abar_-1 = 1, no noise at t = 0."""
    betas = np.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=F64) ** 2
    abar = np.cumprod(1.0 - betas)
    a_t, a_prev = abar[t], (abar[t - 1] if t > 0 else 1.0)
    cur_a = a_t / a_prev
    c_x0 = np.sqrt(a_prev) * (1.0 - cur_a) / (1.0 - a_t)
    c_x = np.sqrt(cur_a) * (1.0 - a_prev) / (1.0 - a_t)
    sigma = np.sqrt(max((1.0 - a_prev) / (1.0 - a_t) * (1.0 - cur_a), 1e-20)) if t > 0 else 0.0
    return float(np.sqrt(a_t)), float(np.sqrt(1.0 - a_t)), float(c_x0), float(c_x), float(sigma)


@dataclass(frozen=True)
class CfgCase:
    shape: Tuple[int, int, int]
    cfg: int
    vpred: int
    noise: bool
    x0: bool
    t: int
    g: float

    @property
    def name(self):
        return "b{}_C{}_hw{}".format(*self.shape) + f"_{'cfg' if self.cfg else 'nocfg'}_{'v' if self.vpred else 'eps'}_{'noise' if self.noise else 'nonoise'}_{'x0' if self.x0 else 'nox0'}_t{self.t}_g{self.g}"

    @property
    def coef(self) -> np.ndarray:
        """The six floats the kernel reads."""
        return np.array(ddpm_coefficients(self.t) + (self.g,), F32)


def cfg_cases():
    out, i = [], 0
    for cfg in (1, 0):
        for vpred in (0, 1):
            for noise in (True, False):
                for x0 in (True, False):                                   # all sixteen on (2, 3, 5); t and g rotate independently (4 and 5 apart)
                    out.append(CfgCase(CFG_SHAPES[1], cfg, vpred, noise, x0, CFG_TIMESTEPS[i % 4], GUIDANCE[(i // 4 + i) % 4]))
                    i += 1
    for shape in (CFG_SHAPES[0], CFG_SHAPES[2], CFG_SHAPES[3]):
        out += [CfgCase(shape, 1, 0, True, True, 999, 7.5), CfgCase(shape, 1, 1, False, True, 500, 5.0), CfgCase(shape, 0, 0, True, False, 1, 1.0),
                CfgCase(shape, 1, 0, False, False, 0, 0.0), CfgCase(shape, 0, 1, True, True, 999, 7.5)]
    return out


@lru_cache(maxsize=None)
def cfg_inputs(shape):
    """(eps fp32 [2 batch][hw][C], uncond first; latents fp32 [batch][C][hw]; noise fp32 [batch][C][hw])."""
    b, c, hw = shape
    rng = _rng("cfg", shape)
    return rng.normal(size=(2 * b, hw, c)).astype(F32), (rng.normal(size=(b, c, hw)) * 1.5).astype(F32), rng.normal(size=(b, c, hw)).astype(F32)


def cfg_roundings(case: CfgCase) -> Tuple[int, int]:
    """(n of x0, n of the new latents)."""
    n0 = 3 * case.cfg + (2 if case.vpred else 3)
    return n0, n0 + 2 + (1 if case.noise else 0)


def _cfg_eps(case: CfgCase, dtype, defect=None):
    b, c, hw = case.shape
    eps = cfg_inputs(case.shape)[0]
    if defect == "eps_nchw":
        eps = eps.reshape(2 * b, c, hw)
    else:
        eps = eps.transpose(0, 2, 1)
    eu, ec = eps[:b].astype(dtype), eps[b:].astype(dtype)
    return (ec, eu) if defect == "cond_uncond_swapped" else (eu, ec)


def cfg_reference(case: CfgCase):
    """(new latents float64 NCHW, bound, x0, bound)."""
    sa, sb, c0, cx, sigma, g = (float(v) for v in case.coef)
    eu, ec = _cfg_eps(case, F64)
    _, lat, noise = (v.astype(F64) for v in cfg_inputs(case.shape))
    e, ea = eu, np.abs(eu)
    if case.cfg:
        e, ea = eu + g * (ec - eu), np.abs(eu) + abs(g) * (np.abs(ec) + np.abs(eu))
    if case.vpred:
        x0, x0a = sa * lat - sb * e, abs(sa) * np.abs(lat) + abs(sb) * ea
    else:
        x0, x0a = (lat - sb * e) / sa, (np.abs(lat) + abs(sb) * ea) / abs(sa)
    prev, pa = c0 * x0 + cx * lat, abs(c0) * x0a + abs(cx) * np.abs(lat)
    if case.noise:
        prev, pa = prev + sigma * noise, pa + abs(sigma) * np.abs(noise)
    n0, n1 = cfg_roundings(case)
    return prev, gamma(n1) * pa, x0, gamma(n0) * x0a


def emulate_cfg(case: CfgCase, defect=None):
    """(new latents, x0) fp32 NCHW, one fp32 operation at a time (no contraction)."""
    sa, sb, c0, cx, sigma, g = case.coef
    eu, ec = _cfg_eps(case, F32, defect)
    _, lat, noise = cfg_inputs(case.shape)
    e = eu
    if case.cfg:
        e = eu + g * (ec - eu)

    def x0_of(x):
        return sa * x - sb * e if case.vpred or defect == "vpred_for_eps" else (x - sb * e) / sa
    x0 = x0_of(lat)
    prev = c0 * x0 + cx * lat
    if case.noise:
        prev = prev - sigma * noise if defect == "sigma_noise_subtracted" else prev + sigma * noise
    return prev.astype(F32), (x0_of(prev) if defect == "x0_after_update" else x0).astype(F32)


# ------------------------------------------------------------------------------------------------------------------------------------
# defects and the named case each must fail
# ------------------------------------------------------------------------------------------------------------------------------------
HARMLESS = ()
DEFECTS = ("conv_untransposed", "geglu_halves_swapped", "geglu_groups_32", "truncate", "cs_by_row", "lora_b_transposed", "lora_scale_dropped",
           "tile_order_swapped", "tile_pad_unzeroed", "u_unrounded", "v_row_r", "v_no_bias", "cond_uncond_swapped", "eps_nchw", "vpred_for_eps",
           "x0_after_update", "sigma_noise_subtracted", "u8_half_even", "clamp_left_out", "logvar_unclamped", "exp_full_logvar",
           "moment_halves_swapped", "vae_nchw_read", "pos_by_row", "transpose_copy")
_CFG16 = cfg_cases()[:16]
DEFECT_CASES = {
    "conv_untransposed": ("pack_conv", (3, 5, 9), "f16"),
    "geglu_halves_swapped": ("pack_matrix", (32, 3, 1), "bf16"),
    "geglu_groups_32": ("pack_scaled", (64, 64, 1), "f16"),
    "truncate": ("pack_matrix", (7, 37, 0), "bf16"),
    "cs_by_row": ("pack_scaled", (7, 37, 0), "f16"),
    "lora_b_transposed": ("lora", LoraCase((7, 37, 4), 0.5, False), "bf16"),
    "lora_scale_dropped": ("lora", LoraCase((33, 64, 16), -1.75, True), "f16"),
    "tile_order_swapped": ("tile", (17, 128)),
    "tile_pad_unzeroed": ("tile", (3, 128)),
    "u_unrounded": ("fold", FOLD_CASES[2], "bf16"),
    "v_row_r": ("fold", FOLD_CASES[4], "f16"),          # 96 rows: at 32 rows the interleave is the identity
    "v_no_bias": ("fold", FOLD_CASES[4], "bf16"),
    "cond_uncond_swapped": ("cfg", next(c for c in _CFG16 if c.cfg and c.g == 7.5)),
    "eps_nchw": ("cfg", next(c for c in _CFG16 if not c.cfg and not c.vpred)),
    "vpred_for_eps": ("cfg", next(c for c in _CFG16 if not c.vpred and c.x0)),
    "x0_after_update": ("cfg", next(c for c in _CFG16 if c.x0 and c.vpred)),
    "sigma_noise_subtracted": ("cfg", next(c for c in _CFG16 if c.noise and c.t == 999)),
    "u8_half_even": ("post", "sweep"),
    "clamp_left_out": ("post", "edge257"),
    "logvar_unclamped": ("vae", (2, 3, 5), True),
    "exp_full_logvar": ("vae", (3, 4, 80), True),
    "moment_halves_swapped": ("vae", (2, 3, 5), False),
    "vae_nchw_read": ("vae", (3, 4, 80), False),
    "pos_by_row": ("embed", (2, 3, 8, 5), "f16"),
    "transpose_copy": ("transpose", (2, 3, 5), "f32"),
}


def defect_fails(defect: str) -> bool:
    """True when `defect`, injected into the emulation of its named case, violates that case's criterion."""
    kind, *key = DEFECT_CASES[defect]
    if kind == "pack_conv":
        return not np.array_equal(emulate_pack_conv(*key, defect=defect), pack_conv_reference(*key))
    if kind == "pack_matrix":
        return not np.array_equal(emulate_pack_matrix(*key, defect=defect), pack_matrix_reference(*key))
    if kind == "pack_scaled":
        return not member(emulate_pack_scaled(*key, defect=defect), pack_scaled_exact(*key), key[1])[0]
    if kind == "lora":
        case, dt = key
        ref, bound = lora_reference(case, dt)
        return not check(from_bits(emulate_lora(case, dt, defect), dt).reshape(ref.shape), ref, bound)[0]
    if kind == "tile":
        return not np.array_equal(tile_reference(key[0], defect), tile_reference(key[0]))
    if kind == "fold":
        case, dt = key
        u, bu, v, bv = fold_reference(case, dt)
        eu, ev = emulate_fold(case, dt, defect)
        return not (check(eu, u, bu)[0] and check(ev, v, bv)[0])
    if kind == "cfg":
        prev, bp, x0, b0 = cfg_reference(key[0])
        ep, e0 = emulate_cfg(key[0], defect)
        return not (check(ep, prev, bp)[0] and (not key[0].x0 or check(e0, x0, b0)[0]))
    if kind == "post":
        v, u8 = post_reference(key[0])
        ev, eu8 = emulate_post(key[0], defect)
        return not (np.array_equal(ev.view(np.uint32), v.view(np.uint32)) and np.array_equal(eu8, u8))
    if kind == "vae":
        ref, bound, mean, lv = vae_reference(*key)
        z, m, l2 = emulate_vae(*key, defect=defect)
        return not (check(z, ref, bound)[0] and np.array_equal(m.view(np.uint32), mean.view(np.uint32)) and np.array_equal(l2.view(np.uint32), lv.view(np.uint32)))
    if kind == "embed":
        return not member(emulate_embed(*key, defect=defect), embed_exact(*key), key[1])[0]
    return not np.array_equal(transpose_reference(*key, defect=defect).view(np.uint32), transpose_reference(*key).view(np.uint32))
