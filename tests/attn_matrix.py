"""The idb_attention test matrix shared by test_attn_matrix_cpu.py (plan query, validation, emulation, teeth) and
test_attn_matrix_gpu.py (launch + compare): cases, input recipes, a float64 reference, a plain emulation of the kernel's arithmetic
contract, and the element-wise criteria.

Which kernel form (2-wave 64-row, 4-wave 128-row, 8-wave key-split, 12-wave 192-row key-split) a case runs is never derived here: a
case names the form it was chosen for (`waves`) and both test files ask idb_attention_plan whether that is what would launch.  The
cases on either side of each threshold of the plan function are found by threshold_cases(), a search over (batch, heads, n_q) with the
plan query.

Bound, element-wise, u = unit roundoff of the operand dtype (UNIT), ref = P V and absref = P |V| in float64 with P the exact softmax:

    |out - ref| <= C_O * u * |ref|                       the single rounding of the output to the operand dtype
                 + C_P * u * absref                      every p_j is rounded to the operand dtype (relative error <= u) before the second
                                                         MFMA while the denominator sums the unrounded p_j: sum_j |dp_j| |v_j| / l <= u * absref
                 + C_A * sqrt(n_kv) * 2^-24 * absref     fp32 exp2, the running sum and the MFMA accumulation over n_kv terms, each a
                                                         2^-24 relative error on a term of P |V| (random-sign growth, as gemm_matrix)
                 + f16 only: n_kv * 2^-25 * max|V| / l   f16 has subnormals below 2^-14 with spacing 2^-24: a rounded p_j there is off
                                                         by up to 2^-25 absolutely, n_kv of them, each times |v| <= max|V|, over the
                                                         denominator l (relative to the row max, so l >= 1)

C_O = C_P = C_A = 1.  The P term is a worst case and is not tightened by a statistical factor.  Recipes with structure have sharper
criteria: `count` (every p_j is exactly 1, every product exact) drops the P term, and an element whose bound is 0 must be exact;
`const_v` and `one_hot` have exactly known outputs and every element must equal them bit for bit.  No element is excluded anywhere.

With C = 1 the defect-free emulation reaches at most 0.992 (bf16) / 0.966 (f16) of its criterion over the whole case list, both on
`count`, whose criterion is the output rounding alone (half an ulp just above a power of two: C_O cannot go lower); on the full bound it
reaches 0.876 / 0.735 (`normal`), 0.493 / 0.463 (`peaked`), 0.812 / 0.496 (`wide_range`); the worst const_v deviation before the output
rounding is 0.092 u / 0.097 u against the 0.25 u limit (test_attn_matrix_cpu.py::test_emulation_meets_criteria prints all of these).
No constant had to be raised for the GPU; its figures are in test_attn_matrix_gpu.py's docstring.

What the old criterion (tensor-wide max-abs error <= 2^-7 (bf16) / 2^-9 (f16) * max(1, |ref|max), N(0,1) inputs, scale 1/8, 256
queries, seed 60) made of the defects in DEFECTS, on the emulation, at n_kv 77 / 545 / 1000 / 4096 (OLD_CRITERION_TABLE, regenerated
and compared by test_attn_matrix_cpu.py::test_teeth): it passed truncated P everywhere in both dtypes and, in bf16, one key too many
or too few at n_kv 4096; it failed everything else.  The new criteria fail every defect in both dtypes: `count` the index defects
(extra / missing key, skipped tiles, causal off by one, swapped halves, a one-wave merge), `one_hot` the running-max defects (missing
rescale of the accumulator or the denominator, a merge without max correction), `const_v` the truncation of P."""
import ctypes as C
import math
from dataclasses import dataclass, replace
from typing import Dict, List, Optional, Tuple

import torch

from faceposegenerator_amd import _lib as L
from matrix_common import check_t as check  # noqa: F401  (the torch verdict, re-exported to the two test files)

UNIT = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11}
TDT = {"bf16": torch.bfloat16, "f16": torch.float16}
IDB_DT = {"bf16": L.IDB_BF16, "f16": L.IDB_F16}
C_O = C_P = C_A = 1.0
CANARY = 0x7FC1          # int16 pattern the kernel must not overwrite outside its output; a NaN in bf16 and in f16
GUARD_ROWS = 2
PTR = 1 << 20            # any non-null 16-byte-aligned address: the host-side calls never dereference it

# recipes whose output is known exactly (criterion: bit-equal)
EXACT = ("const_v", "one_hot")

# the old criterion's verdict per defect on the emulation: "P" passes, "F" fails, at n_kv 77 / 545 / 1000 / 4096 -> (bf16, f16)
OLD_CRITERION_TABLE = {
    "extra_key": ("FFFP", "FFFF"),
    "missing_key": ("FFFP", "FFFF"),
    "causal_plus": ("FFFF", "FFFF"),
    "causal_minus": ("FFFF", "FFFF"),
    "p_trunc": ("PPPP", "PPPP"),
    "skip_first_tile": ("FFFF", "FFFF"),
    "skip_last_full_tile": ("FFFF", "FFFF"),
    "no_acc_rescale": ("FFFF", "FFFF"),
    "no_l_rescale": ("FFFF", "FFFF"),
    "swap_halves": ("FFFF", "FFFF"),
    "merge_one": ("FFFF", "FFFF"),
    "merge_no_max": ("FFFF", "FFFF"),
}


# ------------------------------------------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    name: str
    waves: int                       # the kernel form this case was chosen for (asserted through idb_attention_plan)
    batch: int
    heads: int
    n_q: int
    n_kv: int
    recipes: Tuple[str, ...] = ("normal", "count")
    n_kv_alloc: int = 0              # 0: n_kv
    layout: str = "kv"               # "qkv": one packed buffer; "kv": packed K|V, separate Q; "sep": separate Q, K, V
    pad: Tuple[int, int, int] = (0, 0, 0)     # extra elements per row of q / kv / out beyond the packed width
    scale: float = 0.125
    causal: bool = False
    poison: Optional[str] = None     # K/V rows n_kv .. n_kv_alloc-1: None zeros, "nan", "max" (largest finite value)

    @property
    def alloc(self) -> int:
        return self.n_kv_alloc or self.n_kv

    @property
    def c(self) -> int:
        return self.heads * 64

    def strides(self) -> Tuple[int, int, int]:
        c = self.c
        qw, kvw = (3 * c, 3 * c) if self.layout == "qkv" else (c, 2 * c) if self.layout == "kv" else (c, c)
        if self.layout == "qkv":
            return qw + self.pad[0], qw + self.pad[0], c + self.pad[2]
        return qw + self.pad[0], kvw + self.pad[1], c + self.pad[2]


def plan(lib, batch, heads, n_q, n_kv, causal) -> Tuple[int, Tuple[int, int, int, int]]:
    """(return code, (waves, key_split, rows, blocks)) of idb_attention_plan."""
    o = [C.c_int32(-1) for _ in range(4)]
    rc = lib.idb_attention_plan(batch, heads, n_q, n_kv, int(causal), *[C.byref(x) for x in o])
    return rc, tuple(x.value for x in o)


def case_plan(lib, case: Case):
    rc, p = plan(lib, case.batch, case.heads, case.n_q, case.n_kv, case.causal)
    assert rc == 0, (case.name, rc)
    return p


def _blocks(n_q, rows, heads, batch):
    return -(-n_q // rows) * heads * batch


# every threshold of the plan function: (name, which grid count, value below, value above, n_kv)
THRESHOLDS = [
    ("blocks128_127_128", 128, 127, 128, 77),           # 2-wave | 4-wave
    ("blocks128_127_128_long", 128, 127, 128, 520),     # 2-wave | 8-wave
    ("blocks128_256_257", 128, 256, 257, 520),          # 8-wave | 12-wave (where 192-row blocks fit one round)
    ("blocks128_511_512", 128, 511, 512, 520),          # key-split | 4-wave
    ("blocks192_256_257", 192, 256, 257, 520),          # 12-wave | 8-wave, with 257..511 blocks of 128 rows
]

_threshold_cache: Dict[int, List[Case]] = {}


def threshold_cases(lib) -> List[Case]:
    """For each threshold the cheapest (batch, heads, n_q) on each side of it, searched with the plan query: the two sides must report
    different forms, else the threshold is not where this list thinks it is (and the search fails loudly)."""
    key = id(lib)
    if key in _threshold_cache:
        return _threshold_cache[key]
    out: List[Case] = []
    for name, rows, lo, hi, n_kv in THRESHOLDS:
        side_forms = []
        for side, target in (("lo", lo), ("hi", hi)):
            best = None
            for batch in (1, 2):
                for heads in range(1, 520):
                    if target % (batch * heads):
                        continue
                    nblk = target // (batch * heads)
                    n_q = rows * nblk - (28 if nblk > 1 else rows - 100)
                    if _blocks(n_q, rows, heads, batch) != target:
                        continue
                    if rows == 192 and not 256 < _blocks(n_q, 128, heads, batch) < 512:
                        continue
                    rc, p = plan(lib, batch, heads, n_q, n_kv, 0)
                    if rc != 0:
                        continue
                    # on the 256 | 257 threshold of blocks128 the upper side must also fit 192-row blocks in one round
                    if name == "blocks128_256_257" and side == "hi" and _blocks(n_q, 192, heads, batch) > 256:
                        continue
                    cost = batch * heads * n_q
                    if best is None or cost < best[0]:
                        best = (cost, batch, heads, n_q, p)
            assert best is not None, f"no (batch, heads, n_q) reaches {name} {side}"
            _, batch, heads, n_q, p = best
            side_forms.append(p[0])
            out.append(Case(f"thr_{name}_{side}", p[0], batch, heads, n_q, n_kv, recipes=("normal", "count")))
        assert side_forms[0] != side_forms[1], f"threshold {name}: both sides run the {side_forms[0]}-wave form"
    # n_kv = 511 | 512 on a key-split-eligible grid (128 blocks of 128 rows)
    forms = []
    for n_kv in (511, 512):
        rc, p = plan(lib, 1, 128, 100, n_kv, 0)
        assert rc == 0
        forms.append(p[0])
        out.append(Case(f"thr_nkv_{n_kv}", p[0], 1, 128, 100, n_kv, recipes=("normal", "count")))
    assert forms[0] != forms[1], "threshold n_kv 511 | 512: both sides run the same form"
    _threshold_cache[key] = out
    return out


def _fixed_cases() -> List[Case]:
    cs: List[Case] = []
    tails = (1, 31, 32, 33, 63, 64, 65, 77, 127, 128, 129)
    # n_kv tails, 2-wave (2 heads x 70 queries: two 64-row workgroups per head, the second with 6 rows) and 4-wave (128 heads)
    for n in tails:
        cs.append(Case(f"w2_nkv{n}", 2, 1, 2, 70, n, recipes=("normal", "count", "one_hot")))
        cs.append(Case(f"w4_nkv{n}", 4, 1, 128, 40, n, recipes=("normal", "count", "one_hot")))
    # key-split forms: 1 / 31 / 32 / 33 / 63 keys in the last tile and an exact multiple of 64
    for n in (513, 543, 544, 545, 575, 576):
        cs.append(Case(f"w8_nkv{n}", 8, 1, 128, 100, n, recipes=("normal", "count", "one_hot", "const_v")))
        cs.append(Case(f"w12_nkv{n}", 12, 1, 129, 150, n, recipes=("normal", "count", "one_hot", "const_v")))
    # n_q edges: a last workgroup with whole waves beyond n_q, one query, fewer than 32 queries
    cs.append(Case("w2_nq65", 2, 1, 3, 65, 77))
    cs.append(Case("w2_nq1", 2, 2, 3, 1, 77))
    cs.append(Case("w2_nq17", 2, 1, 3, 17, 130, recipes=("normal", "count", "one_hot")))
    cs.append(Case("w4_nq1", 4, 1, 128, 1, 77))
    cs.append(Case("w4_nq17", 4, 2, 64, 17, 200))
    cs.append(Case("w4_nq300", 4, 1, 43, 300, 300, layout="qkv", recipes=("normal", "count", "one_hot")))
    cs.append(Case("w8_nq300", 8, 1, 43, 300, 600, recipes=("normal", "count", "const_v")))
    cs.append(Case("w12_nq1600", 12, 2, 11, 1600, 1600, layout="qkv", recipes=("normal", "count", "const_v")))
    cs.append(Case("w12_nq130", 12, 1, 129, 130, 640, recipes=("normal", "count", "one_hot")))
    # causal: every n around a tile and a workgroup edge in the 2-wave form; three query blocks per head in the 4-wave form
    for n in (1, 64, 65, 77, 128, 129):
        cs.append(Case(f"w2_causal{n}", 2, 1, 2, n, n, layout="qkv", causal=True, recipes=("normal", "count", "one_hot")))
    cs.append(Case("w4_causal300", 4, 1, 43, 300, 300, layout="qkv", causal=True, recipes=("normal", "count", "one_hot")))
    cs.append(Case("w4_causal129", 4, 1, 64, 129, 129, layout="qkv", causal=True))
    cs.append(Case("w4_causal600_long", 4, 1, 26, 600, 600, layout="qkv", causal=True))      # n_kv >= 512 and causal: not key-split
    # layouts: strides larger than the packed width and different from each other, n_kv_alloc > n_kv, poisoned padding rows
    cs.append(Case("w2_sep_pad", 2, 2, 3, 70, 77, n_kv_alloc=80, layout="sep", pad=(8, 24, 12)))
    cs.append(Case("w4_sep_pad", 4, 2, 64, 100, 77, n_kv_alloc=96, layout="sep", pad=(16, 8, 4)))
    cs.append(Case("w8_kv_pad", 8, 2, 64, 100, 545, n_kv_alloc=576, layout="kv", pad=(8, 16, 20), recipes=("normal", "count", "one_hot")))
    cs.append(Case("w12_sep_pad", 12, 1, 129, 150, 545, n_kv_alloc=547, layout="sep", pad=(24, 8, 12)))
    cs.append(Case("w2_qkv_pad", 2, 2, 3, 77, 77, layout="qkv", pad=(8, 0, 4)))
    for form, (b, h, nq, nkv) in {2: (2, 3, 70, 77), 4: (2, 64, 100, 65), 8: (2, 64, 100, 513), 12: (1, 129, 150, 575)}.items():
        for poison in ("nan", "max"):
            cs.append(Case(f"w{form}_poison_{poison}", form, b, h, nq, nkv, n_kv_alloc=nkv + 70, layout="kv", pad=(0, 8, 4), poison=poison,
                           recipes=("normal", "count", "one_hot")))
    # scale: peaked and near-uniform softmax; structured logits
    for form, (b, h, nq, nkv) in {2: (1, 3, 100, 200), 4: (1, 128, 100, 200), 8: (1, 128, 100, 600), 12: (1, 129, 150, 600)}.items():
        cs.append(Case(f"w{form}_scale2", form, b, h, nq, nkv, scale=2.0, recipes=("normal",)))
        cs.append(Case(f"w{form}_scale512th", form, b, h, nq, nkv, scale=1.0 / 512, recipes=("normal",)))
        cs.append(Case(f"w{form}_wide_range", form, b, h, nq, nkv, scale=1.0, recipes=("wide_range",)))
    cs.append(Case("w2_peaked512", 2, 1, 2, 512, 512, layout="qkv", recipes=("peaked",)))
    cs.append(Case("w8_peaked1024", 8, 2, 10, 1024, 1024, layout="qkv", recipes=("peaked", "one_hot")))
    # the real shapes: SD-2.1 self-attention at batch 1 and 2 (classifier-free guidance doubles it), cross-attention to 77, CLIP
    # (tokens, heads, batch) -> (self-attention form, cross-attention form)
    sd = {(4096, 5, 1): (8, 4), (1024, 10, 1): (2, 2), (256, 20, 1): (2, 2), (64, 20, 1): (2, 2),
          (4096, 5, 2): (12, 4), (1024, 10, 2): (8, 4), (256, 20, 2): (2, 2), (64, 20, 2): (2, 2)}
    for (n, h, b), (fs, fc) in sd.items():
        rec = ("normal", "count", "const_v") if n >= 512 else ("normal", "count")
        cs.append(Case(f"sd_self{n}_b{b}", fs, b, h, n, n, layout="qkv", recipes=rec))
        cs.append(Case(f"sd_cross{n}_b{b}", fc, b, h, n, 77))
    cs.append(Case("clip_causal77", 2, 1, 16, 77, 77, layout="qkv", causal=True))
    cs.append(Case("clip_causal77_b2", 2, 2, 16, 77, 77, layout="qkv", causal=True))
    return cs


def cases(lib) -> List[Case]:
    return _fixed_cases() + threshold_cases(lib)


# ------------------------------------------------------------------------------------------------------------------------------------
# input recipes (logical float64 tensors [batch][heads][n][64], already rounded to the operand dtype)
# ------------------------------------------------------------------------------------------------------------------------------------
@dataclass
class Inputs:
    q: torch.Tensor
    k: torch.Tensor                # [batch][heads][n_kv][64]: the attended keys only (padding rows are added by pack())
    v: torch.Tensor
    exact: Optional[torch.Tensor]  # the exactly known output of the EXACT recipes


def rnd(x: torch.Tensor, dtype: str) -> torch.Tensor:
    """float64 -> operand dtype (round to nearest even) -> float64."""
    return x.float().to(TDT[dtype]).double()


def trunc(x: torch.Tensor, dtype: str) -> torch.Tensor:
    """float64 >= 0 -> operand dtype rounded toward zero -> float64."""
    r = x.float().to(TDT[dtype])
    bits = r.view(torch.int16) - (r.double() > x).to(torch.int16)
    return bits.view(TDT[dtype]).double()


def _dominant_keys(case: Case) -> torch.Tensor:
    """The key that query i of one_hot is aligned with: the first rows walk the places where kernels go wrong (key 0, either 32-key
    half of the first tile, the first key of the second tile, the last tile's first key and both of its halves, the last valid key),
    the rest a fixed stride through all keys.  Causal: folded into 0..i."""
    n, t0 = case.n_kv, 64 * ((case.n_kv - 1) // 64)
    special = [x for x in (0, n - 1, 31, 32, 63, 64, t0, t0 + 31, t0 + 32, n - 2, t0 - 1, t0 - 33) if 0 <= x < n]
    i = torch.arange(case.n_q)
    idx = (i * 37 + 11) % n
    sp = torch.tensor(special)
    idx = torch.where(i % 3 == 0, sp[(i // 3) % len(special)], idx)
    if case.causal:
        idx = torch.where(idx <= i, idx, idx % (i + 1))
    return idx


def make_inputs(case: Case, recipe: str, dtype: str, seed: int = 60) -> Inputs:
    g = torch.Generator().manual_seed(seed)
    b, h, nq, nk = case.batch, case.heads, case.n_q, case.n_kv

    def randn(n):
        return rnd(torch.randn(b, h, n, 64, generator=g, dtype=torch.float32).double(), dtype)

    def randint(n, lo, hi):
        return torch.randint(lo, hi + 1, (b, h, n, 64), generator=g).double()

    exact = None
    if recipe == "normal":
        q, k, v = randn(nq), randn(nk), randn(nk)
    elif recipe == "count":
        q, k = torch.zeros(b, h, nq, 64, dtype=torch.float64), randn(nk)
        v = (torch.arange(nk)[:, None] % 64 == torch.arange(64)[None, :]).double().expand(b, h, nk, 64).contiguous()
    elif recipe == "const_v":
        assert nk >= 512, "const_v needs a long sweep (its margin is re-established per case by the CPU test)"
        q, k = randn(nq), randn(nk)
        cd = 2.0 ** ((torch.arange(64) % 8) - 4).double() * (1 - 2 * (torch.arange(64) // 8 % 2)).double()
        v = cd.expand(b, h, nk, 64).contiguous()
        exact = cd.expand(b, h, nq, 64).contiguous()
    elif recipe == "one_hot":
        # keys are +-1 vectors, query i is 64 x its dominant key: raw logit 4096 for that key and at most about 64 * 40 for any other
        # (all exact integers in fp32), so after scale 1/8 every other weight is below e^-190: zero in fp32, let alone bf16 / f16
        assert case.scale == 0.125
        k = randint(nk, 0, 1) * 2 - 1
        idx = _dominant_keys(case)
        q = 64.0 * k[:, :, idx, :]
        v = randint(nk, -8, 8)
        exact = v[:, :, idx, :].contiguous()
    elif recipe == "peaked":
        q, k, v = randn(nq), randn(nk), randn(nk)
        m = min(nq, nk)
        idx = torch.randperm(nk, generator=g)[:m]
        k[:, :, idx, :] = rnd(k[:, :, idx, :] + 3.0 * q[:, :, :m, :], dtype)
    elif recipe == "wide_range":
        # integer Q and K: raw logits are exact integers of a few hundred (so no fp32 score error hides behind the exponent), and
        # with scale 1 the exp2 arguments reach far below -126 while everything stays finite in fp32
        q, k, v = randint(nq, -6, 6), randint(nk, -6, 6), randn(nk)
    else:
        raise ValueError(recipe)
    return Inputs(q, k, v, exact)


# ------------------------------------------------------------------------------------------------------------------------------------
# float64 reference and the emulation of the kernel's arithmetic contract
# ------------------------------------------------------------------------------------------------------------------------------------
@dataclass
class Ref:
    ref: torch.Tensor        # P V
    absref: torch.Tensor     # P |V|
    l: torch.Tensor          # softmax denominator relative to the row max (>= 1), [..., n_q, 1]
    vmax: float


def _scores(q, k, n_kv, scale, causal, q_pos=None):
    s = (q @ k[..., :n_kv, :].transpose(-1, -2)) * scale
    if causal:
        pos = torch.arange(q.shape[-2], device=q.device) if q_pos is None else q_pos
        s = s.masked_fill(torch.arange(n_kv, device=q.device)[None, :] > pos[:, None], -math.inf)
    return s


def reference(q, k, v, n_kv, scale, causal, q_pos=None) -> Ref:
    """float64 softmax(q k^T * scale) v over the first n_kv keys (causal: query i, or q_pos[i], attends keys 0..i)."""
    s = _scores(q.double(), k.double(), n_kv, scale, causal, q_pos)
    p = torch.exp(s - s.amax(-1, keepdim=True))
    del s
    l = p.sum(-1, keepdim=True)
    vv = v[..., :n_kv, :].double()
    return Ref((p @ vv) / l, (p @ vv.abs()) / l, l, vv.abs().max().item())


DIRECT_DEFECTS = ("extra_key", "missing_key", "causal_plus", "causal_minus", "p_trunc")
TILED_DEFECTS = ("skip_first_tile", "skip_last_full_tile", "no_acc_rescale", "no_l_rescale", "swap_halves")
SPLIT_DEFECTS = ("merge_one", "merge_no_max")
DEFECTS = DIRECT_DEFECTS + TILED_DEFECTS + SPLIT_DEFECTS


def emulate(q, k, v, n_kv, scale, causal, dtype, defect=None, tiled=False, split=False, q_pos=None):
    """The kernel's arithmetic contract, plainly: scores in float64, p = exp(s - rowmax), P rounded to nearest even to the operand dtype
    for the numerator and unrounded for the denominator, one division, one rounding of the output.  tiled=True sweeps 64-key tiles with
    a running max and sum (split=True: the lower and upper 32 keys of every tile in two independent sweeps merged at the end, as the
    key-split forms do); it exists to host the TILED_DEFECTS / SPLIT_DEFECTS.  Only ever compared with the float64 reference."""
    assert defect is None or defect in DEFECTS
    if tiled or split or defect in TILED_DEFECTS + SPLIT_DEFECTS:
        return _emulate_tiled(q, k, v, n_kv, scale, causal, dtype, defect, split or defect in SPLIT_DEFECTS, q_pos)
    kk, vv = k[..., :n_kv, :], v[..., :n_kv, :]
    if defect == "extra_key":          # a missed tail mask reads, after the clamp, a copy of key n_kv - 1
        kk, vv = torch.cat([kk, kk[..., -1:, :]], -2), torch.cat([vv, vv[..., -1:, :]], -2)
    elif defect == "missing_key":
        kk, vv = kk[..., :-1, :], vv[..., :-1, :]
    pos = torch.arange(q.shape[-2]) if q_pos is None else q_pos
    if defect == "causal_plus":
        pos = pos + 1
    elif defect == "causal_minus":
        pos = (pos - 1).clamp(min=0)
    s = _scores(q, kk, kk.shape[-2], scale, causal, pos)
    p = torch.exp(s - s.amax(-1, keepdim=True))
    pr = trunc(p, dtype) if defect == "p_trunc" else rnd(p, dtype)
    return rnd((pr @ vv) / p.sum(-1, keepdim=True), dtype)


def _emulate_tiled(q, k, v, n_kv, scale, causal, dtype, defect, split, q_pos):
    s_all = _scores(q, k, n_kv, scale, causal, q_pos)
    nt = -(-n_kv // 64)
    parts = []
    for half in ((0, 1) if split else (0,)):
        m = torch.full(s_all.shape[:-1] + (1,), -math.inf, dtype=torch.float64)
        l = torch.zeros_like(m)
        acc = torch.zeros(s_all.shape[:-1] + (64,), dtype=torch.float64)
        for t in range(nt):
            if defect == "skip_first_tile" and t == 0 and nt > 1:
                continue
            if defect == "skip_last_full_tile" and t == n_kv // 64 - 1:
                continue
            lo = t * 64 + 32 * half
            hi = min(lo + (32 if split else 64), n_kv)
            if lo >= hi:
                continue
            s = s_all[..., lo:hi]
            m_new = torch.maximum(m, s.amax(-1, keepdim=True))
            alpha = torch.where(m == -math.inf, torch.zeros_like(m), torch.exp(m - m_new))
            p = torch.nan_to_num(torch.exp(s - m_new), nan=0.0)          # a row with nothing attended yet: all weights 0
            idx = torch.arange(lo, hi)
            if defect == "swap_halves":
                idx = (((idx - t * 64) ^ 32) + t * 64).clamp(max=n_kv - 1)
            l = l * (1.0 if defect == "no_l_rescale" else alpha) + p.sum(-1, keepdim=True)
            acc = acc * (1.0 if defect == "no_acc_rescale" else alpha) + rnd(p, dtype) @ v[..., idx, :]
            m = m_new
        parts.append((m, l, acc))
    if defect == "merge_one":
        parts = parts[:1]
    m = parts[0][0] if len(parts) == 1 else torch.maximum(parts[0][0], parts[1][0])
    l_tot, acc_tot = 0.0, 0.0
    for mi, li, ai in parts:
        w = torch.where(mi == -math.inf, torch.zeros_like(mi), torch.ones_like(mi) if defect == "merge_no_max" else torch.exp(mi - m))
        l_tot, acc_tot = l_tot + li * w, acc_tot + ai * w
    return rnd(acc_tot / l_tot, dtype)


# ------------------------------------------------------------------------------------------------------------------------------------
# criteria
# ------------------------------------------------------------------------------------------------------------------------------------
def bound(r: Ref, n_kv: int, dtype: str, recipe: str) -> torch.Tensor:
    u = UNIT[dtype]
    if recipe in EXACT:
        return torch.zeros_like(r.ref)
    b = C_O * u * r.ref.abs() + C_A * math.sqrt(n_kv) * 2.0 ** -24 * r.absref
    if recipe == "count":
        return b
    b = b + C_P * u * r.absref
    if dtype == "f16":
        b = b + n_kv * 2.0 ** -25 * r.vmax / r.l
    return b


def expected(inp: Inputs, r: Ref, recipe: str) -> torch.Tensor:
    return inp.exact.to(r.ref.device) if recipe in EXACT else r.ref


def old_criterion(out: torch.Tensor, ref: torch.Tensor, dtype: str) -> Tuple[bool, float, float]:
    """The criterion of test_self_attention / test_cross_attention / test_causal_attention."""
    tol = (2.0 ** -7 if dtype == "bf16" else 2.0 ** -9) * max(1.0, ref.abs().max().item())
    err = (out.double() - ref).abs().max().item()
    return err <= tol, err, tol


# ------------------------------------------------------------------------------------------------------------------------------------
# packing into the C ABI's layouts (GPU file; also usable on the CPU)
# ------------------------------------------------------------------------------------------------------------------------------------
@dataclass
class Packed:
    bufs: list                      # keeps the allocations alive
    q_ptr: int
    k_ptr: int
    v_ptr: int
    out_ptr: int
    obuf: torch.Tensor              # int16 view [GUARD_ROWS + batch*n_q + GUARD_ROWS][out_ld]
    q_ld: int
    kv_ld: int
    out_ld: int


def _rows(x: torch.Tensor) -> torch.Tensor:
    b, h, n, d = x.shape
    return x.permute(0, 2, 1, 3).reshape(b, n, h * d)


def pack(case: Case, inp: Inputs, dtype: str, device) -> Packed:
    """Every element the ABI does not hand to the kernel as Q, K or V data (row padding beyond the packed width) is NaN; K/V rows
    n_kv .. n_kv_alloc-1 hold zeros, NaN or the largest finite value (case.poison); `out` is all CANARY with guard rows around it."""
    t = TDT[dtype]
    b, c, nq, na = case.batch, case.c, case.n_q, case.alloc
    q_ld, kv_ld, out_ld = case.strides()
    fill = {None: 0.0, "nan": math.nan, "max": torch.finfo(t).max}[case.poison]

    def kv_rows(x):
        full = torch.full((b, na, c), fill, dtype=torch.float64)
        full[:, :case.n_kv] = _rows(x)
        return full.to(t)

    q, k, v = _rows(inp.q).to(t), kv_rows(inp.k), kv_rows(inp.v)
    es = 2
    if case.layout == "qkv":
        assert nq == case.n_kv == na
        buf = torch.full((b * nq, q_ld), math.nan, dtype=t)
        buf[:, :c], buf[:, c:2 * c], buf[:, 2 * c:3 * c] = q.reshape(-1, c), k.reshape(-1, c), v.reshape(-1, c)
        bufs = [buf.to(device)]
        p = bufs[0].data_ptr()
        ptrs = (p, p + c * es, p + 2 * c * es)
    elif case.layout == "kv":
        qb = torch.full((b * nq, q_ld), math.nan, dtype=t)
        qb[:, :c] = q.reshape(-1, c)
        kvb = torch.full((b * na, kv_ld), math.nan, dtype=t)
        kvb[:, :c], kvb[:, c:2 * c] = k.reshape(-1, c), v.reshape(-1, c)
        bufs = [qb.to(device), kvb.to(device)]
        ptrs = (bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[1].data_ptr() + c * es)
    else:
        qb = torch.full((b * nq, q_ld), math.nan, dtype=t)
        qb[:, :c] = q.reshape(-1, c)
        kb, vb = torch.full((b * na, kv_ld), math.nan, dtype=t), torch.full((b * na, kv_ld), math.nan, dtype=t)
        kb[:, :c], vb[:, :c] = k.reshape(-1, c), v.reshape(-1, c)
        bufs = [qb.to(device), kb.to(device), vb.to(device)]
        ptrs = tuple(x.data_ptr() for x in bufs)
    obuf = torch.full((2 * GUARD_ROWS + b * nq, out_ld), CANARY, dtype=torch.int16, device=device)
    bufs.append(obuf)
    return Packed(bufs, ptrs[0], ptrs[1], ptrs[2], obuf.data_ptr() + GUARD_ROWS * out_ld * es, obuf, q_ld, kv_ld, out_ld)


def launch(lib, case: Case, pk: Packed, dtype: str, stream) -> int:
    return lib.idb_attention(pk.q_ptr, pk.q_ld, pk.k_ptr, pk.v_ptr, pk.kv_ld, pk.out_ptr, pk.out_ld, case.batch, case.heads, case.n_q,
                             case.n_kv, case.alloc, case.scale, int(case.causal), IDB_DT[dtype], stream)


def unpack_out(case: Case, pk: Packed, dtype: str) -> Tuple[torch.Tensor, int]:
    """(out as [batch][heads][n_q][64] in the operand dtype, number of elements outside the ABI's output that lost the canary)."""
    b, nq, c = case.batch, case.n_q, case.c
    owned = torch.zeros_like(pk.obuf, dtype=torch.bool)
    owned[GUARD_ROWS:GUARD_ROWS + b * nq, :c] = True
    touched = int(((pk.obuf != CANARY) & ~owned).sum())
    out = pk.obuf[GUARD_ROWS:GUARD_ROWS + b * nq, :c].contiguous().view(TDT[dtype])
    return out.view(b, nq, case.heads, 64).permute(0, 2, 1, 3), touched


def with_layout(case: Case, **kw) -> Case:
    return replace(case, **kw)
