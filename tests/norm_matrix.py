"""The idb_groupnorm / idb_groupnorm_fp8 / idb_groupnorm_stats / idb_layernorm / idb_softmax_rows test matrix shared by
test_norm_matrix_cpu.py (plan query, validation, emulation, teeth) and test_norm_matrix_gpu.py (launch + compare): cases, input recipes,
float64 references, a plain emulation of the kernels' arithmetic contract with injectable defects, and the element-wise criteria.

Which form (0 two launches, 1 single launch with hand-off, 2 normalise only from partials_in) and which geometry (slice width, pixel
chunks, rows per pass) a GroupNorm case runs is never derived here for a launch: a case names what it was chosen for (GN_TABLE) and both
test files ask idb_groupnorm_plan; py_plan() is the pure-Python statement of the same rules, compared with the query case by case.
IDB_GN_ALIGN is a process-wide static of the library: the matrix assumes its default (16 Mi elements) and reaches the aligned geometry
with tensors of that size.

Reference: float64 from the operand-dtype-rounded inputs: two-pass population variance, 1 / sqrt(var + eps) with eps the fp32 value the
ABI receives, affine, SiLU as x / (1 + exp(-x)).  fp8: e4m3 round-to-nearest-even of clamp(y * inv_scale, -448, 448).

GroupNorm criterion, element-wise, nothing excluded.  u = unit roundoff of the output (UNIT), z = pre-activation, out = act(z),
r = 1 / sqrt(var + eps), g = gamma, e = 2^-24, S1 = mean |x| and S2 = mean x^2 over the group, L = sup |SiLU'| = 1.0998 (at x = 2.3994;
L_SILU = 1.1; 1 without SiLU), d = the longest chain of fp32 additions an addend passes through (gn_depth: pixels per thread + the 8
channel fold + threads per lane + 6 shuffle stages + chunks per lane + 3 shuffle stages + 1 for the rounding of x*x):

    |got - ref| <= u |ref|                                                    the one output rounding
                 + L e (4 |x| r|g| + 6 |mu| r|g| + 2 |beta|)                  fp32 x*ks + kh.  The constants are derived, not 1: |x| r|g| sees
                                                                              the roundings of rstd, of ks = rstd*gamma, of x*ks and of the final
                                                                              add; |mu| r|g| those of mean, rstd, ks, mean*ks, beta - mean*ks and
                                                                              the final add; |beta| the last two (fewer when the compiler fuses)
                 + L r|g| d e S1                                              error of the mean
                 + L |x - mu| r|g| (1/2) d e (S2 + 2 |mu| S1) / (var + eps)   error of rstd: the variance is one-pass, E[x^2] - mean^2
                 + 7 e |ref|   (SiLU only)                                    v_exp_f32 and v_rcp_f32 are 1 ulp = 2 e each; the argument -z log2(e)
                                                                              is rounded (relative error of exp <= |z| e, weighted by 1 - sigmoid:
                                                                              <= 0.28 e); 1 + exp and the product round once each: <= 6.3 e
                 + 2^-25       (f16 only)                                     f16 results below 2^-14 are spaced 2^-24 apart

`count` (x in {0, 1, 2}) and `constant_group` (every group constant: var is exactly 0, eps decides) have exact sums in fp32: the two
statistics lines are dropped, and the partial sums must equal the integers bit for bit.  LayerNorm: the same with the exact two-pass
variance, i.e. the rstd line is |x - mu| r|g| (1/2) (d + 3) e with no S2 / (var + eps) amplification (d = 24 serial + 6 shuffle stages; 3:
the rounding of the mean enters (x - mean)^2 only to second order, the division, the rsqrt), the mean line carries d + 1 (its division
is fp32), the affine line is L = 1.  Softmax: u ref + e (|x - max| + d + 6) ref + f16's 2^-25 (d = 8 cols / 2048 serial + 6 + 3; 6: v_exp 2,
the subtraction's rounding is 0 (operands are 16-bit), 1 / sum 1.5, the product 0.5, rounding of the exp argument scaled by log2(e) is the
|x - max| term).  Statistics partials: |got - want| <= d e sum |addend|.  fp8: the byte must be the e4m3 rounding of some value inside
the interval the float criterion (without its first line, plus e |ref| for the scaling product) allows.

Worst err / criterion of the defect-free emulation over the case list, bf16 / f16 (test_norm_matrix_cpu.py prints them): GroupNorm
normal 0.995 / 0.994, offset 0.985 / 0.934, mixed_scale 0.995 / 0.992, constant_group 0.987 / 0.980, constant_offset 0.043 / 0.029, tiny_var
0.996 / 0.996, count 0.994 / 0.995, ramp 0.995 / 0.991, outlier 0.996 / 0.996; LayerNorm 0.995 .. 0.997 on every recipe; softmax normal 0.995 /
1.000, peaked 0.992 / 0.000 (f16: every off-peak output underflows to 0 inside the 2^-25 term), constant_row 0.500 / 0.484, shifted 0.993 /
1.000.  Nearly all of these are the output rounding (half an ulp just above a power of two); the statistics partials reach 0.13 of theirs.
No constant had to be raised for the emulation or for the GPU (test_norm_matrix_gpu.py's docstring has its figures).

What today's criterion (`_check(out, ref, _tol(eng))` of tests/test_kernels_gpu.py: tensor-wide max |err| <= 2^-7 (bf16) / 2^-9 (f16) *
max(1, max |ref|), on its own N(0,1)-like inputs) makes of every defect of the emulation is OLD_CRITERION_TABLE, regenerated and compared by
test_norm_matrix_cpu.py::test_teeth: it passes a missing eps, an unclamped variance, a one-pass LayerNorm variance and a softmax without max
subtraction everywhere, and on some shapes a lost group slot, x1 read with C0's stride, idle thread rows included, the count taken from
full chunks, a stale partial, partials_in indexed with the wrong chunk count, the neighbouring slice's gamma / beta and even a skipped SiLU.
The new criteria fail every defect in both dtypes: `count` the index defects, `constant_group` / `constant_offset` the eps and clamp
defects, `offset` the one-pass LayerNorm, `shifted` the softmax without max subtraction."""
import ctypes as C
import math
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import torch

from faceposegenerator_amd import _lib as L
from matrix_common import check_t as check  # noqa: F401  (the torch verdict, re-exported to the two test files)

UNIT = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11}
TDT = {"bf16": torch.bfloat16, "f16": torch.float16}
IDB_DT = {"bf16": L.IDB_BF16, "f16": L.IDB_F16}
F8 = torch.float8_e4m3fn
E24 = 2.0 ** -24
L_SILU = 1.1
SILU_EVAL = 7.0
CANARY = 0x7FC1          # int16 pattern the kernels must not overwrite outside their output; a NaN in bf16 and in f16
CANARY8 = 0x7F           # e4m3 NaN
GUARD_ROWS = 2
PTR = 1 << 20            # any non-null 16-byte-aligned address: the host-side calls never dereference it
SYNC_LEN = 4096          # the counter array the engine owns
GN_THREADS, GN_MAXCHUNKS, GN_SYNC_MAXIT, GN_SYNC_MAXBLOCKS, GN_ALIGN = 256, 64, 4, 1024, 16 << 20

EXACT_SUMS = ("count", "constant_group")
GN_RECIPES = ("normal", "offset", "mixed_scale", "constant_group", "constant_offset", "tiny_var", "count", "ramp", "outlier")
BIG_RECIPES = ("normal", "count")
LN_RECIPES = ("normal", "offset", "constant_row", "count", "outlier")
SM_RECIPES = ("normal", "peaked", "constant_row", "shifted")

# today's criterion per defect on `normal` inputs, (bf16, f16): P passes, F fails, - not applicable; GroupNorm on u1280p640_hw100 / u640_hw1024 /
# cpg2_hw256 / u320_hw4096, LayerNorm on 77x640 / 513x1280 / 64x64, softmax on 30x4096 (test_norm_matrix_cpu.py::test_teeth regenerates it)
OLD_CRITERION_TABLE = {
    "tail_twice": ("FFFF", "FFFF"),
    "group_off_by_one": ("FFFF", "FFFF"),
    "last_slot_lost": ("PPFP", "PPFP"),
    "x1_stride": ("FPPP", "FPPP"),
    "inactive_rows": ("PFPF", "FFPF"),
    "last_chunk_dropped": ("FFFF", "FFFF"),
    "cnt_full_chunks": ("FPPP", "FFPP"),
    "no_eps": ("PPPP", "PPPP"),
    "no_clamp": ("PPPP", "PPPP"),
    "stale_partial": ("FPFP", "FFFP"),
    "apply_wrong_chunks": ("-FPP", "-FPP"),
    "neighbour_gamma": ("FFPF", "FFPF"),
    "silu_skipped": ("FPFF", "FPFF"),
    "fp8_no_saturation": ("----", "----"),
    "fp8_double_rounding": ("----", "----"),
    "ln_padded_count": ("FFF", "FFF"),
    "ln_one_pass": ("PPP", "PPP"),
    "sm_no_max": ("P", "P"),
    "sm_three_waves": ("F", "F"),
}


# ------------------------------------------------------------------------------------------------------------------------------------
# the plan: query and pure-Python statement
# ------------------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Plan:
    form: int
    sw: int            # slice_channels
    slices: int
    chunks: int
    chunk_len: int
    pr: int            # rows_per_pass
    apply_blocks: int

    @property
    def cols(self):
        return self.sw // 8


def plan(lib, c0, c1, batch, hw, groups, sync_len=0, pchunks=0) -> Tuple[int, Plan]:
    o = [C.c_int32(-1) for _ in range(7)]
    rc = lib.idb_groupnorm_plan(c0, c1, batch, hw, groups, sync_len, pchunks, *[C.byref(x) for x in o])
    return rc, Plan(*[x.value for x in o])


def _ceil(a, b):
    return -(-a // b)


def py_plan(c0, c1, batch, hw, groups, sync_len=0, pchunks=0) -> Plan:
    """The geometry and form rules of idb_norm.hip, restated: a threshold edit there shows up as a difference here."""
    c = c0 + c1
    cpg = c // groups
    sw = math.lcm(cpg, 8)
    while sw // 8 < 8 and c % (sw * 2) == 0:
        sw *= 2
    sa = math.lcm(cpg, 64)
    if batch * hw * c >= GN_ALIGN and c0 % 64 == 0 and c1 % 64 == 0 and c % sa == 0 and sa // 8 <= GN_THREADS and sa // cpg <= 64:
        sw = sa
    pr, slices = GN_THREADS // (sw // 8), c // sw
    chunks = max(1, min(_ceil(1024, batch * slices), _ceil(hw, 2 * pr), GN_MAXCHUNKS))
    ppb = max(_ceil(hw, _ceil(2048, batch * slices)), 2 * pr)
    blocks = _ceil(hw, ppb)
    if pchunks:
        return Plan(2, sw, slices, pchunks, 64, pr, blocks)
    fch = _ceil(hw, GN_SYNC_MAXIT * pr)
    if sync_len > 0 and fch <= GN_MAXCHUNKS and fch * slices * batch <= GN_SYNC_MAXBLOCKS and 2 * batch * slices <= sync_len:
        return Plan(1, sw, slices, fch, _ceil(hw, fch), pr, 0)
    return Plan(0, sw, slices, chunks, _ceil(hw, chunks), pr, blocks)


def gn_depth(p: Plan) -> int:
    """Longest chain of fp32 additions in the statistics of this plan (see the module docstring)."""
    return _ceil(p.chunk_len, p.pr) + 8 + _ceil(p.cols * p.pr, 64) + 6 + _ceil(p.chunks, 8) + 3 + 1


# ------------------------------------------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class GnCase:
    name: str
    c0: int
    c1: int
    batch: int
    hw: int
    groups: int
    sw: int                 # slice width the case was chosen for
    chunks: int             # pixel chunks of the two-launch form
    single: bool            # eligible for the single-launch form with SYNC_LEN counters
    silu: bool = True
    eps: float = 1e-5
    recipes: Tuple[str, ...] = GN_RECIPES
    fp8: bool = False

    @property
    def c(self):
        return self.c0 + self.c1

    @property
    def cpg(self):
        return self.c // self.groups

    @property
    def big(self):
        return self.batch * self.hw * self.c >= 1 << 23

    @property
    def cpu_recipes(self):
        """What the CPU emulation runs: the full list, except on tensors of >= 8 Mi elements and on the threshold cases, where the serial
        fp32 emulation of every recipe would take the CPU test from one minute to many (the device test launches every recipe on them)."""
        return BIG_RECIPES if self.big or self.name.startswith("thr_") else self.recipes

    @property
    def pin_ok(self):
        return self.c1 == 0 and self.hw % 64 == 0 and self.hw // 64 <= GN_MAXCHUNKS


# name, c0, c1, batch, hw, groups, slice width, chunks (two-launch), single-launch eligible, silu, eps, fp8
GN_TABLE = [
    # the UNet's channel families; 320+640, 640+320, 1280+640 and 640+1280 have 120-channel slices that straddle the x0 | x1 boundary,
    # 320+320 and 1280+1280 do not; cpg 10, 20, 30, 60 do not divide the 8-channel vector
    ("u320_hw4096", 320, 0, 2, 4096, 32, 80, 64, True, True, 1e-5, True),
    ("u640_hw1024", 640, 0, 2, 1024, 32, 80, 21, True, False, 1e-5, False),
    ("u1280_hw256", 1280, 0, 2, 256, 32, 80, 6, True, True, 1e-6, True),
    ("u320p320_hw2304", 320, 320, 2, 2304, 32, 80, 47, True, True, 1e-5, False),
    ("u640p320_hw1024", 640, 320, 2, 1024, 32, 120, 31, True, True, 1e-5, False),
    ("u320p640_hw576", 320, 640, 1, 576, 32, 120, 17, True, True, 1e-6, True),
    ("u1280p640_hw256", 1280, 640, 2, 256, 32, 120, 8, True, False, 1e-5, False),
    ("u640p1280_hw144", 640, 1280, 1, 144, 32, 120, 5, True, True, 1e-5, False),
    ("u1280p1280_hw64", 1280, 1280, 2, 64, 32, 80, 2, True, True, 1e-5, True),
    ("u1280_hw16", 1280, 0, 1, 16, 32, 80, 1, True, True, 1e-5, False),
    ("u1280_hw1", 1280, 0, 3, 1, 32, 80, 1, True, True, 1e-5, False),
    ("u640_hw4", 640, 0, 2, 4, 32, 80, 1, True, False, 1e-6, False),
    ("u320_hw63", 320, 0, 2, 63, 32, 80, 2, True, True, 1e-5, False),
    ("u320_hw65", 320, 0, 1, 65, 32, 80, 2, True, True, 1e-5, False),
    ("u1280p640_hw100", 1280, 640, 2, 100, 32, 120, 3, True, True, 1e-5, False),
    ("u320_hw1600", 320, 0, 2, 1600, 32, 80, 32, True, True, 1e-5, False),
    ("empty_chunk_hw3201", 320, 0, 1, 3201, 32, 80, 64, True, True, 1e-5, False),      # 64 chunks of 51 pixels: the last one starts beyond hw
    ("u320_hw9216", 320, 0, 1, 9216, 32, 80, 64, False, True, 1e-5, False),
    # the VAE's; hw 262144 at batch 1 is the last decoder stage (32 Mi elements: the aligned rule applies and gives the same 64)
    ("v128_hw4096", 128, 0, 1, 4096, 32, 64, 64, True, True, 1e-6, True),
    ("v256_hw9216", 256, 0, 1, 9216, 32, 64, 64, False, True, 1e-6, False),
    ("v512_hw1024", 512, 0, 1, 1024, 32, 64, 16, True, True, 1e-6, False),
    ("v512_hw4096", 512, 0, 2, 4096, 32, 64, 64, True, False, 1e-6, False),
    ("v128_hw262144", 128, 0, 1, 262144, 32, 64, 64, False, True, 1e-6, False),
    # group widths: cpg 2 and 3 (four groups per 8-channel vector), 5, 64 with 8 groups and with 1, groups = C / 2
    ("cpg2_hw256", 64, 0, 2, 256, 32, 64, 4, True, True, 1e-5, True),
    ("cpg3_hw100", 96, 0, 3, 100, 32, 96, 3, True, True, 1e-5, False),
    ("cpg5_hw65", 160, 0, 2, 65, 32, 80, 2, True, False, 1e-5, False),
    ("cpg64_g8_hw64", 512, 0, 1, 64, 8, 64, 1, True, True, 1e-5, False),
    ("cpg64_g1_hw16", 64, 0, 2, 16, 1, 64, 1, True, True, 1e-6, False),
    ("half_groups_hw144", 128, 0, 2, 144, 64, 64, 3, True, True, 1e-5, False),
    ("c0_lt_c1_cpg2", 24, 40, 2, 64, 32, 64, 1, True, True, 1e-5, False),
    # >= 16 Mi elements: slices of lcm(cpg, 64) channels (40 or 120 vector columns: 240 of 256 threads), and the twin just below
    ("big_cpg10", 320, 0, 52, 1024, 32, 320, 20, False, True, 1e-5, True),
    ("twin_cpg10", 320, 0, 51, 1024, 32, 80, 6, False, True, 1e-5, True),
    ("big_cpg20", 320, 320, 103, 256, 32, 320, 5, False, True, 1e-5, False),
    ("twin_cpg20", 320, 320, 102, 256, 32, 80, 2, False, True, 1e-5, False),
    ("big_cpg30", 640, 320, 69, 256, 32, 960, 15, False, True, 1e-5, False),
    ("twin_cpg30", 640, 320, 68, 256, 32, 120, 2, False, True, 1e-5, False),
    ("big_cpg40", 1280, 0, 205, 64, 32, 320, 2, False, False, 1e-5, False),
    ("twin_cpg40", 1280, 0, 204, 64, 32, 80, 1, False, False, 1e-5, False),
    ("big_cpg60", 1280, 640, 137, 64, 32, 960, 4, False, True, 1e-5, False),
    ("twin_cpg60", 1280, 640, 136, 64, 32, 120, 1, False, True, 1e-5, False),
    ("big_cpg80", 1280, 1280, 103, 64, 32, 320, 2, False, True, 1e-5, False),
    ("twin_cpg80", 1280, 1280, 102, 64, 32, 80, 1, False, True, 1e-5, False),
    ("big_empty_chunk", 640, 320, 32, 550, 32, 960, 32, False, True, 1e-5, False),      # 32 chunks of 18 pixels, 2 rows per pass: the last is empty
    ("big_cpg8", 256, 0, 1, 65536, 32, 64, 64, False, True, 1e-6, False),
    ("twin_cpg8", 256, 0, 1, 65535, 32, 64, 64, False, True, 1e-6, False),
    ("big_cpg16", 512, 0, 1, 32768, 32, 64, 64, False, True, 1e-6, False),
    ("twin_cpg16", 512, 0, 1, 32767, 32, 64, 64, False, True, 1e-6, False),
    ("twin_cpg4", 128, 0, 1, 131071, 32, 64, 64, False, True, 1e-6, False),
]


def _fixed_gn_cases() -> List[GnCase]:
    out = []
    for name, c0, c1, b, hw, g, sw, ch, single, silu, eps, fp8 in GN_TABLE:
        out.append(GnCase(name, c0, c1, b, hw, g, sw, ch, single, silu, eps, GN_RECIPES, fp8))
    return out


_thr_cache: Dict[int, List[GnCase]] = {}


def threshold_cases(lib) -> List[GnCase]:
    """A case on each side of each eligibility limit of the single-launch form, found with the query (C = 320, 80-channel slices, 25
    rows per pass, so the hand-off form takes ceil(hw / 100) chunks): 64 chunks (batch 1: hw 6400 | 6401), 1024 workgroups (batch 8:
    32 chunks x 4 slices x 8 | 33 x 4 x 8).  The sync_len limit (2 * batch * slices counters | one fewer) changes no tensor and is asserted
    through the query alone by test_norm_matrix_cpu.py.  The fourth condition of the host code, at most 4 passes per chunk, cannot fail
    on its own: chunks = ceil(hw / (4 * rows_per_pass)) makes chunk_len <= 4 * rows_per_pass; a search over hw 1..20000 and the slice
    widths 40, 64, 80, 96, 120 found no shape where it alone decides."""
    key = id(lib)
    if key in _thr_cache:
        return _thr_cache[key]
    out = []
    for name, batch in (("thr_chunks64", 1), ("thr_blocks1024", 8)):
        found = None
        for hw in range(64, 8000):
            rc_a, a = plan(lib, 320, 0, batch, hw, 32, SYNC_LEN)
            rc_b, b = plan(lib, 320, 0, batch, hw + 1, 32, SYNC_LEN)
            assert rc_a == 0 and rc_b == 0
            if a.form == 1 and b.form == 0:
                found = (hw, a, b)
                break
        assert found, f"{name}: no hw where the single-launch form stops being eligible"
        hw, a, b = found
        for side, h, p in (("lo", hw, a), ("hi", hw + 1, b)):
            p0 = plan(lib, 320, 0, batch, h, 32)[1]
            out.append(GnCase(f"{name}_{side}", 320, 0, batch, h, 32, p0.sw, p0.chunks, side == "lo", True, 1e-5, GN_RECIPES))
    _thr_cache[key] = out
    return out


# cases whose two-launch geometry already has hw / 64 chunks of 64 pixels: there idb_groupnorm_stats' output is a valid partials_in
PIN_STAT_CASES = ("u320_hw4096", "v128_hw4096", "v512_hw1024", "v512_hw4096", "cpg2_hw256", "cpg64_g8_hw64", "twin_cpg40")

# (channels, batch, side): statistics produced by idb_gemm (idb_gemm_desc.gn_partials) for a [batch][side*side][channels] output, 32 groups,
# at shapes where hw / 64 differs from the two-launch chunk count or chunk length (asserted through the query)
GEMM_PIN = ((320, 2, 32), (640, 2, 32), (1280, 2, 16), (128, 16, 64), (256, 8, 64), (512, 4, 64))


def gemm_pin_case(lib, c, batch, side) -> GnCase:
    p = plan(lib, c, 0, batch, side * side, 32)[1]
    return GnCase(f"gemm_{c}_b{batch}_hw{side * side}", c, 0, batch, side * side, 32, p.sw, p.chunks, False, True, 1e-5, ("count", "normal"))


def gn_cases(lib) -> List[GnCase]:
    return _fixed_gn_cases() + threshold_cases(lib)


LN_C = (8, 64, 320, 504, 512, 520, 640, 768, 1024, 1032, 1280, 1536)
LN_ROWS = (1, 2, 3, 4, 5, 77, 513, 4097)
SM_COLS = (8, 64, 504, 2048, 2056, 4096, 9216)
SM_ROWS = (1, 3, 300)


# ------------------------------------------------------------------------------------------------------------------------------------
# input recipes (float64, already rounded to the operand dtype)
# ------------------------------------------------------------------------------------------------------------------------------------
def rnd(x: torch.Tensor, dtype: str) -> torch.Tensor:
    return x.float().to(TDT[dtype]).double()


def gn_inputs(case: GnCase, recipe: str, dtype: str, device="cpu", seed=30):
    """(x [batch][hw][C] float64 rounded to the operand dtype, gamma, beta fp32 values as float64)."""
    g = torch.Generator(device=device).manual_seed(seed)
    b, hw, c, cpg = case.batch, case.hw, case.c, case.cpg
    grp = torch.arange(c, device=device) // cpg
    pix = torch.arange(hw, device=device)[None, :, None]
    ch = torch.arange(c, device=device)[None, None, :]

    def randn():
        return torch.randn(b, hw, c, generator=g, device=device, dtype=torch.float32).double()

    if recipe == "normal":               # the distribution of test_groupnorm
        x = randn() * 2 + 0.5
        if case.c1:
            x[..., case.c0:] = (x[..., case.c0:] - 0.5) / 2 - 1.0
    elif recipe == "offset":             # per-group mean / std of 4, 16, 64
        x = randn() + torch.tensor([4.0, 16.0, 64.0], device=device, dtype=torch.float64)[grp % 3]
    elif recipe == "mixed_scale":
        x = (randn() + (ch % cpg).double() / cpg * 2) * torch.tensor([1.0, 1024.0], device=device, dtype=torch.float64)[grp % 2]
    elif recipe == "constant_group":
        x = (((grp[None, None, :] * 5 + torch.arange(b, device=device)[:, None, None] * 3) % 13 - 6).double() / 2).expand(b, hw, c).contiguous()
    elif recipe == "constant_offset":    # constant per group, but sums that are not exact: the one-pass variance comes out as +- rounding noise
        x = ((grp[None, None, :] % 7 + 60).double() + 0.3).expand(b, hw, c).contiguous()
    elif recipe == "tiny_var":
        x = randn() * 0.003
    elif recipe == "count":
        x = torch.randint(0, 3, (b, hw, c), generator=g, device=device).double()
    elif recipe == "ramp":
        x = ((pix * 3 + ch * 5 + torch.arange(b, device=device)[:, None, None]) % 17 - 8).double() / 4
    elif recipe == "outlier":
        x = randn()
        x[0, hw // 2, 1] = 4096.0
    else:
        raise ValueError(recipe)
    gamma = (torch.randn(c, generator=g, device=device, dtype=torch.float32) * 0.2 + 1).double()
    beta = (torch.randn(c, generator=g, device=device, dtype=torch.float32) * 0.1).double()
    return rnd(x, dtype), gamma, beta


def ln_inputs(rows, c, recipe, dtype, device="cpu", seed=40):
    g = torch.Generator(device=device).manual_seed(seed)
    x = torch.randn(rows, c, generator=g, device=device, dtype=torch.float32).double()
    r = torch.arange(rows, device=device)[:, None]
    if recipe == "normal":               # test_layernorm's
        x = x * 3 + 1
    elif recipe == "offset":             # mean / std 4 .. 1024 by row
        x = x + torch.tensor([4.0, 16.0, 64.0, 256.0, 1024.0], device=device, dtype=torch.float64)[r % 5]
    elif recipe == "constant_row":
        x = ((r % 13 - 6).double() / 2).expand(rows, c).contiguous()
    elif recipe == "count":
        x = torch.randint(0, 3, (rows, c), generator=g, device=device).double()
    elif recipe == "outlier":
        x[:, c // 2] = 4096.0
    else:
        raise ValueError(recipe)
    gamma = (torch.randn(c, generator=g, device=device, dtype=torch.float32) * 0.2 + 1).double()
    beta = (torch.randn(c, generator=g, device=device, dtype=torch.float32) * 0.1).double()
    return rnd(x, dtype), gamma, beta


def sm_inputs(rows, cols, recipe, dtype, device="cpu", seed=50):
    g = torch.Generator(device=device).manual_seed(seed)
    x = torch.randn(rows, cols, generator=g, device=device, dtype=torch.float32).double() * 4
    r = torch.arange(rows, device=device)
    if recipe == "peaked":               # one logit 30 above the rest: the rest land in f16's subnormals
        x = x / 4
        x[r, (r * 37 + cols - 1) % cols] = x.amax(-1) + 30
    elif recipe == "constant_row":
        x = ((r[:, None] % 7 - 3).double() * 8).expand(rows, cols).contiguous()
    elif recipe == "shifted":            # softmax is shift-invariant; exp(x) itself over- or underflows
        x = x + torch.tensor([200.0, -200.0, 1000.0], device=device, dtype=torch.float64)[r % 3][:, None]
    elif recipe != "normal":
        raise ValueError(recipe)
    return rnd(x, dtype)


# ------------------------------------------------------------------------------------------------------------------------------------
# float64 references
# ------------------------------------------------------------------------------------------------------------------------------------
def eps32(eps: float) -> float:
    return float(torch.tensor(eps, dtype=torch.float32).double())


def act(z, silu):
    return z / (1 + torch.exp(-z)) if silu else z


@dataclass
class GnRef:
    ref: torch.Tensor
    z: torch.Tensor
    x: torch.Tensor
    mu: torch.Tensor         # broadcastable to x, per (sample, channel's group)
    var: torch.Tensor
    s1: torch.Tensor
    s2: torch.Tensor
    gamma: torch.Tensor
    beta: torch.Tensor
    eps: float
    silu: bool


def gn_reference(x, gamma, beta, groups, eps, silu) -> GnRef:
    b, hw, c = x.shape
    cpg = c // groups
    xg = x.view(b, hw, groups, cpg)
    mu = xg.mean(dim=(1, 3), keepdim=True)
    var = ((xg - mu) ** 2).mean(dim=(1, 3), keepdim=True)
    s1 = xg.abs().mean(dim=(1, 3), keepdim=True)
    s2 = (xg * xg).mean(dim=(1, 3), keepdim=True)
    e = eps32(eps)
    ex = lambda t: t.expand(b, 1, groups, cpg).reshape(b, 1, c)     # noqa: E731
    z = ((xg - mu) / torch.sqrt(var + e)).view(b, hw, c) * gamma + beta
    return GnRef(act(z, silu), z, x, ex(mu), ex(var), ex(s1), ex(s2), gamma, beta, e, silu)


def gn_bound(r: GnRef, p: Plan, dtype: str, recipe: str, out_rounding=True, stat_factor=1.0) -> torch.Tensor:
    lip = L_SILU if r.silu else 1.0
    rg = r.gamma.abs() / torch.sqrt(r.var + r.eps)
    b = lip * E24 * (4 * r.x.abs() * rg + 6 * r.mu.abs() * rg + 2 * r.beta.abs())
    if out_rounding:
        b = b + UNIT[dtype] * r.ref.abs()
        if dtype == "f16":
            b = b + 2.0 ** -25
    if recipe not in EXACT_SUMS:
        d = gn_depth(p) * stat_factor
        b = b + lip * rg * d * E24 * r.s1
        b = b + lip * (r.x - r.mu).abs() * rg * 0.5 * d * E24 * (r.s2 + 2 * r.mu.abs() * r.s1) / (r.var + r.eps)
    if r.silu:
        b = b + SILU_EVAL * E24 * r.ref.abs()
    return b


def fp8_value(y: torch.Tensor, inv_scale: float) -> torch.Tensor:
    """e4m3 round-to-nearest-even of clamp(y * inv_scale, -448, 448), as float64."""
    return (y * inv_scale).clamp(-448.0, 448.0).float().to(F8).double()


def fp8_interval(r: GnRef, p: Plan, dtype: str, recipe: str, inv_scale: float):
    b = gn_bound(r, p, dtype, recipe, out_rounding=False) + E24 * r.ref.abs()
    return fp8_value(r.ref - b, inv_scale), fp8_value(r.ref + b, inv_scale)


def ln_reference(x, gamma, beta, eps):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps32(eps)) * gamma + beta, mu, var


LN_DEPTH = 24 + 6


def ln_bound(x, gamma, beta, eps, dtype, recipe):
    ref, mu, var = ln_reference(x, gamma, beta, eps)
    rg = gamma.abs() / torch.sqrt(var + eps32(eps))
    b = UNIT[dtype] * ref.abs() + E24 * (4 * x.abs() * rg + 6 * mu.abs() * rg + 2 * beta.abs())
    if dtype == "f16":
        b = b + 2.0 ** -25
    if recipe not in ("count", "constant_row"):
        b = b + rg * (LN_DEPTH + 1) * E24 * x.abs().mean(-1, keepdim=True)
    b = b + (x - mu).abs() * rg * 0.5 * (LN_DEPTH + 3) * E24
    return ref, b


def sm_reference(x):
    p = torch.exp(x - x.amax(-1, keepdim=True))
    return p / p.sum(-1, keepdim=True)


def sm_bound(x, dtype):
    ref = sm_reference(x)
    d = _ceil(x.shape[-1], 2048) * 8 + 6 + 3
    b = UNIT[dtype] * ref + E24 * ((x - x.amax(-1, keepdim=True)).abs() + d + 6) * ref
    if dtype == "f16":
        b = b + 2.0 ** -25
    return ref, b


def gn_partial_sums(x, p: Plan, groups):
    """float64 {sum, sum of squares} and {sum |x|, sum x^2} per (sample, chunk, group): [batch][chunks][groups][2] each."""
    b, hw, c = x.shape
    pad = p.chunks * p.chunk_len - hw
    xp = torch.cat([x, torch.zeros(b, pad, c, dtype=x.dtype, device=x.device)], 1) if pad > 0 else x[:, :p.chunks * p.chunk_len]
    xg = xp.reshape(b, p.chunks, p.chunk_len, groups, c // groups)
    want = torch.stack([xg.sum(dim=(2, 4)), (xg * xg).sum(dim=(2, 4))], -1)
    mag = torch.stack([xg.abs().sum(dim=(2, 4)), (xg * xg).sum(dim=(2, 4))], -1)
    return want, mag


def old_criterion(out, ref, dtype, scale=1.0) -> bool:
    """`_check(out, ref, _tol(eng, scale))` of tests/test_kernels_gpu.py."""
    tol = (2.0 ** -7 if dtype == "bf16" else 2.0 ** -9) * scale
    return bool((out.double() - ref).abs().max().item() <= tol * max(1.0, ref.abs().max().item()))


# ------------------------------------------------------------------------------------------------------------------------------------
# the emulation of the kernels' arithmetic contract, with injectable defects
# ------------------------------------------------------------------------------------------------------------------------------------
GN_STAT_DEFECTS = ("tail_twice", "group_off_by_one", "last_slot_lost", "x1_stride", "inactive_rows")
GN_COMBINE_DEFECTS = ("last_chunk_dropped", "cnt_full_chunks", "no_eps", "no_clamp", "stale_partial", "apply_wrong_chunks")
GN_APPLY_DEFECTS = ("neighbour_gamma", "silu_skipped")
FP8_DEFECTS = ("fp8_no_saturation", "fp8_double_rounding")
GN_DEFECTS = GN_STAT_DEFECTS + GN_COMBINE_DEFECTS + GN_APPLY_DEFECTS + FP8_DEFECTS
LN_DEFECTS = ("ln_padded_count", "ln_one_pass")
SM_DEFECTS = ("sm_no_max", "sm_three_waves")
DEFECTS = GN_DEFECTS + LN_DEFECTS + SM_DEFECTS

_XOR = {o: torch.arange(64) ^ o for o in (1, 2, 4, 8, 16, 32)}


def _butterfly(v, stages):
    """__shfl_xor tree over the last axis (64 lanes, or groups of 8 for stages (1, 2, 4)), fp32."""
    for o in stages:
        v = v + v[..., _XOR[o][:v.shape[-1]].to(v.device)]
    return v


def emulate_gn_partials(x, c0, groups, p: Plan, defect=None):
    """gn_stats_kernel (and the first half of gn_sync_kernel): which element enters which fp32 partial, in the kernel's order: a thread's
    serial sum over the pixels it owns (rows row, row + PR, ... of its chunk), the fold of its 8 channels into <= 4 group slots, per group
    the lane-strided serial sum over the threads and the shuffle tree.  x: [batch][hw][C] float64 -> fp32 [batch][chunks][groups][2]."""
    dev = x.device
    b, hw, c = x.shape
    cpg, pr, cols, n, cl, sw = c // groups, p.pr, p.cols, p.chunks, p.chunk_len, p.sw
    nsl, gps = c // sw, sw // cpg
    xf = x.float()
    if defect == "x1_stride" and c0 < c:          # x1 + pix * C0 + (c - C0) instead of pix * C1
        c1 = c - c0
        flat = xf[..., c0:].reshape(-1)
        idx = (torch.arange(b * hw, device=dev)[:, None] * c0 + torch.arange(c1, device=dev)[None, :]) % flat.numel()
        xf = torch.cat([xf[..., :c0], flat[idx].view(b, hw, c1)], -1)
    kk = _ceil(_ceil(cl, pr), 4) * 4                                           # loads are issued in batches of 4
    k_i, r_i, ch_i = torch.arange(kk, device=dev)[None, :, None], torch.arange(pr, device=dev)[None, None, :], torch.arange(n, device=dev)[:, None, None]
    p0 = ch_i * cl
    p1 = torch.clamp(p0 + cl, max=hw)
    pos = p0 + r_i + k_i * pr                                                  # [n][kk][pr]
    valid = pos < p1
    ran = (p0 + r_i + (k_i // 4) * 4 * pr) < p1                                # the batch this load belongs to was issued
    src = torch.minimum(pos, (p1 - 1).clamp(min=0))
    take = (ran if defect == "tail_twice" else valid)
    s = torch.zeros(b, n, pr, c, dtype=torch.float32, device=dev)
    ss = torch.zeros_like(s)
    for k in range(kk):
        v = xf[:, src[:, k]] * take[:, k, :, None]                             # [b][n][pr][c]
        s = s + v
        ss = ss + v * v
    if defect == "inactive_rows" and cols * pr < GN_THREADS:                   # threads cols*PR .. 255 (row == PR) accumulate too
        extra = GN_THREADS - cols * pr
        m = torch.zeros(nsl, cols, 8, device=dev)
        m[:, :extra] = 1
        m = m.view(1, 1, c)
        e_s, e_ss = torch.zeros_like(s[:, :, 0]), torch.zeros_like(s[:, :, 0])
        for k in range(1, kk):
            v = xf[:, src[:, k, 0]] * valid[:, k, 0, None]
            e_s, e_ss = e_s + v, e_ss + v * v
        s = torch.cat([s, (e_s * m)[:, :, None]], 2)
        ss = torch.cat([ss, (e_ss * m)[:, :, None]], 2)
        pr = pr + 1
    chn = torch.arange(c, device=dev).view(nsl, cols, 8)
    g_first = chn[..., 0] // cpg                                               # [nsl][cols]
    slot = chn // cpg - g_first[..., None]
    if defect == "group_off_by_one":
        slot = torch.where(slot[..., 7:8] > 0, ((chn + 1) // cpg - g_first[..., None]).clamp(max=3), slot)
    outs = []
    for acc in (s, ss):
        a = acc.view(b, n, pr, nsl, cols, 8)
        gs = torch.zeros(b, n, pr, nsl, cols, 4, dtype=torch.float32, device=dev)
        for e in range(8):
            for q in range(4):
                gs[..., q] = gs[..., q] + a[..., e] * (slot[..., e] == q)
        if defect == "last_slot_lost":
            gs[..., 3] = 0
        # group gl of slice sl takes slot k = sl * gps + gl - g_first[sl][col] of thread (row, col)
        kidx = (torch.arange(nsl, device=dev)[:, None, None] * gps + torch.arange(gps, device=dev)[None, :, None]) - g_first[:, None, :]   # [nsl][gps][cols]
        w = torch.zeros(b, n, nsl, gps, pr, cols, dtype=torch.float32, device=dev)
        gsp = gs.permute(0, 1, 3, 2, 4, 5)                                      # [b][n][nsl][pr][cols][4]
        for q in range(4):
            w = w + gsp[..., q][:, :, :, None] * (kidx == q)[None, None, :, :, None, :]
        nact = pr * cols
        w = w.reshape(b, n, nsl, gps, nact)
        m64 = _ceil(nact, 64)
        w = torch.cat([w, torch.zeros(b, n, nsl, gps, m64 * 64 - nact, dtype=torch.float32, device=dev)], -1).view(b, n, nsl, gps, m64, 64)
        lane = torch.zeros(b, n, nsl, gps, 64, dtype=torch.float32, device=dev)
        for i in range(m64):
            lane = lane + w[..., i, :]
        outs.append(_butterfly(lane, (32, 16, 8, 4, 2, 1))[..., 0].reshape(b, n, groups))
    return torch.stack(outs, -1)


def emulate_gn_combine(partial, hw, cpg, eps, defect=None, cnt_plan: Optional[Plan] = None):
    """Second half: 8 lanes per group sum the chunks' partials (lane sub takes sub, sub + 8, ...), a 3-stage shuffle tree, then mean, var and
    rstd in double, stored as fp32.  partial: fp32 [batch][chunks][groups][2] -> (mean, rstd) fp32 [batch][groups]."""
    b, n, groups, _ = partial.shape
    if defect == "last_chunk_dropped" and n > 1:
        partial, n = partial[:, :-1], n - 1
    pp = torch.cat([partial, torch.zeros(b, 64 - n, groups, 2, dtype=torch.float32, device=partial.device)], 1).view(b, 8, 8, groups, 2)
    acc = torch.zeros(b, 8, groups, 2, dtype=torch.float32, device=partial.device)
    for u in range(8):
        acc = acc + pp[:, u]
    tot = _butterfly(acc.permute(0, 2, 3, 1), (1, 2, 4))[..., 0].double()       # [b][groups][2]
    cnt = float(hw) * cpg
    if defect == "cnt_full_chunks":
        cnt = float(cnt_plan.chunks * cnt_plan.chunk_len) * cpg
    mean = tot[..., 0] / cnt
    var = tot[..., 1] / cnt - mean * mean
    if defect != "no_clamp":
        var = var.clamp(min=0.0)
    e = 0.0 if defect == "no_eps" else eps32(eps)
    return mean.float(), (1.0 / torch.sqrt(var + e)).float()


def _round_fma(a, b, c):
    """fp32 fma(a, b, c): the product of two fp32 values is exact in double."""
    return (a.double() * b.double() + c.double()).float()


def emulate_gn_apply(x, mean, rstd, gamma, beta, groups, silu, dtype, p: Plan, defect=None, fp8_inv_scale=0.0):
    b, hw, c = x.shape
    cpg = c // groups
    ga, be = gamma.float(), beta.float()
    if defect == "neighbour_gamma":
        ga, be = torch.roll(ga, -p.sw), torch.roll(be, -p.sw)
    ex = lambda t: t[:, :, None].expand(b, groups, cpg).reshape(b, 1, c)    # noqa: E731
    ks = ex(rstd) * ga
    kh = _round_fma(-ex(mean), ks, be.expand(b, 1, c))
    y = _round_fma(x.float(), ks, kh)
    if silu and defect != "silu_skipped":
        y = y / (1 + torch.exp(-y))
    if fp8_inv_scale > 0:
        if defect == "fp8_double_rounding":
            y = y.to(TDT[dtype]).float()
        y = y * fp8_inv_scale
        if defect != "fp8_no_saturation":
            y = y.clamp(-448.0, 448.0)
        return y.to(F8).double()
    return y.to(TDT[dtype]).double()


def emulate_gn(x, c0, gamma, beta, groups, eps, silu, dtype, p: Plan, defect=None, fp8_inv_scale=0.0, stale=None, pin=None, wrong: Optional[Plan] = None):
    """One idb_groupnorm / idb_groupnorm_fp8 call under plan p.  pin: the partials_in of form 2 (else the statistics are emulated with p's
    chunks); stale: partials of an earlier launch through the same workspace (stale_partial); wrong: the plan whose chunk count a defective
    apply-only pass would index partials_in with (apply_wrong_chunks)."""
    b, hw, c = x.shape
    partial = pin if pin is not None else emulate_gn_partials(x, c0, groups, p, defect)
    if defect == "stale_partial" and stale is not None and partial.shape[1] > 1:
        partial = partial.clone()
        partial[:, 1] = stale[:, 1]
    if defect == "apply_wrong_chunks" and wrong is not None:
        flat = partial.reshape(-1)
        n = wrong.chunks
        idx = ((torch.arange(b)[:, None, None] * n + torch.arange(n)[None, :, None]) * groups + torch.arange(groups)[None, None, :]) * 2
        partial = torch.stack([flat[idx % flat.numel()], flat[(idx + 1) % flat.numel()]], -1)
    mean, rstd = emulate_gn_combine(partial, hw, c // groups, eps, defect, p)
    return emulate_gn_apply(x, mean, rstd, gamma, beta, groups, silu, dtype, p, defect, fp8_inv_scale)


def emulate_ln(x, gamma, beta, eps, dtype, defect=None):
    """layernorm_kernel: lane l owns the 8-channel vectors l, l + 64, l + 128; serial fp32 sums per lane, a 6-stage shuffle tree, the mean,
    then the sum of (x - mean)^2 the same way (two passes over registers), rsqrt, affine, one rounding."""
    rows, c = x.shape
    ct = c // 8
    nch = _ceil(ct, 64)
    v = torch.cat([x.float(), torch.zeros(rows, nch * 512 - c)], -1).view(rows, nch, 64, 8)
    inside = (torch.arange(nch)[:, None] * 64 + torch.arange(64)[None, :] < ct)[None, :, :, None]
    s = torch.zeros(rows, 64)
    for i in range(nch):
        for e in range(8):
            s = s + v[:, i, :, e]
    count = float(nch * 512 if defect == "ln_padded_count" else c)
    mean = (_butterfly(s, (32, 16, 8, 4, 2, 1))[:, :1] / torch.tensor(count, dtype=torch.float32))
    sq = torch.zeros(rows, 64)
    for i in range(nch):
        for e in range(8):
            d = (v[:, i, :, e] - mean) * inside[0, i, :, 0]
            sq = sq + (v[:, i, :, e] * v[:, i, :, e] if defect == "ln_one_pass" else d * d)
    tot = _butterfly(sq, (32, 16, 8, 4, 2, 1))[:, :1] / torch.tensor(count, dtype=torch.float32)
    if defect == "ln_one_pass":
        tot = tot - mean * mean
    rstd = torch.rsqrt(tot + torch.tensor(eps, dtype=torch.float32))
    y = (x.float() - mean) * rstd * gamma.float() + beta.float()
    return y.to(TDT[dtype]).double()


def emulate_sm(x, dtype, defect=None):
    """softmax_rows_kernel: thread t owns vectors t, t + 256, ...; exact max; serial fp32 sum of exp per thread, wave trees, the four wave
    sums added in order; exp(x - max) * (1 / sum), one rounding."""
    rows, cols = x.shape
    ct = cols // 8
    nj = _ceil(ct, 256)
    xf = x.float()
    mx = torch.zeros(rows, 1) if defect == "sm_no_max" else xf.amax(-1, keepdim=True)
    ex = torch.exp(xf - mx)
    v = torch.cat([ex, torch.zeros(rows, nj * 2048 - cols)], -1).view(rows, nj, 256, 8)
    s = torch.zeros(rows, 256)
    for j in range(nj):
        for e in range(8):
            s = s + v[:, j, :, e]
    waves = _butterfly(s.view(rows, 4, 64), (32, 16, 8, 4, 2, 1))[..., 0]
    tot = waves[:, 0] + waves[:, 1] + waves[:, 2]
    if defect != "sm_three_waves":
        tot = tot + waves[:, 3]
    return (ex * (1.0 / tot)[:, None]).to(TDT[dtype]).double()


# ------------------------------------------------------------------------------------------------------------------------------------
# the conditioning envelope of the one-pass variance
# ------------------------------------------------------------------------------------------------------------------------------------
ENVELOPE_R = (1, 4, 16, 64, 256)


def envelope_cases() -> List[GnCase]:
    """The three sum lengths that matter: 64 pixels x 40 channels (the UNet's deepest level), 4096 x 10 (its first), 262144 x 4 (the
    VAE decoder's last stage)."""
    return [GnCase("env_64x40", 1280, 0, 2, 64, 32, 80, 2, True, False, 1e-5), GnCase("env_4096x10", 320, 0, 2, 4096, 32, 80, 64, True, False, 1e-5),
            GnCase("env_262144x4", 128, 0, 1, 262144, 32, 64, 64, False, False, 1e-5)]


def envelope_inputs(case: GnCase, ratio: float, dtype: str, device="cpu", seed=70):
    """N(0, 1) + ratio in every group, gamma = 1, beta = 0 (so the output is the normalised value itself)."""
    g = torch.Generator(device=device).manual_seed(seed)
    x = torch.randn(case.batch, case.hw, case.c, generator=g, device=device, dtype=torch.float32).double() + ratio
    return rnd(x, dtype), torch.ones(case.c, dtype=torch.float64, device=device), torch.zeros(case.c, dtype=torch.float64, device=device)


def envelope_figures(out, r: GnRef, p: Plan, dtype: str) -> Tuple[float, float]:
    """(worst |got - ref|, worst statistics lines of the criterion), both over u * max(|ref|, 1): the error of the mean is absolute in z,
    so relative to an output near zero it is unbounded at any conditioning; outputs of magnitude >= 1 are a third of the tensor."""
    den = UNIT[dtype] * r.ref.abs().clamp(min=1.0)
    stat = gn_bound(r, p, dtype, "offset") - gn_bound(r, p, dtype, "count")
    return float(((out.double() - r.ref).abs() / den).max()), float((stat / den).max())
