"""The idb_gemm test matrix shared by test_gemm_matrix_cpu.py (host-only enumeration) and test_gemm_matrix_gpu.py (launch + compare):
a fixed set of problem cases chosen to hit tile edges, every tile id 0..109 (0 = the planner's own choice), and a list of descriptor
feature combinations.  classify() decides, without any GPU call, whether idb_gemm accepts a (case, tile, feature) combination; only
accepted combinations are ever launched.

idb_gemm refuses a few descriptors that idb_gemm_plan accepts (row_stats_out, ln_stats, gn_in_* and w_groups are checked inside
idb_gemm, before any HIP call; tests/test_plan_table_cpu.py).  classify() probes the first three the way the plan table does: the probe
descriptor carries a defect that idb_gemm rejects with IDB_EINVAL right after the check under test, so idb_gemm answers -2 (refused) or
-1 (accepted) and never launches.  The w_groups check is the last one and is predicted from the plan (persistent variant, or
w_group_rows not a multiple of the tile height).

check() is the element-wise comparison:  |out - ref| <= C_R * u * |ref| + C_A * sqrt(K) * 2^-24 * absprod, elementwise, where u is the
unit roundoff of the output dtype and absprod the float64 |A||W| product carried through the epilogue (plus |bias|, |residual|, ...),
so the bound follows cancellation instead of the tensor's largest value."""
import ctypes as C
import math
from dataclasses import dataclass
from typing import List, Tuple

import numpy as np

from faceposegenerator_amd import _lib as L

PTR = 1 << 20          # any non-null 16-byte-aligned address: the host-side calls never dereference it

# tile id = shape + 10 * family (include/idb_kernels.h); shape -> (rows, cols) of the 64/128-row forms
SHAPE_TILE = {1: (128, 160), 2: (128, 128), 3: (64, 160), 4: (64, 64), 5: (128, 32), 6: (64, 160), 7: (64, 128), 8: (128, 160), 9: (128, 128)}
FAMILIES = {0: "ring2", 1: "ring3", 2: "ring4", 3: "regstaged", 4: "persistent", 5: "lw3x4", 6: "lw3x8", 7: "lw4x4", 8: "lw256", 9: "patch256",
            10: "patch_small"}
GN_GROUPS = 32
# the tile ids idb_gemm builds (its variant table kVariants); test_gemm_matrix_cpu.py checks this list against the planner
VARIANT_IDS = [1, 2, 3, 4, 5, 6, 7, 8, 9, 11, 12, 13, 14, 16, 17, 18, 19, 21, 22, 23, 31, 32, 33, 35, 41, 42, 54, 56, 57, 58, 59,
               64, 66, 67, 68, 69, 74, 76, 77, 78, 79, 88, 89, 98, 99, 104, 106, 107, 108, 109]


def tile_dims(tile: int) -> Tuple[int, int]:
    bm, bn = SHAPE_TILE[tile % 10]
    return (2 * bm if tile // 10 in (8, 9) else bm), bn


# ------------------------------------------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    name: str
    batch: int
    out_h: int
    out_w: int
    n: int
    srcs: Tuple[Tuple[int, int, int, int, int], ...]     # (channels, taps, in_h, in_w, upsample)
    stride: int = 1
    pad_mode: int = 0
    split_k: int = 0

    @property
    def M(self) -> int:
        return self.batch * self.out_h * self.out_w

    @property
    def K(self) -> int:
        return sum(c * t for c, t, *_ in self.srcs)

    @property
    def hw(self) -> int:
        return self.out_h * self.out_w


def _lin(name, m, k, n, split_k=0):
    return Case(name, m, 1, 1, n, ((k, 1, 1, 1, 0),), split_k=split_k)


def _conv(name, b, ih, iw, cin, n, stride=1, up=0, pad_mode=0, extra=(), split_k=0):
    lh, lw = ih << up, iw << up
    oh, ow = (lh + stride - 1) // stride, (lw + stride - 1) // stride
    srcs = ((cin, 9, ih, iw, up),) + tuple((c, taps, oh, ow, 0) for c, taps in extra)
    return Case(name, b, oh, ow, n, srcs, stride, pad_mode, split_k)


CASES: List[Case] = [
    # ragged M and N against every tile height (64 / 128 / 256) and width (32 / 64 / 128 / 160)
    _lin("lin_300x264", 300, 320, 264),
    _lin("lin_200x100", 200, 192, 100),                 # n = 96 + 4: not a multiple of 8 (direct epilogue)
    _lin("lin_1000x20", 1000, 128, 20),                 # n <= 32: the 128x32 tile
    # 1x1 convs on a spatial grid: a tile spans two or more samples (per-sample bias switch, gn_partials chunks)
    Case("grid_3x10x10", 3, 10, 10, 160, ((256, 1, 10, 10, 0),)),
    Case("grid_5x8x8", 5, 8, 8, 192, ((128, 1, 8, 8, 0),)),
    # 3x3 convs: square / non-square grids, stride 2, upsample, pad_mode 1
    _conv("conv_3x8x8", 3, 8, 8, 128, 160),
    _conv("conv_2x12x20", 2, 12, 20, 64, 128),
    _conv("conv_1x16x16", 1, 16, 16, 192, 320),
    _conv("conv_s2_2x17x15", 2, 17, 15, 64, 96, stride=2),
    _conv("conv_up_2x6x5", 2, 6, 5, 128, 128, up=1),
    _conv("conv_pad1_2x16x16", 2, 16, 16, 64, 64, stride=2, pad_mode=1),
    # two and three K segments: resnet conv2 + 1x1 shortcut over a skip concatenation, and a 3x3 skip concatenation
    _conv("conv2_sc_2x8x8", 2, 8, 8, 192, 192, extra=((64, 1), (128, 1))),
    Case("cat_1x16x16", 1, 16, 16, 128, ((128, 9, 16, 16, 0), (64, 9, 16, 16, 0))),
    # split-K: K = 2880 (45 K-steps); 4 / 8 / 16 take the K-slice-per-XCD remap, 3 / 5 do not; 4 and 8 end on a short slice, 16 on an
    # empty one (kt_per_split 3: slices 0..14 hold all 45 steps)
    _lin("lin_k2880_sk3", 256, 2880, 320, 3),
    _lin("lin_k2880_sk4", 256, 2880, 320, 4),
    _lin("lin_k2880_sk5", 256, 2880, 320, 5),
    _lin("lin_k2880_sk8", 256, 2880, 320, 8),
    _lin("lin_k2880_sk16", 256, 2880, 320, 16),
    _conv("conv_k2880_sk4", 2, 8, 8, 320, 160, split_k=4),
    # long K
    _lin("lin_k5120", 128, 5120, 256),
]


# ------------------------------------------------------------------------------------------------------------------------------------
# feature combinations (each on top of bias unless it replaces it)
# ------------------------------------------------------------------------------------------------------------------------------------
FEATURES = {
    "plain": (),
    "res": ("res",),
    "sb": ("sb",),
    "f32": ("f32",),
    "gelu": ("gelu",),
    "prelu": ("prelu",),
    "relu": ("relu",),
    "geglu": ("geglu",),
    "out2": ("out2",),
    "gnp": ("gnp",),
    "rows": ("rows",),
    "ln": ("ln",),
    "gn": ("gn",),
    "gn_nosilu": ("gn", "nosilu"),
    "gn2": ("gn", "gn2"),
    "tiled": ("tiled",),
    "wgroups": ("wgroups",),
    "flags4": ("flags4",),
    "flags8": ("flags8",),
    "flags16": ("flags16",),
    "ln_flags256": ("ln", "flags256"),
    # the combinations the engine uses
    "res_sb_gnp": ("res", "sb", "gnp"),
    "gn_gnp": ("gn", "gnp"),
    "prelu_out2": ("prelu", "out2"),
    "res_out2": ("res", "out2"),
    "prelu_out2_res": ("prelu", "out2", "res"),
    "rows_flags16": ("rows", "flags16"),
    "tiled_res_sb": ("tiled", "res", "sb"),
}


def applicable(case: Case, feat: str) -> bool:
    """Feature combinations that do not describe the case at all (not refusals: the descriptor cannot even be written)."""
    f = FEATURES[feat]
    if "gn2" in f and len(case.srcs) < 2:
        return False
    if "gn" in f and any(s[2:4] != (case.out_h, case.out_w) or s[4] for s in case.srcs[:2 if "gn2" in f else 1]):
        return False          # the fused GroupNorm normalises sources on the output grid only
    if "gn" in f and case.out_h * case.out_w == 1:
        return False          # a plain matrix has no GroupNorm
    if "ln" in f and (len(case.srcs) != 1 or case.srcs[0][1] != 1):
        return False          # a folded LayerNorm reads one 1x1 source
    if "geglu" in f and case.n % 32:
        return False
    if "gnp" in f and case.out_h * case.out_w == 1:
        return False
    return True


def make_desc(case: Case, dt: int, tile: int, feat: str, ptrs=None, bm: int = 0) -> L.GemmDesc:
    """The descriptor of one combination.  ptrs: name -> device address (GPU run); None: the non-null dummy PTR everywhere (host-only
    queries).  bm: the plan's tile height (w_group_rows); 0 before the plan is known."""
    f = FEATURES[feat]
    P = (lambda k: ptrs[k]) if ptrs is not None else (lambda k: PTR)
    d = L.GemmDesc()
    d.dtype, d.batch, d.out_h, d.out_w, d.stride, d.n, d.nsrc = dt, case.batch, case.out_h, case.out_w, case.stride, case.n, len(case.srcs)
    d.pad_mode = case.pad_mode
    for i, (ch, taps, ih, iw, up) in enumerate(case.srcs):
        d.src[i].ptr, d.src[i].channels, d.src[i].taps, d.src[i].in_h, d.src[i].in_w, d.src[i].upsample = P(f"src{i}"), ch, taps, ih, iw, up
    d.w, d.out, d.out_dtype = P("w_tiled" if "tiled" in f else "w"), P("out32" if "f32" in f else "out"), L.IDB_F32 if "f32" in f else dt
    d.geglu = int("geglu" in f)
    d.out_ld = case.n // 2 if d.geglu else case.n
    d.w_layout = int("tiled" in f)
    d.split_k, d.tile = case.split_k, tile
    if "ln" not in f:
        d.bias = P("bias")
    if "res" in f:
        d.residual = P("res")
    if "sb" in f:
        d.sample_bias, d.sample_bias_ld = P("sbias"), case.n
    if "f32" in f:
        d.out_scale = 0.5
    d.act = 1 if "gelu" in f else 2 if "prelu" in f else 3 if "relu" in f else 0
    if "prelu" in f:
        d.act_slope = P("slope")
    if "out2" in f:
        d.out2, d.out2_scale, d.out2_shift = P("out2"), P("out2_scale"), P("out2_shift")
    if "gnp" in f:
        d.gn_partials, d.gn_groups = P("gnp"), GN_GROUPS
    if "rows" in f:
        d.row_stats_out = P("rows")
    if "ln" in f:
        d.ln_stats, d.ln_tiles, d.ln_u, d.ln_v, d.ln_eps = P("ln_stats"), 2, P("ln_u"), P("ln_v"), 1e-5
    if "gn" in f:
        d.gn_in_partials, d.gn_in_chunks, d.gn_in_groups, d.gn_in_eps = P("gn_part"), gn_chunks(case), GN_GROUPS, 1e-5
        d.gn_in_gamma, d.gn_in_beta = P("gn_gamma"), P("gn_beta")
        d.gn_in_silu, d.gn_in_nsrc = int("nosilu" not in f), 2 if "gn2" in f else 1
    if "wgroups" in f:
        d.w_groups, d.w_group_rows, d.w_group_stride = 2, bm or 64, case.n * case.K * 2
    flags = (4 if "flags4" in f else 0) | (8 if "flags8" in f else 0) | (16 if "flags16" in f else 0) | (256 if "flags256" in f else 0)
    d.flags = flags
    if flags & 16:
        d.counters, d.counters_len = P("counters"), COUNTERS
    return d


COUNTERS = 1 << 14


def gn_chunks(case: Case) -> int:
    return 2 if case.hw % 2 == 0 else 1


# ------------------------------------------------------------------------------------------------------------------------------------
# host-side classification
# ------------------------------------------------------------------------------------------------------------------------------------
@dataclass
class Verdict:
    accepted: bool
    tile: int = 0          # the plan's tile id (accepted, or refused by idb_gemm after planning)
    split_k: int = 0
    where: str = ""        # refusals: "plan" or the idb_gemm check ("rows", "ln", "gn", "wgroups")
    row_tiles: int = 0     # idb_gemm_row_stats_tiles
    emits_gn: int = 0      # idb_gemm_emits_gn_partials
    fuses_gn: int = 0


def classify(lib, case: Case, dt: int, tile: int, feat: str) -> Verdict:
    d = make_desc(case, dt, tile, feat)
    t, sk, bl = C.c_int32(), C.c_int32(), C.c_int32()
    rc = lib.idb_gemm_plan(C.byref(d), C.byref(t), C.byref(sk), C.byref(bl))
    if rc != 0:
        assert rc in (-1, -2), rc
        return Verdict(False, where="plan")
    v = Verdict(True, t.value, sk.value, row_tiles=lib.idb_gemm_row_stats_tiles(C.byref(d)),
                emits_gn=lib.idb_gemm_emits_gn_partials(C.byref(d), GN_GROUPS), fuses_gn=lib.idb_gemm_fuses_groupnorm(C.byref(d)))
    f = FEATURES[feat]
    # the checks inside idb_gemm, in its order; each probe is invalid right behind the check under test
    probes = []
    if "rows" in f or "ln" in f:
        def probe_rows_ln(p):
            if p.row_stats_out:
                p.row_stats_out = PTR + 4            # misaligned: IDB_EINVAL after the refusal check
            else:
                p.ln_tiles = 0                       # IDB_EINVAL after the refusal check
        probes.append(("rows" if "rows" in f else "ln", probe_rows_ln))
    if "gn" in f:
        probes.append(("gn", lambda p: setattr(p, "gn_in_gamma", 0)))
    for where, mutate in probes:
        p = make_desc(case, dt, tile, feat)
        mutate(p)
        g = lib.idb_gemm(C.byref(p), C.c_void_p(PTR), C.c_size_t(1 << 60), None)
        assert g in (-1, -2), (case.name, tile, feat, g)       # never 0: the probe is invalid past the check
        if g == -2:
            v.accepted, v.where = False, where
            return v
    if "wgroups" in f and (v.tile // 10 == 4):
        v.accepted, v.where = False, "wgroups"
    return v


def enumerate_matrix(lib, dts=(L.IDB_BF16, L.IDB_F16), cases=None):
    """{(case name, dtype, tile, feature): Verdict} over every applicable combination."""
    out = {}
    for case in cases or CASES:
        for dt in dts:
            for feat in FEATURES:
                if not applicable(case, feat):
                    continue
                for tile in range(110):
                    out[(case.name, dt, tile, feat)] = classify(lib, case, dt, tile, feat)
    return out


def family_of(tile: int) -> str:
    return FAMILIES[tile // 10]


# ------------------------------------------------------------------------------------------------------------------------------------
# element-wise comparison
# ------------------------------------------------------------------------------------------------------------------------------------
# Calibrated on the MI355X (worst measured ratios in test_gemm_matrix_gpu.py's docstring: 0.995 with operand-dtype outputs, set by
# the output rounding alone; 0.13 with fp32 outputs, i.e. the accumulation uses an eighth of its term).
C_R = 1.0           # output rounding: the kernels round once, so |err| <= u |ref| plus what the accumulation adds
C_A = 1.0           # fp32 accumulation: sqrt(K) 2^-24 per unit of |A||W| (accumulation in blocks of MFMA dot products)
UNIT = {L.IDB_BF16: 2.0 ** -8, L.IDB_F16: 2.0 ** -11, L.IDB_F32: 2.0 ** -24}


def bound(ref, absprod, out_dtype: int, K: int, extra=None):
    b = C_R * UNIT[out_dtype] * ref.abs() + C_A * math.sqrt(K) * 2.0 ** -24 * absprod
    return b if extra is None else b + extra


def ratio(out, ref, absprod, out_dtype: int, K: int, extra=None):
    """Elementwise err / bound (float64); an element whose bound is 0 must be exact (ratio 0) or counts as infinitely wrong."""
    import torch
    err = (out.double() - ref).abs()
    b = bound(ref, absprod, out_dtype, K, extra)
    r = torch.where(b > 0, err / torch.where(b > 0, b, torch.ones_like(b)), torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    return r


def check(out, ref, absprod, out_dtype: int, K: int, what: str = "", extra=None) -> float:
    """Asserts every element within its bound; returns the worst err / bound ratio."""
    r = ratio(out, ref, absprod, out_dtype, K, extra)
    worst = r.max().item() if r.numel() else 0.0
    if not worst <= 1.0:
        i = int(r.argmax().item())
        idx = tuple(int(x) for x in np.unravel_index(i, tuple(r.shape)))
        raise AssertionError(f"{what}: element {idx}: out {out.reshape(-1)[i].item():.6g} ref {ref.reshape(-1)[i].item():.6g} "
                             f"ratio {worst:.3g} ({int((r > 1).sum().item())} of {r.numel()} elements out of bound)")
    return worst


def sum_bound(x_abs_sum, count: int):
    """fp32 summation of `count` terms in any order: |err| <= count * 2^-24 * sum |x_i| (doubled: the squares are rounded too)."""
    return 2.0 * count * 2.0 ** -24 * x_abs_sum
