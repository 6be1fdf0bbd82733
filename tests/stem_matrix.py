"""The test matrix of the VALU kernels at the ends of the networks: idb_conv_in, idb_linear_f32, idb_timestep_sinusoid (csrc/idb_misc.hip),
idb_arcface_stem, idb_arcface_head (csrc/idb_arcface.hip), idb_pose_stem and idb_pose_head (csrc/idb_pose.hip).  Shared by
test_stem_matrix_cpu.py (references against torch, recipes, teeth, argument checks) and test_stem_matrix_gpu.py (launch + compare): cases,
input recipes from fixed seeds, float64 references written from the definitions, numpy float32 emulations of the kernels' arithmetic in the
kernels' order, injectable defects and the bounds; the verdicts and the 16-bit conversions are matrix_common.py's.  numpy only, no GPU.

Criteria.  u = 2^-24, gamma_n = n u / (1 - n u) (forward bound of n fp32 roundings on one term of a sum), u_T = 2^-11 (f16) or 2^-8
(bf16).  Every count below is read off the kernel source; no constant is tuned.

  stems      K = 27 fmaf's onto the bias in (ky, kx, ci) order [27 roundings], one PReLU multiply (ArcFace; the pose stem's ReLU rounds
  conv_in    nothing, and gets the same count) [1], one rounding to T.  S = |bias| + sum |x w| per output in float64,
                 e = gamma_(K + 1 + a) S max(1, |slope|),      bound = e + max(u_T (|ref| + e), sub_T),
             sub_T = 2^-25 for f16 (below 2^-14 f16 is spaced 2^-24, so u_T |ref| is not the half-spacing there), 0 for bf16.
             a = roundings in front of the taps.  Stems: a = 0, because the reference starts from the kernel's own taps: the uint8
             normalisations are restated in numpy float32 one operation at a time ((u / 255 - 0.5) / 0.5 and (u / 255 - mean[c]) / std[c];
             csrc/Makefile relaxes no fp32 division, so both are exact over all 256 x 3 values), and the ArcFace stem's rounding of its
             input to T (both entries) is a rounding to nearest even that numpy reproduces bit for bit.  conv_in: K = 9 cin; a term passes
             its multiply [1] and at most K additions (whether or not the compiler contracts them, K + 1 is the same count as K fmaf's
             and one activation multiply); x * in_scale [a += 1 unless in_scale == 1, where the product is exact]; the 1x1 pre-conv
             v = pre_b + sum_cj pre_w raw [one multiply and at most cin additions: a += cin + 1], propagated through |w|:
             S = |bias| + sum |w| (|pre_b| + sum |pre_w| |x in_scale|).  A padded tap is 0 after the pre-conv, not pre_b.
  out2       (ArcFace stem) bit-equal to fma(float(out), s2, b2) rounded once to fp32 and then once to T, from the GPU's own `out`: fma32
             is a true single-rounding fma (the exact product of two fp32 values fits a float64; the float64 sum is rounded to odd
             with the TwoSum residue, and 53 >= 2 * 24 + 2 bits make the final rounding to fp32 the rounding of the exact value).
  head       idb_arcface_head: every slice is a chain of at most K fmaf's [K], the reduce adds `splits` partials to 0 [splits] and the
             bias [1]:            bound = gamma_(K + splits + 1) (sum |x w| + |bias|), whatever the order.
  linear     idb_linear_f32: a term passes one multiply [1], at most ceil(k / 64) <= K - 1 additions in its lane for K >= 2 (none for
             K = 1), six shuffle additions [6] and the bias [1]:    bound = gamma_(K + 7) (sum |x w| + |bias|).
             silu_in: x * rcp(1 + __expf(-x)) is approximate.  Its numpy float32 emulation's worst relative error r against float64
             silu on the case's x gives the allowance  max(3 r, 4 u) sum |silu(x) w|  (3: device transcendentals against numpy's, the
             project's standing factor), added to the bound, whose sum is then over |silu(x)| (1 + max(3 r, 4 u)).
  pose head  the six linear outputs: HW - 1 additions of the pool [HW], one division [1], C fmaf's [C], six shuffle additions [6],
             three wave additions [3], the bias [1]: at most HW + C + 11 roundings on a term, bounded with HW + C + 12:
                 delta6 = gamma_(HW + C + 12) (sum_c |w_c| mean_p |x_pc| + |bias|).
             R and the angles against float64 Gram-Schmidt / Euler of the float64 six-vector, tolerance = 2 x the first-order
             propagation of delta6 through a float64 central-difference Jacobian (2: the second-order term) + 3 x the worst error of
             the numpy float32 emulation of the post-linear arithmetic on that case, at least 4 ulp32(1) = 2^-21 (R) and
             4 ulp32(180) = 2^-14 (angles).  The recipe keeps the six-vector well conditioned (asserted on the CPU).
  sinusoid   expf(-logf(10000) j / half), the product with t, cosf / sinf, emulated in numpy float32; per case the bar is 3 x the
             emulation's worst error against float64, at least 2 ulp32(1) = 2^-22 (the softmax rule of detect_matrix.py).

The unmodified emulations must meet every criterion at err / bound <= 0.5 (test_stem_matrix_cpu.py).  For the three kernels that round to T
the half applies to e (e_scale): the rounding term is sharp, a correctly rounded value attains u_T |ref| (measured 0.99 of it over a case's
thousands of outputs), so it is kept whole.

DEFECTS lists what is injected into the emulations on the CPU and DEFECT_CASES the named case each one must fail under the criteria above;
`prelu_gt` (PReLU on > instead of >=) differs only at an accumulator of exactly 0, where 0 * slope is 0 again: HARMLESS."""
from dataclasses import dataclass
from functools import lru_cache
from typing import List, Tuple

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

from matrix_common import (DTYPES, F32, F64, GUARD, NAN16, NAN32, SUB_T, U, U_T, bf16_bits, check, describe, fma32, from_bits,  # noqa: F401
                           gamma, round_T, to_bits, ulp32)                     # re-exported to the two test files

IN_SCALES = (1.0, 1.0 / 0.18215)
TIMESTEPS = (0.0, 1.0, 34.0, 925.0, 958.0, 999.0)
POSE_MEAN, POSE_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def _fma(a64, b64, acc32):
    """The emulations' fmaf: float64 product (exact), float64 sum, rounded to fp32."""
    return (a64 * b64 + acc32.astype(F64)).astype(F32)


def _rng(*key):
    return np.random.default_rng([ord(ch) for ch in "/".join(str(k) for k in key)])


# ------------------------------------------------------------------------------------------------------------------------------------
# 3x3, pad-1 windows
# ------------------------------------------------------------------------------------------------------------------------------------
def _windows(x, stride=1, pad_mode="constant", rows_from_2y=False):
    """x [B][H][W][C] -> [B][oh][ow][3][3][C], the window of output (y, x) starting at input (stride y - 1, stride x - 1)."""
    h, w = x.shape[1], x.shape[2]
    xp = np.pad(x, ((0, 0), (0, 2) if rows_from_2y else (1, 1), (1, 1), (0, 0)), mode=pad_mode)
    v = sliding_window_view(xp, (3, 3), axis=(1, 2))[:, ::stride, ::stride]
    return v[:, :(h + stride - 1) // stride, :(w + stride - 1) // stride].transpose(0, 1, 2, 4, 5, 3)


def _conv_ref(win, wt, bias):
    """float64 (z, S) [B][oh][ow][cout] of windows [B][oh][ow][3][3][C] with wt [cout][3][3][C] and bias [cout]."""
    win, wt, bias = np.asarray(win, F64), np.asarray(wt, F64), np.asarray(bias, F64)
    flat, wf = win.reshape(-1, wt[0].size), wt.reshape(wt.shape[0], -1)
    z = (flat @ wf.T + bias).reshape(win.shape[:3] + (wt.shape[0],))
    s = (np.abs(flat) @ np.abs(wf).T + np.abs(bias)).reshape(z.shape)
    return z, s


def _conv_emu(win, wt, bias, order, drop_last_tap=False):
    """fp32 [B][oh][ow][cout]: the bias, then one fmaf per tap in `order` (a list of (ky, kx, ci))."""
    win64, wt64 = np.asarray(win, F32).astype(F64), np.asarray(wt, F32).astype(F64)
    acc = np.broadcast_to(np.asarray(bias, F32), win.shape[:3] + (wt.shape[0],)).copy()
    for ky, kx, ci in (order[:-1] if drop_last_tap else order):
        acc = _fma(win64[:, :, :, ky, kx, ci, None], wt64[:, ky, kx, ci], acc)
    return acc


def _t_bound(ref, e, dt):
    return e + np.maximum(U_T[dt] * (np.abs(ref) + e), SUB_T[dt])


STEM_ORDER = [(ky, kx, ci) for ky in range(3) for kx in range(3) for ci in range(3)]


# ------------------------------------------------------------------------------------------------------------------------------------
# the stems: idb_arcface_stem (stride 1, PReLU, second output) and idb_pose_stem (stride 2, ReLU)
# ------------------------------------------------------------------------------------------------------------------------------------
ASTEM_SHAPES = ((1, 1, 1), (3, 3, 5), (2, 7, 33), (1, 2, 256))             # W * 8 > 256: a second pass of the pixel loop; 256: the LDS limit
PSTEM_SHAPES = ((1, 1, 1), (2, 4, 6), (3, 5, 7), (1, 9, 65), (1, 2, 512), (1, 3, 511))
ENTRIES = ("u8", "f32")               # uint8 NHWC with the normalisation fused | fp32 NCHW taken as is


@lru_cache(maxsize=None)
def stem_params(kind: str):
    """(weight fp32 [64][3][3][3] as [cout][ky][kx][cin], bias [64], slope [64], out2 scale [64], out2 shift [64]); the slopes are
    all distinct, of both signs and on both sides of 1 in magnitude."""
    rng = _rng("stem", kind)
    wt = (rng.normal(size=(64, 3, 3, 3)) * 0.3).astype(F32)
    bias = (rng.normal(size=64) * 0.05).astype(F32)
    slope = np.concatenate([np.linspace(0.05, 0.45, 40), -np.linspace(1.05, 1.6, 24)])[rng.permutation(64)].astype(F32)
    s2 = rng.uniform(0.5, 1.5, size=64).astype(F32) * np.where(np.arange(64) % 5 == 0, -1, 1).astype(F32)
    b2 = (rng.normal(size=64) * 0.3).astype(F32)
    return wt, bias, slope, s2, b2


@lru_cache(maxsize=None)
def stem_raw(kind: str, shape, entry: str) -> np.ndarray:
    """What the host hands the kernel: uint8 [B][H][W][3], or fp32 [B][3][H][W] (values of order 1 that no 16-bit format holds)."""
    b, h, w = shape
    rng = _rng("stemx", kind, shape, entry)
    if entry == "u8":
        return rng.integers(0, 256, size=(b, h, w, 3), dtype=np.uint8)
    return rng.normal(size=(b, 3, h, w)).astype(F32)


def stem_taps(kind, shape, entry, dt, defect=None) -> np.ndarray:
    """fp32 [B][H][W][3]: the values the kernel stages in LDS, restated one fp32 operation at a time."""
    b, h, w = shape
    raw = stem_raw(kind, shape, entry)
    swapped = defect == "layout_swapped"
    if entry == "u8":
        v = (raw.reshape(b, 3, h, w).transpose(0, 2, 3, 1) if swapped else raw).astype(F32)
        v = v / F32(255)
        if kind == "arcface":
            v = (v - F32(0.5)) / F32(0.5)
        else:
            ch = (np.arange(3) + (1 if defect == "norm_other_channel" else 0)) % 3
            v = (v - np.asarray(POSE_MEAN, F32)[ch]) / np.asarray(POSE_STD, F32)[ch]
    else:
        v = raw.reshape(b, h, w, 3) if swapped else raw.transpose(0, 2, 3, 1)
    if kind == "arcface" and defect != "input_unrounded":
        v = round_T(v, dt)
    return np.ascontiguousarray(v, F32)


def stem_reference(kind, shape, entry, dt, e_scale=1.0):
    """(out float64 [B][oh][ow][64], bound, pre-activation z): the convolution of the kernel's taps from its definition, then PReLU
    (ArcFace) or ReLU (pose).  e_scale shrinks the fp32 part e of the bound (the CPU half holds the emulations to e / 2; the rounding
    to T is sharp, a correctly rounded value attains u_T |ref|, so that term cannot be halved)."""
    wt, bias, slope, _, _ = stem_params(kind)
    z, s = _conv_ref(_windows(stem_taps(kind, shape, entry, dt).astype(F64), 1 if kind == "arcface" else 2), wt, bias)
    if kind == "arcface":
        sl = slope.astype(F64)
        out, amp = np.where(z >= 0, z, z * sl), np.maximum(1.0, np.abs(sl))
    else:
        out, amp = np.maximum(z, 0.0), 1.0
    return out, _t_bound(out, e_scale * gamma(27 + 1) * s * amp, dt), z


def emulate_stem(kind, shape, entry, dt, defect=None):
    """(out, out2 or None): fp32 arrays holding the T values the kernel would store."""
    wt, bias, slope, s2, b2 = stem_params(kind)
    taps = stem_taps(kind, shape, entry, dt, defect)
    win = _windows(taps, 1 if kind == "arcface" else 2, "edge" if defect == "replicate_pad" else "constant", defect == "window_from_2y")
    acc = _conv_emu(win, wt, bias, STEM_ORDER, defect == "tap_dropped")
    if kind == "pose":
        return round_T(np.maximum(acc, F32(0)), dt), None
    sl = np.roll(slope, -1) if defect == "slope_neighbour" else slope
    v = np.where(acc > 0 if defect == "prelu_gt" else acc >= 0, acc, acc * sl)
    out = round_T(v, dt)
    return out, out2_of(v if defect == "out2_unrounded" else out, s2, b2, dt)


def out2_of(out32, s2, b2, dt):
    """The second output the ArcFace stem must store for the `out` it stored: fma rounded once to fp32, then once to T."""
    return round_T(fma32(out32, s2, b2).reshape(np.shape(out32)), dt)


# ------------------------------------------------------------------------------------------------------------------------------------
# idb_conv_in
# ------------------------------------------------------------------------------------------------------------------------------------
CONV_IN_SHAPES = ((1, 4, 1, 1, 8, 1), (2, 1, 5, 7, 8, 1), (3, 3, 16, 17, 24, 2), (2, 4, 9, 31, 16, 2))     # (batch, cin, H, W, cout, rep)


@dataclass(frozen=True)
class ConvInCase:
    shape: Tuple[int, int, int, int, int, int]
    scale: int                        # index into IN_SCALES
    pre: bool

    @property
    def name(self):
        return "b{}_cin{}_{}x{}_cout{}_rep{}".format(*self.shape) + f"_{'vae_scale' if self.scale else 'scale1'}_{'pre' if self.pre else 'nopre'}"

    @property
    def in_scale(self) -> float:
        """As the ABI receives it: fp32."""
        return float(F32(IN_SCALES[self.scale]))


def conv_in_cases() -> List[ConvInCase]:
    return [ConvInCase(s, sc, pre) for s in CONV_IN_SHAPES for sc in (0, 1) for pre in (False, True)]


@lru_cache(maxsize=None)
def conv_in_inputs(case: ConvInCase):
    """(x fp32 [batch][cin][H][W], w [cout][cin][3][3], bias [cout], pre_w [cin][cin] or None, pre_b [cin] or None)."""
    b, cin, h, w, cout, _ = case.shape
    rng = _rng("conv_in", case.shape)
    x = rng.normal(size=(b, cin, h, w)).astype(F32)
    wt = (rng.normal(size=(cout, cin, 3, 3)) * 0.3).astype(F32)
    bias = (rng.normal(size=cout) * 0.1).astype(F32)
    pre_w = (rng.normal(size=(cin, cin)) * 0.6).astype(F32)
    pre_b = (rng.normal(size=cin) * 0.5 + np.where(np.arange(cin) % 2, -1.0, 1.0)).astype(F32)
    return x, wt, bias, (pre_w if case.pre else None), (pre_b if case.pre else None)


def conv_in_roundings(case: ConvInCase) -> int:
    """K + 1 + a of the module docstring."""
    cin = case.shape[1]
    return 9 * cin + 1 + (1 if case.in_scale != 1.0 else 0) + (cin + 1 if case.pre else 0)


def conv_in_reference(case: ConvInCase, dt, e_scale=1.0):
    """(out float64 [rep][batch][H][W][cout], bound); e_scale as in stem_reference."""
    x, wt, bias, pre_w, pre_b = conv_in_inputs(case)
    v = x.astype(F64).transpose(0, 2, 3, 1) * case.in_scale                # NHWC
    a = np.abs(v)
    if case.pre:
        v = v @ pre_w.astype(F64).T + pre_b.astype(F64)
        a = a @ np.abs(pre_w.astype(F64)).T + np.abs(pre_b.astype(F64))
    w9 = wt.transpose(0, 2, 3, 1)                                         # [cout][ky][kx][cin]
    z, _ = _conv_ref(_windows(v), w9, bias)
    _, s = _conv_ref(_windows(a), np.abs(w9), np.abs(bias))
    rep = case.shape[5]
    out = np.broadcast_to(z, (rep,) + z.shape)
    return out, np.broadcast_to(_t_bound(z, e_scale * gamma(conv_in_roundings(case)) * s, dt), out.shape)


def emulate_conv_in(case: ConvInCase, dt, defect=None):
    """fp32 [rep][batch][H][W][cout] holding T values: x * in_scale, the pre-conv as fmaf's onto pre_b, zero padding, the taps as
    fmaf's onto the bias in (ci, tap) order, one rounding; every copy of `rep` the same."""
    x, wt, bias, pre_w, pre_b = conv_in_inputs(case)
    cin, rep = case.shape[1], case.shape[5]
    v = x.transpose(0, 2, 3, 1) * F32(case.in_scale)
    if case.pre:
        raw64, acc = v.astype(F64), np.broadcast_to(pre_b, v.shape).copy()
        for cj in range(cin):
            acc = _fma(pre_w[:, cj].astype(F64), raw64[..., cj, None], acc)
        v = acc
    win = _windows(v)
    if case.pre and defect == "pre_b_on_pad":
        win = np.where(_windows(np.ones(v.shape[:3] + (1,), bool)), win, pre_b)
    order = [(t // 3, t % 3, ci) for ci in range(cin) for t in range(9)]
    out = round_T(_conv_emu(win, wt.transpose(0, 2, 3, 1), bias, order, defect == "tap_dropped"), dt)
    out = np.broadcast_to(out, (rep,) + out.shape).copy()
    if defect == "rep1_unwritten" and rep > 1:
        out[1] = np.nan
    return out


# ------------------------------------------------------------------------------------------------------------------------------------
# idb_linear_f32
# ------------------------------------------------------------------------------------------------------------------------------------
LINEAR_SHAPES = ((1, 1, 1), (8, 4, 64), (9, 5, 65), (30, 7, 130), (17, 13, 320))       # (m, n, k)


@dataclass(frozen=True)
class LinearCase:
    shape: Tuple[int, int, int]
    silu: bool
    bias: bool

    @property
    def name(self):
        return "m{}_n{}_k{}".format(*self.shape) + f"_{'silu' if self.silu else 'plain'}_{'bias' if self.bias else 'nobias'}"


def linear_cases() -> List[LinearCase]:
    return [LinearCase(s, silu, bias) for s in LINEAR_SHAPES for silu in (False, True) for bias in (True, False)]


@lru_cache(maxsize=None)
def linear_inputs(case: LinearCase):
    m, n, k = case.shape
    rng = _rng("linear", case.shape)
    x = (rng.normal(size=(m, k)) * 1.5).astype(F32)
    wt = rng.normal(size=(n, k)).astype(F32)
    bias = rng.normal(size=n).astype(F32)
    return x, wt, (bias if case.bias else None)


def silu32(x):
    """The kernel's x * rcp(1 + __expf(-x)) in numpy float32."""
    x = np.asarray(x, F32)
    return x * (F32(1) / (F32(1) + np.exp(-x)))


def silu64(x):
    x = np.asarray(x, F64)
    return x / (1.0 + np.exp(-x))


def silu_allowance(x) -> Tuple[float, float]:
    """(relative allowance max(3 r, 4 u), r) for the case's x."""
    ref = silu64(x)
    r = float((np.abs(silu32(x).astype(F64) - ref) / np.abs(ref)).max())
    return max(3.0 * r, 4.0 * U), r


def linear_reference(case: LinearCase):
    """(y float64 [m][n], bound)."""
    x, wt, bias = linear_inputs(case)
    k = case.shape[2]
    xv, allow = x.astype(F64), 0.0
    if case.silu:
        xv, (allow, _) = silu64(x), silu_allowance(x)
    b = np.zeros(wt.shape[0]) if bias is None else bias.astype(F64)
    s = np.abs(xv) @ np.abs(wt.astype(F64)).T
    return xv @ wt.astype(F64).T + b, gamma(k + 7) * (s * (1.0 + allow) + np.abs(b)) + allow * s


def emulate_linear(case: LinearCase, defect=None):
    """fp32 [m][n]: lane l sums k = l, l + 64, ... as fmaf's, the xor shuffle tree 32, 16, ... 1, lane 0 adds the bias."""
    x, wt, bias = linear_inputs(case)
    m, n, k = case.shape
    xv = (silu32(x) if case.silu else x).astype(F64)
    kend = k - k % 64 if defect == "lane_tail_skipped" else k
    acc = np.zeros((m, n, 64), F32)
    for base in range(0, kend, 64):
        idx = np.arange(base, min(base + 64, kend))
        acc[:, :, idx - base] = _fma(xv[:, None, idx], wt.astype(F64)[None, :, idx], acc[:, :, idx - base])
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, :, np.arange(64) ^ o]
    y = acc[:, :, 0] + (F32(0) if bias is None else bias)
    if defect == "last_column_skipped" and n % 4:
        y[:, n - 1] = np.nan
    return y


# ------------------------------------------------------------------------------------------------------------------------------------
# idb_arcface_head
# ------------------------------------------------------------------------------------------------------------------------------------
HEAD_SHAPES = ((1, 64, 32), (5, 64, 256), (65, 128, 512), (3, 64, 544), (130, 512, 800), (2, 512, 25088))      # (M, N, K)
HEAD_SLICES = {(1, 64, 32): [1], (5, 64, 256): [8], (65, 128, 512): [8, 8], (3, 64, 544): [9, 8], (130, 512, 800): [9, 9, 7],
               (2, 512, 25088): [13] * 60 + [4]}                         # K chunks of 32 per slice, worked out by hand from head_splits


def head_splits(m: int, n: int, k: int) -> int:
    """csrc/idb_arcface.hip head_splits, restated: about 512 workgroups, at least 8 chunks of 32 per slice, no empty slice."""
    tiles = ((m + 63) // 64) * (n // 64)
    s = (512 + tiles - 1) // tiles
    nchunks = k // 32
    s = max(1, min(s, nchunks // 8))
    per = (nchunks + s - 1) // s
    return (nchunks + per - 1) // per


def head_slices(m, n, k) -> List[int]:
    splits, nchunks = head_splits(m, n, k), k // 32
    per = (nchunks + splits - 1) // splits
    return [min(nchunks, (z + 1) * per) - z * per for z in range(splits)]


def head_workspace_bytes(m, n, k) -> int:
    return head_splits(m, n, k) * m * n * 4


@dataclass(frozen=True)
class HeadCase:
    shape: Tuple[int, int, int]
    bias: bool

    @property
    def name(self):
        return "M{}_N{}_K{}".format(*self.shape) + ("_bias" if self.bias else "_nobias")


def head_cases() -> List[HeadCase]:
    return [HeadCase(s, b) for s in HEAD_SHAPES for b in (True, False)]


@lru_cache(maxsize=None)
def head_inputs(shape, dt):
    """(x fp32 [M][K] holding T values, w fp32 [N][K], bias [N])."""
    m, n, k = shape
    rng = _rng("head", shape)
    x = round_T(rng.normal(size=(m, k)).astype(F32), dt)
    wt = (rng.normal(size=(n, k)) / np.sqrt(k)).astype(F32)
    return x, wt, (rng.normal(size=n) * 0.3).astype(F32)


def head_reference(case: HeadCase, dt):
    """(y float64 [M][N], bound)."""
    x, wt, bias = head_inputs(case.shape, dt)
    m, n, k = case.shape
    b = bias.astype(F64) if case.bias else np.zeros(n)
    s = np.abs(x.astype(F64)) @ np.abs(wt.astype(F64)).T + np.abs(b)
    return x.astype(F64) @ wt.astype(F64).T + b, gamma(k + head_splits(m, n, k) + 1) * s


def emulate_head(case: HeadCase, dt, defect=None):
    """fp32 [M][N]: per slice a chain of fmaf's over ascending k from 0, then the slices added to 0 in ascending order, then the bias."""
    x, wt, bias = head_inputs(case.shape, dt)
    m, n, k = case.shape
    rows = np.arange(m)
    x64 = x.astype(F64)[np.where(rows >= 64, rows - 64, rows) if defect == "row_wrap64" else rows]
    w64 = wt.astype(F64)
    b = bias if case.bias else np.zeros(n, F32)
    partial, c0 = [], 0
    for z, chunks in enumerate(head_slices(m, n, k)):
        c1 = c0 + chunks - (1 if defect == "last_chunk_skipped" and z == len(head_slices(m, n, k)) - 1 else 0)
        acc = np.zeros((m, n), F32)
        for kk in range(c0 * 32, c1 * 32):
            acc = _fma(x64[:, kk, None], w64[None, :, kk], acc)
        partial.append(acc)
        c0 += chunks
    s = np.zeros((m, n), F32)
    for z, p in enumerate(partial[:-1] if defect == "last_slice_skipped" else partial):
        s = s + p
        if defect == "bias_per_slice" and z:
            s = s + b
    return s + b


# ------------------------------------------------------------------------------------------------------------------------------------
# idb_pose_head
# ------------------------------------------------------------------------------------------------------------------------------------
PHEAD_SHAPES = ((1, 1, 8), (2, 7, 64), (3, 49, 2048), (2, 50, 2056))       # (B, HW, C); C / 8 = 257: a second pass of the channel-group loop
R_FLOOR, ANG_FLOOR = 4 * 2.0 ** -23, 4 * 2.0 ** -16                         # 4 ulp32(1), 4 ulp32(180)


def six_post(o6, dtype=F64):
    """(R [B][9] row-major with columns x, y, z; angles [B][3] pitch, yaw, roll in degrees) of six-vectors [B][6], one operation at a
    time in `dtype`: x = a / |a|, z = normalize(x cross b), y = z cross x, sy = sqrt(R00^2 + R10^2), pitch = atan2(R21, R22),
    yaw = atan2(-R20, sy), roll = atan2(R10, R00) (the regular branch, sy >= 1e-6)."""
    o6 = np.asarray(o6, dtype)
    a, b = o6[:, :3], o6[:, 3:]
    norm = lambda v: np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2])[:, None]      # noqa: E731
    cross = lambda p, q: np.stack([p[:, 1] * q[:, 2] - p[:, 2] * q[:, 1], p[:, 2] * q[:, 0] - p[:, 0] * q[:, 2],      # noqa: E731
                                   p[:, 0] * q[:, 1] - p[:, 1] * q[:, 0]], axis=1)
    x = a / norm(a)
    z = cross(x, b)
    z = z / norm(z)
    y = cross(z, x)
    rot = np.stack([x, y, z], axis=2).reshape(-1, 9)
    sy = np.sqrt(x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1])
    deg = dtype(180.0) / dtype(np.pi)
    ang = np.stack([np.arctan2(y[:, 2], z[:, 2]) * deg, np.arctan2(-x[:, 2], sy) * deg, np.arctan2(x[:, 1], x[:, 0]) * deg], axis=1)
    return rot.astype(dtype), ang.astype(dtype)


@lru_cache(maxsize=None)
def phead_targets(shape) -> np.ndarray:
    """float64 [B][6]: a = |a| R[:, 0], b = |b| (cos t R[:, 0] + sin t R[:, 1]) for R = Rz(roll) Ry(yaw) Rx(pitch) with the three angles
    in [-60, 60] degrees (sy = cos yaw >= 0.5), |a|, |b| in [0.5, 2], t in [45, 135] degrees."""
    rng = _rng("phead_target", shape)
    out = []
    for _ in range(shape[0]):
        al, be, ga = np.radians(rng.uniform(-60, 60, size=3))
        rx = np.array([[1, 0, 0], [0, np.cos(al), -np.sin(al)], [0, np.sin(al), np.cos(al)]])
        ry = np.array([[np.cos(be), 0, np.sin(be)], [0, 1, 0], [-np.sin(be), 0, np.cos(be)]])
        rz = np.array([[np.cos(ga), -np.sin(ga), 0], [np.sin(ga), np.cos(ga), 0], [0, 0, 1]])
        r = rz @ ry @ rx
        t, la, lb = np.radians(rng.uniform(45, 135)), rng.uniform(0.5, 2.0), rng.uniform(0.5, 2.0)
        out.append(np.concatenate([la * r[:, 0], lb * (np.cos(t) * r[:, 0] + np.sin(t) * r[:, 1])]))
    return np.asarray(out)


@lru_cache(maxsize=None)
def phead_inputs(shape, dt):
    """(x fp32 [B][HW][C] holding T values, w fp32 [6][C], bias fp32 [6]): post-ReLU-like features; the bias places the six-vector on
    phead_targets (to fp32 rounding)."""
    b, hw, c = shape
    rng = _rng("phead", shape)
    x = round_T(np.maximum(rng.normal(size=(b, hw, c)) + 0.3, 0).astype(F32), dt)
    wt = (rng.normal(size=(6, c)) / c).astype(F32)
    mean0 = x[0].astype(F64).mean(0)
    bias = (phead_targets(shape)[0] - wt.astype(F64) @ mean0).astype(F32)
    # one bias serves the batch: samples 1.. get their targets through a per-sample shift of their features' mean along w's pseudo-inverse
    for i in range(1, b):
        need = phead_targets(shape)[i] - bias.astype(F64) - wt.astype(F64) @ x[i].astype(F64).mean(0)
        shift = np.linalg.lstsq(wt.astype(F64), need, rcond=None)[0]
        x[i] = round_T((x[i].astype(F64) + shift).astype(F32), dt)
    return x, wt, bias


def phead_linear_reference(shape, dt):
    """(six-vector float64 [B][6], delta6)."""
    x, wt, bias = phead_inputs(shape, dt)
    _, hw, c = shape
    w64, b64 = wt.astype(F64), bias.astype(F64)
    o6 = x.astype(F64).mean(1) @ w64.T + b64
    return o6, gamma(hw + c + 12) * (np.abs(x.astype(F64)).mean(1) @ np.abs(w64).T + np.abs(b64))


def phead_reference(shape, dt):
    """(R float64 [B][9], its tolerance, angles [B][3], their tolerance, six-vector) as the module docstring derives them."""
    o6, d6 = phead_linear_reference(shape, dt)
    rot, ang = six_post(o6)
    prop_r, prop_a, h = np.zeros_like(rot), np.zeros_like(ang), 1e-6
    for j in range(6):
        e = np.zeros(6)
        e[j] = h
        (r1, a1), (r0, a0) = six_post(o6 + e), six_post(o6 - e)
        prop_r += np.abs(r1 - r0) / (2 * h) * d6[:, j, None]
        prop_a += np.abs(a1 - a0) / (2 * h) * d6[:, j, None]
    o32 = o6.astype(F32)
    (r32, a32), (r64, a64) = six_post(o32, F32), six_post(o32.astype(F64))
    emu_r = max(3.0 * float(np.abs(r32.astype(F64) - r64).max()), R_FLOOR)
    emu_a = max(3.0 * float(np.abs(a32.astype(F64) - a64).max()), ANG_FLOOR)
    return rot, 2.0 * prop_r + emu_r, ang, 2.0 * prop_a + emu_a, o6


def emulate_phead(shape, dt, defect=None):
    """(R fp32 [B][9], angles fp32 [B][3]): thread t owns channel groups t, t + 256, ...: the pixel sum in ascending order, one
    division, fmaf's into its six partial sums; the xor shuffle tree per wave, (w0 + w1) + (w2 + w3), the bias; then six_post in fp32."""
    x, wt, bias = phead_inputs(shape, dt)
    b, hw, c = shape
    s = np.zeros((b, c), F32)
    for p in range(hw):
        s = s + x[:, p]
    m64 = (s / F32(hw - 1 if defect == "pool_div_hw_minus_1" else hw)).astype(F64)
    w64 = wt.astype(F64)
    d = np.zeros((b, 256, 6), F32)
    groups = min(c // 8, 256) if defect == "groups_ge_256_skipped" else c // 8
    for g0 in range(0, groups, 256):
        cg = np.arange(g0, min(g0 + 256, groups))
        for e in range(8):
            ch = cg * 8 + e
            d[:, cg - g0] = _fma(m64[:, ch, None], w64[:, ch].T[None], d[:, cg - g0])
    d = d.reshape(b, 4, 64, 6)
    for o in (32, 16, 8, 4, 2, 1):
        d = d + d[:, :, np.arange(64) ^ o]
    red = d[:, :, 0]
    o6 = ((red[:, 0] + red[:, 1]) + (red[:, 2] + red[:, 3])) + bias
    return six_post(o6, F32)


# ------------------------------------------------------------------------------------------------------------------------------------
# idb_timestep_sinusoid
# ------------------------------------------------------------------------------------------------------------------------------------
SIN_SHAPES = ((1, 2), (5, 6), (6, 320))               # (n, dim)
SIN_FLOOR = 2 * 2.0 ** -23                            # 2 ulp32(1)


def sin_inputs(n: int) -> np.ndarray:
    """The last n of TIMESTEPS, fp32."""
    return np.asarray(TIMESTEPS[-n:], F32)


def sin_reference(n, dim):
    """float64 [n][dim]: cos(t f_j) | sin(t f_j), f_j = exp(-ln(10000) j / (dim / 2)) (diffusers get_timestep_embedding, flip_sin_to_cos)."""
    half = dim // 2
    a = sin_inputs(n).astype(F64)[:, None] * np.exp(-np.log(10000.0) * np.arange(half) / half)[None]
    return np.concatenate([np.cos(a), np.sin(a)], axis=1)


def emulate_sin(n, dim, defect=None):
    half = dim // 2
    freq = np.exp(-np.log(F32(10000.0)) * np.arange(half).astype(F32) / F32(half))
    a = sin_inputs(n)[:, None] * freq[None].astype(F32)
    parts = [np.cos(a), np.sin(a)]
    return np.concatenate(parts[::-1] if defect == "halves_swapped" else parts, axis=1).astype(F32)


def sin_bound(n, dim):
    """(reference, the case's bar, the emulation's worst error)."""
    ref = sin_reference(n, dim)
    emu = float(np.abs(emulate_sin(n, dim).astype(F64) - ref).max())
    return ref, max(3.0 * emu, SIN_FLOOR), emu


# ------------------------------------------------------------------------------------------------------------------------------------
# defects and the named case each must fail
# ------------------------------------------------------------------------------------------------------------------------------------
HARMLESS = ("prelu_gt",)
DEFECTS = ("tap_dropped", "replicate_pad", "layout_swapped", "window_from_2y", "norm_other_channel", "slope_neighbour", "out2_unrounded",
           "input_unrounded", "pre_b_on_pad", "rep1_unwritten", "last_chunk_skipped", "last_slice_skipped", "bias_per_slice", "row_wrap64",
           "lane_tail_skipped", "last_column_skipped", "pool_div_hw_minus_1", "groups_ge_256_skipped", "halves_swapped", "prelu_gt")
DEFECT_CASES = {
    "tap_dropped": ("conv_in", ConvInCase((2, 1, 5, 7, 8, 1), 0, False), "f16"),
    "replicate_pad": ("arcface_stem", (3, 3, 5), "u8", "bf16"),
    "layout_swapped": ("pose_stem", (2, 4, 6), "f32", "f16"),
    "window_from_2y": ("pose_stem", (3, 5, 7), "u8", "bf16"),
    "norm_other_channel": ("pose_stem", (1, 9, 65), "u8", "bf16"),
    "slope_neighbour": ("arcface_stem", (2, 7, 33), "f32", "bf16"),
    "out2_unrounded": ("arcface_out2", (2, 7, 33), "u8", "f16"),
    "input_unrounded": ("arcface_stem", (2, 7, 33), "u8", "f16"),
    "pre_b_on_pad": ("conv_in", ConvInCase((3, 3, 16, 17, 24, 2), 1, True), "bf16"),
    "rep1_unwritten": ("conv_in", ConvInCase((3, 3, 16, 17, 24, 2), 0, False), "f16"),
    "last_chunk_skipped": ("head", HeadCase((5, 64, 256), True), "f16"),
    "last_slice_skipped": ("head", HeadCase((3, 64, 544), True), "bf16"),
    "bias_per_slice": ("head", HeadCase((130, 512, 800), True), "f16"),
    "row_wrap64": ("head", HeadCase((65, 128, 512), False), "bf16"),
    "lane_tail_skipped": ("linear", LinearCase((9, 5, 65), False, True)),
    "last_column_skipped": ("linear", LinearCase((30, 7, 130), True, False)),
    "pool_div_hw_minus_1": ("pose_head", (2, 7, 64), "f16"),
    "groups_ge_256_skipped": ("pose_head", (2, 50, 2056), "bf16"),
    "halves_swapped": ("sinusoid", 5, 6),
}


def defect_fails(defect: str) -> bool:
    """True when `defect`, injected into the emulation of its named case, violates that case's criterion."""
    kind, *key = DEFECT_CASES[defect]
    if kind in ("arcface_stem", "pose_stem"):
        ref, bound, _ = stem_reference(kind[:-5], *key)
        return not check(emulate_stem(kind[:-5], *key, defect=defect)[0], ref, bound)[0]
    if kind == "arcface_out2":
        _, _, _, s2, b2 = stem_params("arcface")
        out, out2 = emulate_stem("arcface", *key, defect=defect)
        return not np.array_equal(to_bits(out2, key[2]), to_bits(out2_of(out, s2, b2, key[2]), key[2]))
    if kind == "conv_in":
        ref, bound = conv_in_reference(*key)
        return not check(emulate_conv_in(*key, defect=defect), ref, bound)[0]
    if kind == "head":
        ref, bound = head_reference(*key)
        return not check(emulate_head(*key, defect=defect), ref, bound)[0]
    if kind == "linear":
        ref, bound = linear_reference(*key)
        return not check(emulate_linear(*key, defect=defect), ref, bound)[0]
    if kind == "pose_head":
        rot, tol_r, ang, tol_a, _ = phead_reference(*key)
        r, a = emulate_phead(*key, defect=defect)
        return not (check(r, rot, tol_r)[0] and check(a, ang, tol_a)[0])
    ref, bar, _ = sin_bound(*key)
    return not check(emulate_sin(*key, defect=defect), ref, bar)[0]
