"""The test matrix of the MTCNN detector kernels (csrc/idb_mtcnn.hip: idb_crop_resize_area_u8, idb_conv2d_f32, idb_maxpool2d_f32,
idb_softmax_pairs_f32, idb_nms_mask), shared by test_detect_matrix_cpu.py (references against torch, criteria, teeth, argument checks) and
test_detect_matrix_gpu.py (launch + compare): cases, input recipes, float64 references written from the definitions, emulations of the
kernels' fp32 arithmetic, injectable defects and the bounds; the verdicts are matrix_common.py's.  numpy only, no GPU.

Criteria (u = 2^-24, derived from the arithmetic, no constant was tuned):

  area      The kernel sums the window's uint8 values in fp32 (exact while 255 * window pixels < 2^24: area_sum_exact, asserted for every
            case), divides by the pixel count, subtracts `sub`, multiplies by `mul`.  csrc/Makefile compiles with -O3 and nothing that relaxes
            fp32 division (no -ffast-math, no -fno-hip-fp32-correctly-rounded-divide-sqrt): the division is correctly rounded.  With q the
            float64 mean:   |err| <= (u |q| + u |q - sub|) |mul| + u |out|.
  conv      K = cin * kh * kw sequential fmaf's onto the bias, at most one PReLU multiply; S = sum |x w| + |bias| per output:
                            |err| <= gamma_(K+1) S max(1, |slope|),   gamma_n = n u / (1 - n u)   (forward bound of a recursive sum).
  pool      bit equality (a maximum rounds nothing).
  softmax   p1 = 1 / (1 + exp(a0 - a1)) in float64.  The kernel's steps (max, two subtractions, two expf, one addition, one division) are
            evaluated in numpy float32 (emulate_softmax); per case the bar is 3x that emulation's worst error in ulps of p1, at least 2 ulp
            (3: device expf against numpy's, the factor the DINOv2 tests use for emulated error).  ulp = the fp32 spacing at |p1|, 2^-149
            below the normal range: the sweep reaches outputs that are fp32 subnormals (a1 - a0 = -90) and that round to 0 (-104, -200).
  nms       the bit matrix restated in numpy float32, one operation at a time in the kernel's documented order (nms_mask_fp32): exact by
            construction, so the bar is bit equality; words left of the diagonal are zero.
  decisions p >= 0.6 and p > 0.7 (the host compares the fp32 probability with the threshold as fp32: thresholds(); the distance of that
            fp32 threshold from the decimal one, 2.4e-8 and 1.2e-8, is added to the element's bound) and the suppression bits: wherever
            float64 is further from the threshold than the element's bound the GPU decision must be float64's.  Elements closer than
            that are undecided (for the suppression bits: pairs where the fp32 restatement and float64 disagree); at most 1 % of a case
            (UNDECIDED_CAP), which is a condition on the inputs that test_detect_matrix_cpu.py asserts.

The image sizes: the 3-channel images are 61 x 45; the 1- and 4-channel images are 58 x 64 so that a 50 x 53 box fits into them (it fits
into no orientation of 61 x 45).  The ramp image's value is (2 y + 3 x + 37 c + 11 image) mod 256: a window shifted by one row or column
moves the mean by 2 or 3 whole levels, 1e5 times the bound.

DEFECTS lists what is injected into the references on the CPU and DEFECT_CASES the named case each one must fail under the criteria above;
`prelu_gt` (PReLU on > instead of >=) differs only at an accumulator of exactly 0, where 0 * slope is 0 again: HARMLESS."""
from dataclasses import dataclass
from functools import lru_cache
from typing import Dict, List, Optional, Tuple

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

from matrix_common import F32, GUARD, NAN32, U, bit_equal, check, describe, gamma, ulp32  # noqa: F401  (re-exported to the two test files)

UNDECIDED_CAP = 0.01
THR_P, THR_RO = 0.6, 0.7              # P-Net keeps p >= 0.6, R- and O-Net keep p > 0.7
SUB, MUL = 127.5, 0.0078125           # the detector's normalisation: (x - 127.5) / 128
WORD_GUARD = 0xDEADBEEFCAFEF00D       # the guards' pattern around the uint64 mask


def thresholds() -> Tuple[float, float]:
    """The thresholds as the host applies them: `prob_np >= 0.6` on an fp32 array compares in fp32."""
    return float(F32(THR_P)), float(F32(THR_RO))


def decisions(got32, ref64, bound, thr_index: int):
    """(GPU decisions, float64 decisions, decided mask) for p >= 0.6 (thr_index 0) or p > 0.7 (1)."""
    t32, t = thresholds()[thr_index], (THR_P, THR_RO)[thr_index]
    got32, ref64 = np.asarray(got32, F32), np.asarray(ref64, np.float64)
    g = got32 >= F32(t32) if thr_index == 0 else got32 > F32(t32)
    r = ref64 >= t if thr_index == 0 else ref64 > t
    decided = np.abs(ref64 - t) > np.asarray(bound, np.float64) + abs(t32 - t)
    return g, r, decided


# ------------------------------------------------------------------------------------------------------------------------------------
# area resize
# ------------------------------------------------------------------------------------------------------------------------------------
AREA_DEFECTS = ("win_end_floor", "win_start_next", "chan_stride3")


@lru_cache(maxsize=None)
def area_images() -> Dict[str, np.ndarray]:
    """uint8 [2][h][w][c] image pairs: noise and ramp at 61 x 45 x 3, and at 58 x 64 with 1 and 4 channels."""
    out = {}
    for c, (h, w) in ((3, (61, 45)), (1, (58, 64)), (4, (58, 64))):
        rng = np.random.default_rng(100 + c)
        out[f"noise{c}"] = rng.integers(0, 256, size=(2, h, w, c), dtype=np.uint8)
        i, y, x, ch = np.meshgrid(np.arange(2), np.arange(h), np.arange(w), np.arange(c), indexing="ij")
        out[f"ramp{c}"] = ((2 * y + 3 * x + 37 * ch + 11 * i) % 256).astype(np.uint8)
    return out


@dataclass(frozen=True)
class AreaCase:
    name: str
    image: str                        # key of area_images()
    boxes: Tuple[Tuple[int, int, int, int, int], ...]     # (image, y0, y1, x0, x1), y1 / x1 exclusive
    oh: int
    ow: int

    @property
    def boxes_np(self):
        return np.asarray(self.boxes, np.int32).reshape(-1, 5)


def pyramid_sizes(h, w) -> List[Tuple[int, int]]:
    """int(h s + 1), int(w s + 1) for s = 0.6 * 0.709^k while min(h, w) s >= 12 (mtcnn.pyramid_scales with min_face_size 20)."""
    out, s = [], 0.6
    while min(h, w) * s >= 12:
        out.append((int(h * s + 1), int(w * s + 1)))
        s *= 0.709
    return out


def area_cases() -> List[AreaCase]:
    out = []
    for rec in ("noise", "ramp"):
        im = f"{rec}3"
        full = ((0, 0, 61, 0, 45), (1, 0, 61, 0, 45))
        for k, (oh, ow) in enumerate(pyramid_sizes(61, 45)):
            out.append(AreaCase(f"{im}_pyramid{k}_{oh}x{ow}", im, full, oh, ow))
        out.append(AreaCase(f"{im}_2to1", im, ((0, 0, 60, 0, 44), (1, 1, 61, 1, 45)), 30, 22))
        out.append(AreaCase(f"{im}_4to1", im, ((0, 0, 60, 0, 44), (1, 1, 61, 1, 45)), 15, 11))
        out.append(AreaCase(f"{im}_up_5x7_to_24", im, ((0, 9, 14, 30, 37), (1, 56, 61, 0, 7)), 24, 24))
        out.append(AreaCase(f"{im}_up_13x35_to_48", im, ((1, 40, 53, 3, 38), (0, 0, 13, 10, 45)), 48, 48))
        out.append(AreaCase(f"{im}_1x1_window", im, ((0, 20, 21, 30, 31), (1, 60, 61, 44, 45), (1, 0, 1, 0, 1)), 24, 24))
        out.append(AreaCase(f"{im}_whole_to_1x1", im, full, 1, 1))
        out.append(AreaCase(f"{im}_last_row_col", im, ((1, 40, 61, 20, 45), (1, 3, 61, 10, 45), (0, 3, 60, 10, 44)), 24, 24))
        out.append(AreaCase(f"{im}_n0", im, (), 24, 24))
        for c in (1, 4):
            im = f"{rec}{c}"
            out.append(AreaCase(f"{im}_50x53_to_24", im, ((0, 2, 52, 5, 58), (1, 8, 58, 11, 64)), 24, 24))
            out.append(AreaCase(f"{im}_53x50_to_24", im, ((1, 5, 58, 14, 64), (0, 0, 53, 0, 50)), 24, 24))
            out.append(AreaCase(f"{im}_up_5x7_to_24", im, ((1, 53, 58, 57, 64),), 24, 24))
            out.append(AreaCase(f"{im}_pyramid0", im, ((0, 0, 58, 0, 64), (1, 0, 58, 0, 64)), *pyramid_sizes(58, 64)[0]))
    return out


def area_windows(n_in: int, n_out: int, defect: Optional[str] = None):
    """Window [start, end) of every output index: floor(o in / out), ceil((o + 1) in / out), in integers."""
    o = np.arange(n_out, dtype=np.int64)
    start = (o * n_in) // n_out
    end = -((-(o + 1) * n_in) // n_out)
    if defect == "win_end_floor":
        end = ((o + 1) * n_in) // n_out
    if defect == "win_start_next":
        start = ((o + 1) * n_in) // n_out
    return start, end


def area_window_pixels(case: AreaCase) -> int:
    """The largest window of the case, in pixels."""
    worst = 0
    for _, y0, y1, x0, x1 in case.boxes:
        ys, ye = area_windows(y1 - y0, case.oh)
        xs, xe = area_windows(x1 - x0, case.ow)
        worst = max(worst, int((ye - ys).max() * (xe - xs).max()))
    return worst


def area_sum_exact(case: AreaCase) -> bool:
    return 255 * area_window_pixels(case) < 2 ** 24


def _area_sums(img: np.ndarray, case: AreaCase, defect=None):
    """Exact integer window sums and pixel counts: int64 [n][c][oh][ow], int64 [n][1][oh][ow]."""
    if defect == "chan_stride3":          # the pixel address taken as ((image h + y) w + x) * 3 + channel
        b, h, w, c = img.shape
        i, y, x, ch = np.meshgrid(np.arange(b), np.arange(h), np.arange(w), np.arange(c), indexing="ij")
        img = img.reshape(-1)[(((i * h + y) * w + x) * 3 + ch) % img.size]
    b, h, w, c = img.shape
    integral = np.zeros((b, h + 1, w + 1, c), np.int64)
    integral[:, 1:, 1:] = img.astype(np.int64).cumsum(1).cumsum(2)
    n = len(case.boxes)
    sums, cnt = np.zeros((n, c, case.oh, case.ow), np.int64), np.zeros((n, 1, case.oh, case.ow), np.int64)
    for k, (i, y0, y1, x0, x1) in enumerate(case.boxes):
        ys, ye = area_windows(y1 - y0, case.oh, defect)
        xs, xe = area_windows(x1 - x0, case.ow, defect)
        ys, ye, xs, xe = y0 + ys[:, None], y0 + ye[:, None], x0 + xs[None, :], x0 + xe[None, :]
        ii = integral[i]
        sums[k] = (ii[ye, xe] - ii[ys, xe] - ii[ye, xs] + ii[ys, xs]).transpose(2, 0, 1)
        cnt[k, 0] = (ye - ys) * (xe - xs)
    return sums, cnt


def area_reference(img, case: AreaCase, sub=SUB, mul=MUL, defect=None):
    """(out, bound) float64 [n][c][oh][ow]: the window mean, then (mean - sub) * mul."""
    sums, cnt = _area_sums(img, case, defect)
    with np.errstate(invalid="ignore", divide="ignore"):
        q = sums / cnt.astype(np.float64)
    out = (q - sub) * mul
    return out, (U * np.abs(q) + U * np.abs(q - sub)) * abs(mul) + U * np.abs(out)


def emulate_area(img, case: AreaCase, sub=SUB, mul=MUL):
    """The kernel's steps in fp32: the exact sum as fp32, one division, one subtraction, one multiplication."""
    sums, cnt = _area_sums(img, case)
    return (sums.astype(F32) / cnt.astype(F32) - F32(sub)) * F32(mul)


# ------------------------------------------------------------------------------------------------------------------------------------
# convolution
# ------------------------------------------------------------------------------------------------------------------------------------
CONV_DEFECTS = ("last_tap_dropped", "kykx_swapped", "bias_dropped", "slope0_all", "prelu_gt")


@dataclass(frozen=True)
class ConvCase:
    name: str
    batch: int
    cin: int
    h: int
    w: int
    cout: int
    kh: int
    kw: int
    bias: bool = True
    prelu: bool = True
    recipe: str = "mixed"             # mixed: |x|, |w| of order 1, both signs (with fewer than 8 outputs per channel the odd samples are
                                      # the even ones negated and the bias is 100 times smaller, so that both PReLU branches still occur on every channel);
                                      # negative: every product and the bias negative

    @property
    def k(self):
        return self.cin * self.kh * self.kw

    @property
    def outputs(self):
        return self.batch * self.cout * (self.h - self.kh + 1) * (self.w - self.kw + 1)


def conv_cases() -> List[ConvCase]:
    c = ConvCase
    return [
        # P-Net on a 14 x 17 map, batch 2
        c("pnet_conv1", 2, 3, 14, 17, 10, 3, 3), c("pnet_conv2", 2, 10, 6, 8, 16, 3, 3), c("pnet_conv3", 2, 16, 4, 6, 32, 3, 3),
        c("pnet_conv4_1", 2, 32, 2, 4, 2, 1, 1, prelu=False), c("pnet_conv4_2", 2, 32, 2, 4, 4, 1, 1, prelu=False),
        # R-Net on 24 x 24
        c("rnet_conv1", 2, 3, 24, 24, 28, 3, 3), c("rnet_conv2", 2, 28, 11, 11, 48, 3, 3), c("rnet_conv3", 2, 48, 4, 4, 64, 2, 2),
        c("rnet_dense4_k576", 2, 64, 3, 3, 128, 3, 3), c("rnet_dense5_1", 2, 128, 1, 1, 2, 1, 1, prelu=False),
        c("rnet_dense5_2", 2, 128, 1, 1, 4, 1, 1, prelu=False),
        # O-Net on 48 x 48
        c("onet_conv1", 2, 3, 48, 48, 32, 3, 3), c("onet_conv2", 2, 32, 23, 23, 64, 3, 3), c("onet_conv3", 2, 64, 10, 10, 64, 3, 3),
        c("onet_conv4", 2, 64, 4, 4, 128, 2, 2), c("onet_dense5_k1152", 2, 128, 3, 3, 256, 3, 3),
        c("onet_dense6_1", 2, 256, 1, 1, 2, 1, 1, prelu=False), c("onet_dense6_2", 2, 256, 1, 1, 4, 1, 1, prelu=False),
        c("onet_dense6_3", 2, 256, 1, 1, 10, 1, 1, prelu=False),
        # what the networks never launch
        c("head1x1_prelu", 2, 32, 5, 7, 6, 1, 1), c("head1x1_plain", 2, 32, 5, 7, 6, 1, 1, prelu=False),
        c("no_bias", 2, 5, 7, 9, 4, 3, 3, bias=False), c("no_bias_no_prelu", 1, 4, 5, 5, 3, 2, 2, bias=False, prelu=False),
        c("k2x3", 2, 4, 7, 9, 5, 2, 3), c("k3x1", 2, 4, 7, 9, 5, 3, 1), c("h_eq_kh", 2, 3, 3, 11, 4, 3, 3), c("h_eq_kh_k2x3", 1, 2, 2, 9, 3, 2, 3),
        c("cin1_cout1", 1, 1, 6, 7, 1, 3, 3), c("outputs256", 1, 2, 18, 18, 1, 3, 3), c("outputs257", 1, 2, 3, 259, 1, 3, 3),
        c("all_negative", 2, 6, 8, 9, 7, 3, 3, recipe="negative"),
    ]


def conv_inputs(case: ConvCase, seed=200):
    """(x [b][cin][h][w], w [cout][cin][kh][kw], bias [cout] or None, slope [cout] or None), fp32."""
    rng = np.random.default_rng(seed + sum(map(ord, case.name)))
    x = rng.normal(size=(case.batch, case.cin, case.h, case.w))
    wt = rng.normal(size=(case.cout, case.cin, case.kh, case.kw))
    bias = rng.normal(size=case.cout) * 0.5
    if case.batch * (case.h - case.kh + 1) * (case.w - case.kw + 1) < 8:       # a dense layer: two outputs per channel, made to differ in sign
        x[1::2], bias = -x[0::2], bias * 0.01
    if case.recipe == "negative":
        x, wt, bias = -np.abs(x) - 0.1, np.abs(wt) + 0.1, -np.abs(bias) - 0.1
    slope = np.concatenate([rng.uniform(0.1, 0.4, size=case.cout - case.cout // 2), -rng.uniform(1.0, 1.5, size=case.cout // 2)])
    return (x.astype(F32), wt.astype(F32), bias.astype(F32) if case.bias else None, slope.astype(F32) if case.prelu else None)


def conv_reference(x, wt, bias, slope, defect=None):
    """(out, bound, pre-activation) float64 [b][cout][oh][ow]: the valid convolution from its definition, bias, per-channel PReLU."""
    x, wt = np.asarray(x, np.float64), np.asarray(wt, np.float64)
    b, cin, h, w = x.shape
    cout, _, kh, kw = wt.shape
    oh, ow = h - kh + 1, w - kw + 1
    if defect == "last_tap_dropped":
        wt = wt.copy()
        wt[..., kw - 1] = 0.0
    if defect == "kykx_swapped":          # the filter read at (ci * kh + kx) * kw + ky
        ci, ky, kx = np.meshgrid(np.arange(cin), np.arange(kh), np.arange(kw), indexing="ij")
        wt = wt.reshape(cout, -1)[:, ((ci * kh + kx) * kw + ky) % (cin * kh * kw)]
    win = sliding_window_view(x, (kh, kw), axis=(2, 3)).transpose(0, 2, 3, 1, 4, 5).reshape(b * oh * ow, cin * kh * kw)
    flat = wt.reshape(cout, cin * kh * kw)
    z = (win @ flat.T).reshape(b, oh, ow, cout).transpose(0, 3, 1, 2)
    s = (np.abs(win) @ np.abs(flat).T).reshape(b, oh, ow, cout).transpose(0, 3, 1, 2)
    if bias is not None:
        bb = np.asarray(bias, np.float64)[None, :, None, None]
        s = s + np.abs(bb)
        if defect != "bias_dropped":
            z = z + bb
    out, amp = z, 1.0
    if slope is not None:
        sl = np.asarray(slope, np.float64)
        amp = np.maximum(1.0, np.abs(sl))[None, :, None, None]
        if defect == "slope0_all":
            sl = np.full_like(sl, sl[0])
        sl = sl[None, :, None, None]
        out = np.where(z > 0 if defect == "prelu_gt" else z >= 0, z, z * sl)
    return out, gamma(cin * kh * kw + 1) * s * amp, z


def emulate_conv(x, wt, bias, slope):
    """The kernel's fp32 steps: the bias, K fmaf's in (ci, ky, kx) order (a product of two fp32 values is exact in float64; the sum is
    rounded to float64 and then to fp32), one PReLU multiply."""
    x, wt = np.asarray(x, F32), np.asarray(wt, F32)
    b, cin, h, w = x.shape
    cout, _, kh, kw = wt.shape
    oh, ow = h - kh + 1, w - kw + 1
    acc = np.zeros((b, cout, oh, ow), F32)
    if bias is not None:
        acc += np.asarray(bias, F32)[None, :, None, None]
    for ci in range(cin):
        for ky in range(kh):
            for kx in range(kw):
                xs = x[:, ci, ky:ky + oh, kx:kx + ow].astype(np.float64)[:, None]
                acc = (xs * wt[:, ci, ky, kx].astype(np.float64)[None, :, None, None] + acc.astype(np.float64)).astype(F32)
    if slope is not None:
        acc = np.where(acc >= 0, acc, acc * np.asarray(slope, F32)[None, :, None, None])
    return acc


# ------------------------------------------------------------------------------------------------------------------------------------
# ceil-mode max pooling
# ------------------------------------------------------------------------------------------------------------------------------------
POOL_DEFECTS = ("max_init_zero", "window_unclipped", "last_output_dropped")
POOL_N = tuple(range(1, 14))
POOL_KS = tuple((k, s) for k in (2, 3) for s in (1, 2, 3))
POOL_PLANES = 3                       # all negative | both signs with ties | all negative with -inf entries


def pool_outputs(n: int, k: int, s: int) -> int:
    """Windows start at 0, s, 2 s, ...; the last one is the first that reaches the end of the input, and it must start inside it."""
    t = 0
    while t * s + k < n and (t + 1) * s < n:
        t += 1
    return t + 1


def pool_cases() -> List[Tuple[int, int, int, int]]:
    """(h, w, k, stride): h and w independently over 1..13."""
    return [(h, w, k, s) for k, s in POOL_KS for h in POOL_N for w in POOL_N]


def pool_inputs(h, w, k, s):
    """fp32 [3][h][w]."""
    rng = np.random.default_rng(((h * 16 + w) * 4 + k) * 4 + s)
    x = np.empty((POOL_PLANES, h, w), F32)
    x[0] = -np.abs(rng.normal(size=(h, w))) - 0.25
    x[1] = rng.integers(-3, 4, size=(h, w)) / 2.0
    x[2] = -np.abs(rng.normal(size=(h, w))) - 0.25
    x[2].reshape(-1)[rng.integers(0, h * w, size=max(1, h * w // 4))] = -np.inf
    x[2, h - 1, w - 1] = -np.inf          # the last, clipped window of a 1-wide tail sees nothing else
    return x


def pool_reference(x, k, s, defect=None):
    """fp32 [planes][oh][ow], exact."""
    x = np.asarray(x, F32)
    p, h, w = x.shape
    oh, ow = pool_outputs(h, k, s), pool_outputs(w, k, s)
    if defect == "last_output_dropped":   # floor mode: only windows that lie inside the input
        oh, ow = max(1, (h - k) // s + 1), max(1, (w - k) // s + 1)
    flat = np.concatenate([x.reshape(-1), np.zeros(k * w + k, F32)])
    out = np.empty((p, oh, ow), F32)
    for oy in range(oh):
        for ox in range(ow):
            if defect == "window_unclipped":      # xp[yy * w + xx] for every tap, whatever it lands on
                yy, xx = np.meshgrid(oy * s + np.arange(k), ox * s + np.arange(k), indexing="ij")
                idx = np.arange(p)[:, None] * h * w + (yy * w + xx).reshape(-1)[None, :]
                out[:, oy, ox] = flat[idx].max(1)
            else:
                out[:, oy, ox] = x[:, oy * s:min(oy * s + k, h), ox * s:min(ox * s + k, w)].reshape(p, -1).max(1)
    if defect == "max_init_zero":
        out = np.maximum(out, F32(0))
    return out


# ------------------------------------------------------------------------------------------------------------------------------------
# softmax over a channel pair
# ------------------------------------------------------------------------------------------------------------------------------------
SM_DEFECTS = ("no_max_sub", "p0_returned")
SM_DELTAS = (0.0, 1e-4, 0.4, 0.85, 5.0, 20.0, 90.0, 104.0, 200.0)
SM_OFFSETS = (0.3125, 1e4, -1e4)
SM_HW = (1, 255, 256, 257)
SM_BATCH = 3


def sm_inputs(hw: int, batch: int = SM_BATCH) -> np.ndarray:
    """fp32 [batch][2][hw]: element e = b * hw + i takes a1 - a0 = +-SM_DELTAS and a0 = SM_OFFSETS in turn (hw = 1 starts at the fourth
    delta so that its three elements are not the first three of the sweep)."""
    d = np.array([v for x in SM_DELTAS for v in ((x, -x) if x else (x,))], np.float64)
    e = np.arange(batch * hw) + (3 if hw == 1 else 0)
    a0 = np.array(SM_OFFSETS, np.float64)[(e // d.size) % 3].astype(F32)
    a1 = (a0.astype(np.float64) + d[e % d.size]).astype(F32)
    return np.stack([a0.reshape(batch, hw), a1.reshape(batch, hw)], axis=1)


def sm_reference(x, defect=None):
    """float64 [batch][hw]: p1 = 1 / (1 + exp(a0 - a1)) of the fp32 logits."""
    a0, a1 = np.asarray(x[:, 0], np.float64), np.asarray(x[:, 1], np.float64)
    if defect == "p0_returned":
        a0, a1 = a1, a0
    if defect == "no_max_sub":
        with np.errstate(over="ignore", invalid="ignore"):
            e0, e1 = np.exp(a0.astype(F32)), np.exp(a1.astype(F32))
            return (e1 / (e0 + e1)).astype(np.float64)
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(a0 - a1))


def emulate_softmax(x):
    """The kernel's steps in numpy float32."""
    a0, a1 = np.asarray(x[:, 0], F32), np.asarray(x[:, 1], F32)
    mx = np.maximum(a0, a1)
    e0, e1 = np.exp(a0 - mx), np.exp(a1 - mx)
    return e1 / (e0 + e1)


def sm_bound(x):
    """(float64 reference, per-element bound, the case's bar in ulps, the emulation's worst error in ulps)."""
    ref = sm_reference(x)
    ulp = ulp32(ref)
    emu = float((np.abs(emulate_softmax(x).astype(np.float64) - ref) / ulp).max())
    bar = max(3.0 * emu, 2.0)
    return ref, bar * ulp, bar, emu


# ------------------------------------------------------------------------------------------------------------------------------------
# suppression bit matrix
# ------------------------------------------------------------------------------------------------------------------------------------
NMS_DEFECTS = ("lower_not_skipped", "image_ignored", "nan_swapped")
NMS_N = (1, 63, 64, 65, 128, 129, 577)


@dataclass(frozen=True)
class NmsCase:
    n: int
    method: str                       # "Union" | "Min"
    plus_one: bool
    with_image: bool

    @property
    def name(self):
        return f"n{self.n}_{self.method}_{'plus1' if self.plus_one else 'plus0'}_{'image' if self.with_image else 'noimage'}"

    @property
    def thr(self) -> float:
        """0.5 as at a pyramid level, 0.7 as across levels and after R- / O-Net; fp32, as the ABI receives it."""
        return float(F32(0.5 if self.method == "Union" and not self.plus_one else 0.7))

    @property
    def words(self):
        return (self.n + 63) // 64


def nms_cases() -> List[NmsCase]:
    return [NmsCase(n, m, p, i) for n in NMS_N for m in ("Union", "Min") for p in (False, True) for i in (True, False)]


@lru_cache(maxsize=None)
def nms_inputs(case: NmsCase):
    """(boxes fp32 [n][4] in descending score order, image int32 [n], scores fp32 [n]).  From n = 63 on: an exact duplicate, two identical
    zero-area boxes (0 / 0 without the +1), a pair touching at an edge, and five pairs whose overlap lies -2 .. +2 ulp of the sliding offset
    around thr."""
    n = case.n
    rng = np.random.default_rng(300 + n)
    ctr, wh = rng.uniform(0, 100, size=(n, 2)), rng.uniform(4, 60, size=(n, 2))
    boxes = np.concatenate([ctr - wh / 2, ctr + wh / 2], axis=1).astype(F32)
    image = rng.integers(0, 3, size=n).astype(np.int32)
    if n >= 63:
        boxes[3] = boxes[2]
        boxes[5, 2:] = boxes[5, :2]
        boxes[6] = boxes[5]
        boxes[8] = [boxes[7, 2], boxes[7, 1], boxes[7, 2] + F32(9.5), boxes[7, 3]]
        image[2:9] = 1
        one, thr = (1.0 if case.plus_one else 0.0), case.thr
        a, b, x0, y0 = F32(31.7), F32(12.3), 17.3, F32(40.9)
        share = thr if case.method == "Min" else 2.0 * thr / (1.0 + thr)      # inter / area at which the overlap equals thr
        t = (float(a) + one) * (1.0 - share)
        for q in range(5):                    # of the offsets within 64 ulp of t, the five whose float64 overlap is nearest to thr
            xa = F32(x0 + 3.1 * q)
            cand = []
            for m in range(-64, 65):
                tq = F32(t * (1.0 + m * 2.0 ** -23))
                pair = np.array([[xa, y0, xa + a, y0 + b], [xa + tq, y0, (xa + tq) + a, y0 + b]], F32)
                cand.append((abs(float(_nms_overlap(pair, case.plus_one, case.method == "Min", np.float64)[0, 1]) - thr), m, pair))
            cand.sort(key=lambda c: (c[0], c[1]))
            boxes[10 + 2 * q:12 + 2 * q] = cand[q][2]
        image[10:20] = 2
    scores = np.linspace(0.99, 0.5, n).astype(F32)
    if n >= 63:
        scores[20:24] = scores[20]            # ties: the stable sort keeps their order
    return boxes, image, scores


def _nms_overlap(boxes, plus_one, use_min, dtype):
    """[n][n] overlap of box i (rows) with box j (columns), one operation at a time in `dtype`, in the order of mtcnn._nms."""
    b = np.asarray(boxes, F32).astype(dtype)
    one = dtype(1.0 if plus_one else 0.0)
    x1, y1, x2, y2 = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
    area = ((x2 - x1) + one) * ((y2 - y1) + one)
    w = np.maximum(dtype(0), (np.minimum(x2[:, None], x2[None, :]) - np.maximum(x1[:, None], x1[None, :])) + one)
    h = np.maximum(dtype(0), (np.minimum(y2[:, None], y2[None, :]) - np.maximum(y1[:, None], y1[None, :])) + one)
    inter = w * h
    with np.errstate(invalid="ignore", divide="ignore"):
        if use_min:
            return inter / np.minimum(area[:, None], area[None, :])
        return inter / ((area[:, None] + area[None, :]) - inter)


def nms_bits(boxes, image, thr, method, plus_one, dtype=F32, defect=None) -> np.ndarray:
    """bool [n][n]: box i, if kept, removes box j."""
    n = boxes.shape[0]
    use_min = method == "Min"
    o = _nms_overlap(boxes, plus_one, use_min, dtype)
    t = dtype(thr)
    with np.errstate(invalid="ignore"):
        rule_min = (defect == "nan_swapped") != use_min
        sup = ~(o <= t) if rule_min else (o > t)
    i, j = np.arange(n)[:, None], np.arange(n)[None, :]
    valid = (j > i) if defect != "lower_not_skipped" else (j != i)
    if image is not None and defect != "image_ignored":
        valid = valid & (np.asarray(image)[:, None] == np.asarray(image)[None, :])
    return sup & valid


def pack_bits(bits: np.ndarray) -> np.ndarray:
    """bool [n][n] -> uint64 [n][ceil(n / 64)], bit j & 63 of word j / 64."""
    n = bits.shape[0]
    words = (n + 63) // 64
    padded = np.zeros((n, words * 64), np.uint8)
    padded[:, :n] = bits
    return np.ascontiguousarray(np.packbits(padded, axis=1, bitorder="little")).view("<u8").reshape(n, words)


def nms_mask_fp32(case: NmsCase, boxes, image, defect=None) -> np.ndarray:
    return pack_bits(nms_bits(boxes, image if case.with_image else None, case.thr, case.method, case.plus_one, F32, defect))


def nms_undecided(case: NmsCase, boxes, image) -> Tuple[int, int]:
    """(pairs where the fp32 restatement and float64 disagree, pairs compared)."""
    im = image if case.with_image else None
    a = nms_bits(boxes, im, case.thr, case.method, case.plus_one, F32)
    b = nms_bits(boxes, im, case.thr, case.method, case.plus_one, np.float64)
    n = case.n
    pairs = np.triu(np.ones((n, n), bool), 1)
    if im is not None:
        pairs &= im[:, None] == im[None, :]
    return int((a != b).sum()), int(pairs.sum())


def left_of_diagonal_zero(mask: np.ndarray) -> bool:
    """Every word whose 64 columns all lie below the row's index, and every bit j <= i of the diagonal word."""
    n, words = mask.shape
    i = np.arange(n)
    for wd in range(words):
        full = mask[i // 64 > wd, wd]
        if full.size and full.any():
            return False
    r = (i % 64).astype(np.uint64)
    low = np.where(r == 63, np.uint64(2 ** 64 - 1), (np.uint64(1) << ((r + np.uint64(1)) % np.uint64(64))) - np.uint64(1))      # bits 0 .. i % 64
    return not bool((mask[i, i // 64] & low).any())


def host_scan(mask: np.ndarray) -> np.ndarray:
    """The greedy scan of MTCNN._bnms over the rows of the mask: indices kept, in score order."""
    n, words = mask.shape
    removed = np.zeros(words, np.uint64)
    keep = []
    for i in range(n):
        if (int(removed[i >> 6]) >> (i & 63)) & 1:
            continue
        keep.append(i)
        removed |= mask[i]
    return np.asarray(keep, np.int64)


def bnms_order(kept: np.ndarray, idxs: np.ndarray, scores: np.ndarray) -> np.ndarray:
    """The order MTCNN._bnms returns the scan's survivors in: per-image groups, then descending score, both stable."""
    kept = kept[np.argsort(idxs[kept], kind="stable")]
    return kept[np.argsort(-scores[kept], kind="stable")]


# ------------------------------------------------------------------------------------------------------------------------------------
# defects and the named case each must fail
# ------------------------------------------------------------------------------------------------------------------------------------
HARMLESS = ("prelu_gt",)
DEFECTS = AREA_DEFECTS + CONV_DEFECTS + POOL_DEFECTS + SM_DEFECTS + NMS_DEFECTS
DEFECT_CASES = {
    "win_end_floor": ("area", "ramp3_pyramid0_37x28"),
    "win_start_next": ("area", "ramp3_2to1"),
    "chan_stride3": ("area", "ramp4_50x53_to_24"),
    "last_tap_dropped": ("conv", "k2x3"),
    "kykx_swapped": ("conv", "pnet_conv1"),
    "bias_dropped": ("conv", "pnet_conv4_1"),
    "slope0_all": ("conv", "head1x1_prelu"),
    "max_init_zero": ("pool", (6, 8, 3, 2)),
    "window_unclipped": ("pool", (6, 8, 3, 2)),
    "last_output_dropped": ("pool", (6, 8, 3, 2)),
    "no_max_sub": ("softmax", 255),
    "p0_returned": ("softmax", 255),
    "lower_not_skipped": ("nms", "n65_Union_plus0_image"),
    "image_ignored": ("nms", "n65_Min_plus1_image"),
    "nan_swapped": ("nms", "n63_Union_plus0_image"),
}


def defect_fails(defect: str) -> bool:
    """True when `defect`, injected into the reference of its named case, violates that case's criterion."""
    kind, key = DEFECT_CASES[defect]
    if kind == "area":
        case = {c.name: c for c in area_cases()}[key]
        img = area_images()[case.image]
        ref, bound = area_reference(img, case)
        return not check(area_reference(img, case, defect=defect)[0], ref, bound)[0]
    if kind == "conv":
        case = {c.name: c for c in conv_cases()}[key]
        args = conv_inputs(case)
        ref, bound, _ = conv_reference(*args)
        return not check(conv_reference(*args, defect=defect)[0], ref, bound)[0]
    if kind == "pool":
        h, w, k, s = key
        x = pool_inputs(h, w, k, s)
        return not bit_equal(pool_reference(x, k, s, defect), pool_reference(x, k, s))[0]
    if kind == "softmax":
        x = sm_inputs(key)
        ref, bound, _, _ = sm_bound(x)
        return not check(sm_reference(x, defect), ref, bound)[0]
    case = {c.name: c for c in nms_cases()}[key]
    boxes, image, _ = nms_inputs(case)
    return not np.array_equal(nms_mask_fp32(case, boxes, image, defect), nms_mask_fp32(case, boxes, image))
