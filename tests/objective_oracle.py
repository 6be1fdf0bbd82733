"""ORACLE — test infrastructure only.  Float64 restatement of the training objective's forward pass
(faceposegenerator_amd/objective.py, csrc/idb_objective.hip; train_ID-Booth.py:996-1134) except the networks: the diffusion
targets, the per-sample squared error and predicted x0, the crop + bilinear resize + ArcFace normalisation, the area resize of a float
image, the identity / triplet losses and the host policy (box clipping, timestep weight, the combined loss, the undetected rule).
tests/test_objective_cpu.py checks every piece against torch itself and against this project's DDPMScheduler; the GPU tests compare
the kernels with it.  The fp32 inputs (the alphas_cumprod table included) are taken as given and everything after is float64."""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import torch
import torch.nn.functional as F

from matrix_common import ulp32  # noqa: F401  (used here and by the objective tests)

U32 = 2.0 ** -24
MTCNN_IMAGE_SEED = 23         # the float test image of the detector test (2 x 80 x 96): of the seeds 1..24 the one whose oracle run stays
                              # furthest (7.6e-4) from every stage threshold; test_objective_cpu.py asserts the margin


# ---- schedule -----------------------------------------------------------------------------------------------------------------------
def coefs(alphas_cumprod: torch.Tensor, timesteps):
    """sqrt(abar_t), sqrt(1 - abar_t) per sample, float64 [B,1,1,1]; timesteps clamped into the table as the kernels do."""
    t = torch.as_tensor(timesteps).long().clamp(0, alphas_cumprod.numel() - 1)
    a = alphas_cumprod.double()[t]
    return a.sqrt().view(-1, 1, 1, 1), (1.0 - a).sqrt().view(-1, 1, 1, 1)


def diffuse_targets(x0, noise, timesteps, alphas_cumprod, v_prediction: bool):
    sa, sb = coefs(alphas_cumprod, timesteps)
    x0, noise = x0.double(), noise.double()
    return sa * x0 + sb * noise, (sa * noise - sb * x0 if v_prediction else noise.clone())


def pred_original_sample(pred, noisy, timesteps, alphas_cumprod, v_prediction: bool):
    sa, sb = coefs(alphas_cumprod, timesteps)
    pred, noisy = pred.double(), noisy.double()
    return sa * noisy - sb * pred if v_prediction else (noisy - sb * pred) / sa


def sse(pred, target):
    """Sum of squared differences per sample, float64 [B]."""
    return (pred.double() - target.double()).pow(2).flatten(1).sum(1)


def mse_halves(pred, target, n_instances: int):
    """(instance, prior): F.mse_loss of the first n_instances samples and of the rest (0.0 when there is no rest)."""
    per = sse(pred, target) / pred[0].numel()
    return float(per[:n_instances].mean()), (float(per[n_instances:].mean()) if per.numel() > n_instances else 0.0)


# ---- resizes ------------------------------------------------------------------------------------------------------------------------
def _taps(n_in: int, n_out: int):
    o = np.arange(n_out, dtype=np.float64)
    s = np.maximum((o + 0.5) * (n_in / n_out) - 0.5, 0.0)
    i0 = np.minimum(np.floor(s).astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    l1 = np.clip(s - i0, 0.0, 1.0)
    return i0, i1, 1.0 - l1, l1


def bilinear_restated(img: np.ndarray, oh: int, ow: int) -> np.ndarray:
    """F.interpolate(mode="bilinear", align_corners=False, antialias=False) written out: img float64 [C,H,W] -> [C,oh,ow]."""
    ya, yb, hy0, hy1 = _taps(img.shape[1], oh)
    xa, xb, wx0, wx1 = _taps(img.shape[2], ow)
    top = img[:, ya][:, :, xa] * wx0 + img[:, ya][:, :, xb] * wx1
    bot = img[:, yb][:, :, xa] * wx0 + img[:, yb][:, :, xb] * wx1
    return top * hy0[None, :, None] + bot * hy1[None, :, None]


def crop_resize_bilinear(images: torch.Tensor, boxes, oh: int = 112, ow: int = 112, restated: bool = False) -> torch.Tensor:
    """images float NHWC [B,H,W,C] in [0, 255]; boxes [n][5] = image, y0, y1, x0, x1 -> float64 [n,C,oh,ow] =
    ((resize(crop) / 255) - 0.5) / 0.5, the resize by float64 F.interpolate (or by bilinear_restated)."""
    out = []
    for i, y0, y1, x0, x1 in np.asarray(boxes).reshape(-1, 5).tolist():
        crop = images[i, y0:y1, x0:x1].permute(2, 0, 1).double()
        r = (torch.from_numpy(bilinear_restated(crop.numpy(), oh, ow)) if restated
             else F.interpolate(crop[None], size=(oh, ow), mode="bilinear", align_corners=False, antialias=False)[0])
        out.append(((r / 255.0) - 0.5) / 0.5)
    return torch.stack(out) if out else torch.zeros(0, images.shape[-1], oh, ow, dtype=torch.float64)


def crop_resize_area(images: torch.Tensor, boxes, oh: int, ow: int, exact_sums: bool, sub: float = 127.5, mul: float = 0.0078125):
    """(out, bound) float64 [n,C,oh,ow]: (F.interpolate(crop, mode="area") - sub) * mul in float64 and the bound of
    tests/detect_matrix.py's area criterion, (u |q| + u |q - sub|) |mul| + u |out| with q the window mean.  That criterion presumes
    that the fp32 window sum is exact (uint8 data; multiples of 1/4).  Without exact_sums the sequential fp32 sum of a window of k
    non-negative values adds its forward bound gamma_k |q| |mul|."""
    outs, bounds = [], []
    for i, y0, y1, x0, x1 in np.asarray(boxes).reshape(-1, 5).tolist():
        crop = images[i, y0:y1, x0:x1].permute(2, 0, 1).double()
        q = F.interpolate(crop[None], size=(oh, ow), mode="area")[0]
        k = (-(-(y1 - y0) // oh) + 1) * (-(-(x1 - x0) // ow) + 1)              # no window has more pixels than this
        o = (q - sub) * mul
        outs.append(o)
        bounds.append((U32 * q.abs() + U32 * (q - sub).abs()) * abs(mul) + U32 * o.abs()
                      + (0.0 if exact_sums else k * U32 / (1 - k * U32)) * q.abs() * abs(mul))
    return torch.stack(outs), torch.stack(bounds)


# ---- identity losses ----------------------------------------------------------------------------------------------------------------
def cos_eps(a, b, eps: float):
    """torch's cosine similarity along dim 1: each norm clamped at eps."""
    a, b = a.double(), b.double()
    return (a * b).sum(1) / (a.norm(dim=1).clamp_min(eps) * b.norm(dim=1).clamp_min(eps))


def identity_losses(feat, pos, neg=None):
    """(cos, identity, triplet or None) float64 [n]: nn.CosineSimilarity(eps=1e-6), 1 - cos, and
    TripletMarginWithDistanceLoss(distance_function = 1 - F.cosine_similarity, margin 1) per row."""
    cos = cos_eps(feat, pos, 1e-6)
    trip = None
    if neg is not None:
        trip = ((1.0 - cos_eps(feat, pos, 1e-8)) - (1.0 - cos_eps(feat, neg, 1e-8)) + 1.0).clamp_min(0.0)
    return cos, 1.0 - cos, trip


def loss_bound(ref) -> np.ndarray:
    """2 fp32 ulp of the float64 value, plus the float64 oracle's own error: a handful of 2^-53 roundings of quantities of
    magnitude <= 2 (the cosines, 1 - cos, the hinge argument), which is all that is left of a value that cancels to ~0."""
    return 2.0 * ulp32(ref) + 16.0 * 2.0 ** -53


# ---- host policy --------------------------------------------------------------------------------------------------------------------
def clip_box(box, size: int):
    """bbox.astype(int), then img[max(0, b1):min(b3, S), max(0, b0):min(b2, S)] -> (y0, y1, x0, x1), None when empty."""
    b = [int(np.trunc(float(v))) for v in np.asarray(box).reshape(-1)[:4]]
    y0, y1, x0, x1 = max(0, b[1]), min(b[3], size), max(0, b[0]), min(b[2], size)
    return None if y1 <= y0 or x1 <= x0 else (y0, y1, x0, x1)


def timestep_weight(t: int, T: int, on: bool = True) -> float:
    return (1.0 - t / T) ** 2 if on else 1.0


def combined(instance: float, prior: float, id_losses: Sequence[float], weights: Sequence[float], detected: Sequence[bool],
             prior_loss_weight: float, which_loss: str) -> float:
    """instance + prior_loss_weight * prior + mean over the detected instances of weight_i * id_i (nothing when which_loss is ""
    or no face was detected)."""
    out = instance + prior_loss_weight * prior
    terms = [w * l for w, l, d in zip(weights, id_losses, detected) if d]
    if which_loss and terms:
        out += sum(terms) / len(terms)
    return out


# ---- the detector's float test image ------------------------------------------------------------------------------------------------
def mtcnn_float_image(seed: int = MTCNN_IMAGE_SEED, b: int = 2, h: int = 80, w: int = 96) -> torch.Tensor:
    """Float NHWC [b,h,w,3] in [0, 255] with fractional values: the recipe of tests/test_mtcnn_gpu.py without the uint8 cast."""
    g = torch.Generator().manual_seed(seed)
    base = torch.rand(b, 3, h // 8, w // 8, generator=g)
    return (F.interpolate(base, size=(h, w), mode="bilinear") * 255).permute(0, 2, 3, 1).contiguous()


def mtcnn_threshold_margin(img: torch.Tensor, weights, thresholds=(0.6, 0.7, 0.7)) -> Optional[float]:
    """The smallest distance of any P-, R- or O-Net face probability from its stage's threshold while oracle.mtcnn_oracle.detect_face
    runs on `img` (the stage functions are wrapped for the duration of the call, the oracle itself is untouched)."""
    from oracle import mtcnn_oracle as O
    margins = []
    saved = {n: getattr(O, n) for n in ("pnet", "rnet", "onet")}

    def wrap(name, thr):
        def f(sd, x):
            out = saved[name](sd, x)
            p = out[-1][:, 1]
            if p.numel():
                margins.append(float((p.double() - thr).abs().min()))
            return out
        return f

    try:
        for name, thr in zip(("pnet", "rnet", "onet"), thresholds):
            setattr(O, name, wrap(name, thr))
        O.detect_face(img, weights)
    finally:
        for name, fn in saved.items():
            setattr(O, name, fn)
    return min(margins) if margins else None
