"""Test infrastructure for faceposegenerator_amd/fiqa.py (no GPU): restatements, written from the arithmetic alone, of what the
reference's CR-FIQA script computes around the network.

  * ``coef_table`` / ``resize``: OpenCV's ``cv2.resize(img, (dw, dh))`` with ``INTER_LINEAR`` on 8-bit data, in numpy integers and
    scalar Python loops (deliberately not the vectorised host code of ``fiqa.coef_tables``): per axis the float32 position, its
    floor, the clamps, the int16 coefficients on an 11-bit scale; an int32 horizontal pass; the ``>> 4``, ``>> 16``, ``+ 2``,
    ``>> 2`` vertical pass; and the 2x2 box mean that OpenCV switches to when both axes halve exactly.
    PARITY OF THIS RESTATEMENT WITH A cv2 BINARY IS UNPINNED: cv2 is not installed where this suite runs.  What pins it instead
    (tests/test_fiqa_cpu.py): identity sizes return the source, a constant image stays constant, known tables and rows, and a
    distance below one grey level from unrounded float64 bilinear interpolation (0.78 measured over the shapes of the test).
  * ``forward``: the network.  The body is tests/arcface_oracle.py's fp32 restatement (the reference the ArcFace bounds were set
    against), then the ``qs`` linear head on its output, evaluated in float64.
  * ``normalize``: sklearn.preprocessing.normalize (l2, rows), float64; a zero row stays zero.
  * ``tail``: ``qs`` and ``normalize`` of given embeddings in float64, with the sum of |e_i w_i| that the tail's error bound needs."""
from __future__ import annotations

import os
import sys
from typing import Tuple

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import arcface_oracle as AO  # noqa: E402

COEF_BITS = 11
COEF_ONE = 1 << COEF_BITS


def coef_table(s: int, d: int) -> Tuple[np.ndarray, np.ndarray]:
    """Offsets int64 [d] and coefficients int64 [d][2] of one axis, ``s`` source and ``d`` destination samples."""
    scale = float(s) / float(d)                                  # double
    ofs = np.zeros(d, dtype=np.int64)
    coef = np.zeros((d, 2), dtype=np.int64)
    for i in range(d):
        f = np.float32((i + 0.5) * scale - 0.5)                  # double arithmetic, one rounding to float32
        o = int(np.floor(f))
        f = np.float32(f - np.float32(o))
        if o < 0:
            o, f = 0, np.float32(0)
        if o >= s - 1:
            o, f = s - 1, np.float32(0)
        c0 = np.float32(np.float32(1) - f) * np.float32(COEF_ONE)
        c1 = np.float32(f * np.float32(COEF_ONE))
        ofs[i] = o
        coef[i] = (int(np.rint(c0)), int(np.rint(c1)))           # rint: round half to even
    return ofs, coef


def resize(images: np.ndarray, dh: int, dw: int) -> np.ndarray:
    """uint8 [B, H, W, C] -> uint8 [B, dh, dw, C]."""
    images = np.asarray(images)
    assert images.dtype == np.uint8 and images.ndim == 4
    B, H, W, C = images.shape
    src = images.astype(np.int64)
    if H == 2 * dh and W == 2 * dw:
        box = src[:, 0::2, 0::2] + src[:, 0::2, 1::2] + src[:, 1::2, 0::2] + src[:, 1::2, 1::2]
        return ((box + 2) >> 2).astype(np.uint8)
    ox, cx = coef_table(W, dw)
    oy, cy = coef_table(H, dh)
    ox1 = np.minimum(ox + 1, W - 1)
    oy1 = np.minimum(oy + 1, H - 1)
    rows = src[:, :, ox, :] * cx[None, None, :, 0, None] + src[:, :, ox1, :] * cx[None, None, :, 1, None]      # [B, H, dw, C]
    assert rows.max() < 2 ** 31
    b0, b1 = cy[None, :, 0, None, None], cy[None, :, 1, None, None]
    out = (((b0 * (rows[:, oy] >> 4)) >> 16) + ((b1 * (rows[:, oy1] >> 4)) >> 16) + 2) >> 2
    return np.clip(out, 0, 255).astype(np.uint8)


def bilinear_f64(images: np.ndarray, dh: int, dw: int) -> np.ndarray:
    """Unrounded float64 bilinear interpolation with half-pixel centres and edge clamping (F.interpolate, align_corners=False)."""
    x = torch.from_numpy(np.asarray(images)).double().permute(0, 3, 1, 2)
    y = torch.nn.functional.interpolate(x, size=(dh, dw), mode="bilinear", align_corners=False, antialias=False)
    return y.permute(0, 2, 3, 1).numpy()


def normalize(x: np.ndarray) -> np.ndarray:
    x = np.asarray(x, dtype=np.float64)
    n = np.sqrt((x * x).sum(axis=1, keepdims=True))
    n[n == 0.0] = 1.0
    return x / n


def tail(emb: np.ndarray, w: np.ndarray, b: float):
    """-> (qs [B], normalised embeddings [B, D], sum_i |e_i w_i| [B]), float64."""
    e = np.asarray(emb, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64).reshape(-1)
    prod = e * w[None, :]
    return prod.sum(axis=1) + float(b), normalize(e), np.abs(prod).sum(axis=1)


def forward(sd, arch: str, x: torch.Tensor):
    """x: float [B, 3, 112, 112], already (x/255 - 0.5)/0.5 -> (features [B, 512], qs [B, 1]), float64 tensors."""
    body = {k: v for k, v in sd.items() if not k.startswith("qs.")}
    feat = AO.forward(body, arch, x).double()
    qs = feat @ sd["qs.weight"].double().t() + sd["qs.bias"].double()
    return feat, qs
