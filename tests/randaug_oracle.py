"""Oracle of the FR-training input stage (FR_training/utils/augmentation.py + rand_augment.py of the reference).

Two parts.

(a) The reference's transform restated ON PILLOW ITSELF: ``RandAugment`` with the global-state draws of rand_augment.py:228-237 and
    ``_apply_op`` through the PIL calls of torchvision's PIL backend -- ``Image.transform(AFFINE, NEAREST, fillcolor=(0, 0, 0))``,
    ``Image.rotate``, ``ImageEnhance.Brightness / Color / Contrast / Sharpness``, ``ImageOps.posterize / solarize / autocontrast /
    equalize`` and ``convert("L")`` stacked three times; the flip is ``transpose(FLIP_LEFT_RIGHT)``; ToTensor + Normalize are torch
    CPU ops.  torchvision is not a dependency of this project: its layer is restated from ``transforms/functional.py``,
    ``_functional_pil.py`` and ``autoaugment.py``, so PARITY WITH A torchvision BINARY IS UNPINNED.  Pillow parity is pinned, because
    Pillow is called.

(b) Every op restated in integer / single-float numpy (``np_*``): what csrc/idb_augment.hip transcribes.  tests/test_augment_cpu.py
    proves (b) equal to (a) image for image.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch
from PIL import Image, ImageEnhance, ImageFilter, ImageOps

OPS = ["Identity", "ShearX", "TranslateX", "Rotate", "Brightness", "Color", "Contrast", "Sharpness", "Posterize", "Solarize",
       "AutoContrast", "Equalize", "Grayscale"]


# ---- (a) on Pillow ----------------------------------------------------------------------------------------------------------------
def augmentation_space(num_bins: int, image_size: List[int]) -> Dict[str, Tuple[torch.Tensor, bool]]:
    """rand_augment.py:191-212 (``image_size`` is torchvision's ``get_image_size``: [width, height])."""
    return {
        "Identity": (torch.tensor(0.0), False),
        "ShearX": (torch.linspace(0.0, 0.3, num_bins), True),
        "TranslateX": (torch.linspace(0.0, 150.0 / 331.0 * image_size[0], num_bins), True),
        "Rotate": (torch.linspace(0.0, 30.0, num_bins), True),
        "Brightness": (torch.linspace(0.0, 0.9, num_bins), True),
        "Color": (torch.linspace(0.0, 0.9, num_bins), True),
        "Contrast": (torch.linspace(0.0, 0.9, num_bins), True),
        "Sharpness": (torch.linspace(0.0, 0.9, num_bins), True),
        "Posterize": (8 - (torch.arange(num_bins) / ((num_bins - 1) / 4)).round().int(), False),
        "Solarize": (torch.linspace(255.0, 0.0, num_bins), False),
        "AutoContrast": (torch.tensor(0.0), False),
        "Equalize": (torch.tensor(0.0), False),
        "Grayscale": (torch.tensor(0.0), False),
    }


def inverse_affine_matrix(center, angle, translate, scale, shear) -> List[float]:
    """torchvision ``_get_inverse_affine_matrix``."""
    rot = math.radians(angle)
    sx = math.radians(shear[0])
    sy = math.radians(shear[1])
    cx, cy = center
    tx, ty = translate
    a = math.cos(rot - sy) / math.cos(sy)
    b = -math.cos(rot - sy) * math.tan(sx) / math.cos(sy) - math.sin(rot)
    c = math.sin(rot - sy) / math.cos(sy)
    d = -math.sin(rot - sy) * math.tan(sx) / math.cos(sy) + math.cos(rot)
    matrix = [d, -b, 0.0, -c, a, 0.0]
    matrix = [x / scale for x in matrix]
    matrix[2] += matrix[0] * (-cx - tx) + matrix[1] * (-cy - ty)
    matrix[5] += matrix[3] * (-cx - tx) + matrix[4] * (-cy - ty)
    matrix[2] += cx
    matrix[5] += cy
    return matrix


def _pil_affine(img: Image.Image, angle, translate, scale, shear, center=None) -> Image.Image:
    """torchvision ``F.affine`` of a PIL image: NEAREST, ``fill=None`` -> black."""
    w, h = img.size
    if center is None:
        center = [w * 0.5, h * 0.5]
    matrix = inverse_affine_matrix(center, angle, translate, scale, shear)
    return img.transform((w, h), Image.AFFINE, matrix, Image.NEAREST, fillcolor=(0, 0, 0))


def apply_op(img: Image.Image, op_name: str, magnitude: float) -> Image.Image:
    """rand_augment.py ``_apply_op`` for a PIL RGB image with interpolation NEAREST and fill None."""
    if op_name == "ShearX":
        return _pil_affine(img, 0.0, [0, 0], 1.0, [math.degrees(math.atan(magnitude)), 0.0], center=[0, 0])
    if op_name == "TranslateX":
        return _pil_affine(img, 0.0, [int(magnitude), 0], 1.0, [0.0, 0.0])
    if op_name == "Rotate":
        return img.rotate(magnitude, Image.NEAREST, False, None, fillcolor=(0, 0, 0))
    if op_name == "Brightness":
        return ImageEnhance.Brightness(img).enhance(1.0 + magnitude)
    if op_name == "Color":
        return ImageEnhance.Color(img).enhance(1.0 + magnitude)
    if op_name == "Contrast":
        return ImageEnhance.Contrast(img).enhance(1.0 + magnitude)
    if op_name == "Sharpness":
        return ImageEnhance.Sharpness(img).enhance(1.0 + magnitude)
    if op_name == "Posterize":
        return ImageOps.posterize(img, int(magnitude))
    if op_name == "Solarize":
        return ImageOps.solarize(img, magnitude)
    if op_name == "AutoContrast":
        return ImageOps.autocontrast(img)
    if op_name == "Equalize":
        return ImageOps.equalize(img)
    if op_name == "Grayscale":
        g = np.array(img.convert("L"), np.uint8)
        return Image.fromarray(np.dstack([g, g, g]))
    if op_name == "Identity":
        return img
    raise ValueError(f"The provided operator {op_name} is not recognized.")


class RandAugment:
    """rand_augment.py ``RandAugment.forward`` on the GLOBAL torch and numpy generators, recording its draws in ``self.trace`` as
    (op index, bin, negated) per op."""

    def __init__(self, num_ops: int = 2, magnitude: int = 9, num_magnitude_bins: int = 31):
        self.num_ops, self.magnitude, self.num_magnitude_bins = num_ops, magnitude, num_magnitude_bins
        self.trace: List[Tuple[int, int, bool]] = []

    def __call__(self, img: Image.Image) -> Image.Image:
        for _ in range(self.num_ops):
            op_meta = augmentation_space(self.num_magnitude_bins, list(img.size))
            op_index = int(torch.randint(len(op_meta), (1,)).item())
            op_name = list(op_meta.keys())[op_index]
            magnitudes, signed = op_meta[op_name]
            mag = np.random.choice(np.arange(1, self.magnitude + 1))
            magnitude = float(magnitudes[mag].item()) if magnitudes.ndim > 0 else 0.0
            neg = False
            if signed and torch.randint(2, (1,)):
                magnitude *= -1.0
                neg = True
            self.trace.append((op_index, int(mag), neg))
            img = apply_op(img, op_name, magnitude)
        return img


class RandomHorizontalFlip:
    """torchvision's: ``torch.rand(1) < p`` on the global generator; ``self.trace`` records the decisions."""

    def __init__(self, p: float = 0.5):
        self.p = p
        self.trace: List[bool] = []

    def __call__(self, img: Image.Image) -> Image.Image:
        f = bool(torch.rand(1) < self.p)
        self.trace.append(f)
        return img.transpose(Image.FLIP_LEFT_RIGHT) if f else img


def to_tensor_normalize(img: Image.Image) -> torch.Tensor:
    """``ToTensor`` then ``Normalize(0.5, 0.5)`` with torch CPU ops -> float32 [3, H, W]."""
    x = torch.from_numpy(np.array(img, np.uint8, copy=True)).permute(2, 0, 1).contiguous()
    x = x.to(torch.float32).div(255)
    mean = torch.as_tensor([0.5, 0.5, 0.5], dtype=torch.float32).view(-1, 1, 1)
    std = torch.as_tensor([0.5, 0.5, 0.5], dtype=torch.float32).view(-1, 1, 1)
    return x.sub_(mean).div_(std)


def chain(images_u8: np.ndarray, num_ops: int, magnitude: int, flip_p: Optional[float] = 0.5):
    """[RandomHorizontalFlip ->] RandAugment(num_ops, magnitude) -> ToTensor -> Normalize, image after image on the global generators
    (seed them first) -> (uint8 [N, H, W, 3], float32 [N, 3, H, W], flip trace, op trace)."""
    flip = RandomHorizontalFlip(flip_p) if flip_p is not None else None
    ra = RandAugment(num_ops, magnitude)
    u8, fl = [], []
    for a in images_u8:
        img = Image.fromarray(np.ascontiguousarray(a))
        if flip is not None:
            img = flip(img)
        img = ra(img)
        u8.append(np.array(img, np.uint8))
        fl.append(to_tensor_normalize(img))
    return np.stack(u8), torch.stack(fl), (flip.trace if flip is not None else []), ra.trace


def magnitude_of(op_name: str, bin_: int, neg: bool, width: int, num_bins: int = 31) -> float:
    """The Python float that reaches ``_apply_op``."""
    magnitudes, signed = augmentation_space(num_bins, [width, width])[op_name]
    m = float(magnitudes[bin_].item()) if magnitudes.ndim > 0 else 0.0
    return -m if (neg and signed) else m


def pil_op(image_u8: np.ndarray, op_name: str, magnitude: float) -> np.ndarray:
    return np.array(apply_op(Image.fromarray(np.ascontiguousarray(image_u8)), op_name, magnitude), np.uint8)


def pil_flip(image_u8: np.ndarray) -> np.ndarray:
    return np.array(Image.fromarray(np.ascontiguousarray(image_u8)).transpose(Image.FLIP_LEFT_RIGHT), np.uint8)


# ---- (b) integer / float32 numpy ---------------------------------------------------------------------------------------------------
def _fix(v: float) -> int:
    return int(math.floor(v * 65536.0 + 0.5))


def fixed_affine(m: List[float]) -> List[int]:
    """Pillow's affine_fixed coefficients (Geometry.c) of the inverse matrix ``m``: [a0, a1, a2, a3, a4, a5], 16.16."""
    return [_fix(m[0]), _fix(m[1]), _fix(m[2] + m[0] * 0.5 + m[1] * 0.5), _fix(m[3]), _fix(m[4]), _fix(m[5] + m[3] * 0.5 + m[4] * 0.5)]


def rotate_matrix(angle: float, w: int, h: int) -> List[float]:
    """Image.rotate's matrix (expand False, centre None, no translate) for an angle that is no multiple of 90."""
    angle = angle % 360.0
    cx, cy = w / 2.0, h / 2.0
    a = -math.radians(angle)
    m = [round(math.cos(a), 15), round(math.sin(a), 15), 0.0, round(-math.sin(a), 15), round(math.cos(a), 15), 0.0]
    m[2] = m[0] * -cx + m[1] * -cy + m[2]
    m[5] = m[3] * -cx + m[4] * -cy + m[5]
    m[2] += cx
    m[5] += cy
    return m


def geometry_matrix(op_name: str, magnitude: float, w: int, h: int) -> List[float]:
    if op_name == "ShearX":
        return inverse_affine_matrix([0, 0], 0.0, [0, 0], 1.0, [math.degrees(math.atan(magnitude)), 0.0])
    if op_name == "TranslateX":
        return inverse_affine_matrix([w * 0.5, h * 0.5], 0.0, [int(magnitude), 0], 1.0, [0.0, 0.0])
    if op_name == "Rotate":
        return rotate_matrix(magnitude, w, h)
    raise ValueError(op_name)


def np_affine(x: np.ndarray, a: List[int]) -> np.ndarray:
    h, w = x.shape[:2]
    yy, xx = np.meshgrid(np.arange(h, dtype=np.int64), np.arange(w, dtype=np.int64), indexing="ij")
    xi = (a[2] + a[1] * yy + a[0] * xx) >> 16
    yi = (a[5] + a[4] * yy + a[3] * xx) >> 16
    ok = (xi >= 0) & (xi < w) & (yi >= 0) & (yi < h)
    out = np.zeros_like(x)
    out[ok] = x[yi[ok], xi[ok]]
    return out


def np_luma(x: np.ndarray) -> np.ndarray:
    v = x.astype(np.int64)
    return ((v[..., 0] * 19595 + v[..., 1] * 38470 + v[..., 2] * 7471 + 0x8000) >> 16).astype(np.uint8)


def np_blend(deg: np.ndarray, img: np.ndarray, f: float) -> np.ndarray:
    """Image.blend(deg, img, f): float32, one rounding per operation, truncated (clipped first outside 0 <= f <= 1)."""
    f32 = np.float32(f)
    d = deg.astype(np.float32)
    t = d + f32 * (img.astype(np.float32) - d)
    assert t.dtype == np.float32
    if not 0.0 <= f <= 1.0:
        t = np.clip(t, np.float32(0), np.float32(255))
    return t.astype(np.uint8)


def np_smooth(x: np.ndarray) -> np.ndarray:
    """ImageFilter.SMOOTH: 3x3 [1 1 1; 1 5 1; 1 1 1] / 13 in float32, taps accumulated in row-major order from 0.5; border copied."""
    h, w = x.shape[:2]
    k = (np.array([1, 1, 1, 1, 5, 1, 1, 1, 1], np.float32) / np.float32(13)).astype(np.float32)
    out = x.copy()
    if h < 3 or w < 3:
        return out
    v = x.astype(np.float32)
    acc = np.full((h - 2, w - 2, x.shape[2]), 0.5, np.float32)
    for i in range(3):
        for j in range(3):
            acc = acc + v[i:h - 2 + i, j:w - 2 + j] * k[i * 3 + j]
    assert acc.dtype == np.float32
    out[1:-1, 1:-1] = np.clip(acc, np.float32(0), np.float32(255)).astype(np.uint8)
    return out


def autocontrast_lut(lo: int, hi: int) -> np.ndarray:
    if hi <= lo:
        return np.arange(256, dtype=np.uint8)
    scale = 255.0 / (hi - lo)
    off = -lo * scale
    t = np.arange(256, dtype=np.float64) * np.float64(scale) + np.float64(off)      # one rounding per operation, as Python's floats
    return np.clip(np.trunc(t), 0, 255).astype(np.uint8)


def np_autocontrast(x: np.ndarray) -> np.ndarray:
    out = np.empty_like(x)
    for c in range(3):
        out[..., c] = autocontrast_lut(int(x[..., c].min()), int(x[..., c].max()))[x[..., c]]
    return out


def np_equalize(x: np.ndarray) -> np.ndarray:
    out = np.empty_like(x)
    for c in range(3):
        h = np.bincount(x[..., c].reshape(-1), minlength=256).astype(np.int64)
        nz = np.nonzero(h)[0]
        lut = np.arange(256, dtype=np.int64)
        if len(nz) > 1:
            step = int(h.sum() - h[nz[-1]]) // 255
            if step:
                n = step // 2
                for i in range(256):
                    lut[i] = min(255, n // step)
                    n += int(h[i])
        out[..., c] = lut.astype(np.uint8)[x[..., c]]
    return out


def np_op(x: np.ndarray, op_name: str, magnitude: float) -> np.ndarray:
    """One op on one uint8 [H, W, 3] image; ``magnitude`` is the Python float that reaches ``_apply_op``."""
    h, w = x.shape[:2]
    if op_name == "Identity":
        return x.copy()
    if op_name in ("ShearX", "TranslateX", "Rotate"):
        return np_affine(x, fixed_affine(geometry_matrix(op_name, magnitude, w, h)))
    if op_name == "Brightness":
        return np_blend(np.zeros_like(x), x, 1.0 + magnitude)
    if op_name == "Color":
        return np_blend(np.repeat(np_luma(x)[..., None], 3, axis=2), x, 1.0 + magnitude)
    if op_name == "Contrast":
        s, cnt = int(np_luma(x).astype(np.int64).sum()), h * w
        return np_blend(np.full_like(x, (2 * s + cnt) // (2 * cnt)), x, 1.0 + magnitude)
    if op_name == "Sharpness":
        return np_blend(np_smooth(x), x, 1.0 + magnitude)
    if op_name == "Posterize":
        return x & np.uint8((0xFF << (8 - int(magnitude))) & 0xFF)
    if op_name == "Solarize":
        return np.where(x.astype(np.float64) < magnitude, x, 255 - x).astype(np.uint8)
    if op_name == "AutoContrast":
        return np_autocontrast(x)
    if op_name == "Equalize":
        return np_equalize(x)
    if op_name == "Grayscale":
        return np.repeat(np_luma(x)[..., None], 3, axis=2)
    raise ValueError(op_name)


def np_flip(x: np.ndarray) -> np.ndarray:
    return x[:, ::-1].copy()
