"""The FR-training input stage — what every training image of the reference's FR_training/train_FR.py passes through first
(FR_training/config/FR_config.py:47 ``augmentation = "ra_4_16"``; utils/augmentation.py:49-54, 115-148; utils/rand_augment.py:191-239;
applied per PIL image inside DataLoader workers, utils/dataset.py:154-196):

    RandomHorizontalFlip -> RandAugment(num_ops=4, magnitude=16) -> ToTensor -> Normalize(0.5, 0.5)

Here the chain runs on a whole uint8 batch in ONE launch of idb_randaug (csrc/idb_augment.hip): one workgroup per image, the image in
LDS for the whole chain.  Every op is Pillow's arithmetic restated in integers / single floats (torchvision's PIL backend is thin
wrappers over Pillow); tests/randaug_oracle.py holds the restatement and tests/test_augment_cpu.py proves it equal to Pillow image for
image.  torchvision is not a dependency: its layer (``_get_inverse_affine_matrix``, the fill and centre defaults) is restated, so
PARITY WITH A torchvision BINARY IS UNPINNED; Pillow parity is pinned.

Random draws.  ``RandAugment.plan`` makes the reference's draws for one sample, image after image, in its order: ``torch.rand(1) <
p`` (the flip), then per op ``torch.randint(13, (1,))``, ``np.random.choice(np.arange(1, magnitude + 1))`` (also for ops whose table is
a scalar) and ``torch.randint(2, (1,))`` only if the op is signed.  The reference draws from the global torch and numpy states; here
the draws come from the given ``torch.Generator`` and ``np.random.RandomState`` and the global states are left untouched (the policy of
fiqa.sample_paths and verification.pairs_*).  WHICH STREAM A MULTI-WORKER DataLoader WOULD HAVE GIVEN EACH IMAGE is not defined
upstream (it depends on the worker count, the worker seeds and the scheduling) and is not reproduced.

Supported sizes: 8 <= H, W and H * W * 3 <= 49152 bytes (128 x 128; the workload is 112 x 112).  There is no CPU fallback."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Callable, Dict, List, Optional, Tuple

import numpy as np
import torch

from . import _lib as L

OPS = ["Identity", "ShearX", "TranslateX", "Rotate", "Brightness", "Color", "Contrast", "Sharpness", "Posterize", "Solarize",
       "AutoContrast", "Equalize", "Grayscale"]                     # the reference's dict order: the op index is drawn into it
SIGNED = ("ShearX", "TranslateX", "Rotate", "Brightness", "Color", "Contrast", "Sharpness")
_SIGNED_IDX = frozenset(OPS.index(o) for o in SIGNED)
MAX_BYTES = 49152                                                   # IDB_RANDAUG_MAX_BYTES: one image, H * W * 3
MIN_SIDE = 8


def magnitude_tables(width: int, num_bins: int = 31) -> Dict[str, Tuple[torch.Tensor, bool]]:
    """``RandAugment._augmentation_space(num_bins, image_size)``: op name -> (float32 magnitudes, signed), built with torch exactly as
    upstream.  TranslateX scales with ``image_size[0]``, which is the WIDTH (torchvision's get_image_size)."""
    return {
        "Identity": (torch.tensor(0.0), False),
        "ShearX": (torch.linspace(0.0, 0.3, num_bins), True),
        "TranslateX": (torch.linspace(0.0, 150.0 / 331.0 * width, num_bins), True),
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


@dataclass
class AugPlan:
    """The draws of one batch: ``flip`` bool [n]; ``op`` (index into OPS), ``bin`` (index into the magnitude table) and ``neg`` (the
    magnitude is negated) [n, num_ops].  numpy arrays on the host."""
    flip: np.ndarray
    op: np.ndarray
    bin: np.ndarray
    neg: np.ndarray
    num_magnitude_bins: int = 31

    @property
    def n(self) -> int:
        return int(self.flip.shape[0])

    @property
    def num_ops(self) -> int:
        return int(self.op.shape[1])


def make_plan(flip, op, bin, neg=None, num_magnitude_bins: int = 31) -> AugPlan:
    """A hand-made plan from array-likes (``neg`` defaults to all False), validated."""
    flip = np.ascontiguousarray(np.asarray(flip, dtype=bool).reshape(-1))
    n = flip.shape[0]
    op = np.ascontiguousarray(np.asarray(op, dtype=np.int32).reshape(n, -1))
    bin = np.ascontiguousarray(np.asarray(bin, dtype=np.int32).reshape(n, -1))
    neg = np.zeros(op.shape, bool) if neg is None else np.ascontiguousarray(np.asarray(neg, dtype=bool).reshape(n, -1))
    if not (op.shape == bin.shape == neg.shape):
        raise ValueError(f"make_plan: op {op.shape}, bin {bin.shape} and neg {neg.shape} must agree")
    if op.size and (op.min() < 0 or op.max() >= len(OPS) or bin.min() < 0 or bin.max() >= num_magnitude_bins):
        raise ValueError(f"make_plan: op must lie in 0..{len(OPS) - 1} and bin in 0..{num_magnitude_bins - 1}")
    return AugPlan(flip, op, bin, neg, int(num_magnitude_bins))


class RandAugment:
    """The reference's ``RandAugment(num_ops, magnitude, num_magnitude_bins)`` (interpolation NEAREST, fill None) as a planner: it draws,
    ``apply`` executes."""

    def __init__(self, num_ops: int = 4, magnitude: int = 16, num_magnitude_bins: int = 31):
        if num_ops < 0 or not 1 <= magnitude < num_magnitude_bins:
            raise ValueError(f"RandAugment: num_ops >= 0 and 1 <= magnitude < num_magnitude_bins, got {num_ops}, {magnitude}, {num_magnitude_bins}")
        self.num_ops, self.magnitude, self.num_magnitude_bins = int(num_ops), int(magnitude), int(num_magnitude_bins)

    def plan(self, n: int, torch_generator: Optional[torch.Generator] = None, np_random: Optional[np.random.RandomState] = None,
             flip_p: Optional[float] = 0.5) -> AugPlan:
        """The draws of ``n`` images in sequence (module docstring: order and generators).  ``flip_p=None`` is a chain without the
        flip (nothing is drawn for it).  A missing generator is a fresh unseeded one; the global states are never touched.  Which
        stream a multi-worker DataLoader would have given each image is not defined upstream and is not reproduced."""
        g = torch_generator if torch_generator is not None else torch.Generator()
        if torch_generator is None:
            g.seed()
        r = np_random if np_random is not None else np.random.RandomState()
        flip = np.zeros(n, bool)
        op = np.zeros((n, self.num_ops), np.int32)
        bin_ = np.zeros((n, self.num_ops), np.int32)
        neg = np.zeros((n, self.num_ops), bool)
        choices = np.arange(1, self.magnitude + 1)
        for i in range(n):
            if flip_p is not None:
                flip[i] = bool(torch.rand(1, generator=g) < flip_p)
            for s in range(self.num_ops):
                o = int(torch.randint(len(OPS), (1,), generator=g).item())
                op[i, s] = o
                bin_[i, s] = int(r.choice(choices))
                if o in _SIGNED_IDX and int(torch.randint(2, (1,), generator=g)):
                    neg[i, s] = True
        return AugPlan(flip, op, bin_, neg, self.num_magnitude_bins)


# ---- (op, bin, neg) + image size -> kernel arguments ------------------------------------------------------------------------------
def _inverse_affine_matrix(center, angle, translate, scale, shear) -> List[float]:
    """torchvision's ``_get_inverse_affine_matrix``, in Python doubles."""
    rot, sx, sy = math.radians(angle), math.radians(shear[0]), math.radians(shear[1])
    cx, cy = center
    tx, ty = translate
    a = math.cos(rot - sy) / math.cos(sy)
    b = -math.cos(rot - sy) * math.tan(sx) / math.cos(sy) - math.sin(rot)
    c = math.sin(rot - sy) / math.cos(sy)
    d = -math.sin(rot - sy) * math.tan(sx) / math.cos(sy) + math.cos(rot)
    m = [x / scale for x in (d, -b, 0.0, -c, a, 0.0)]
    m[2] += m[0] * (-cx - tx) + m[1] * (-cy - ty)
    m[5] += m[3] * (-cx - tx) + m[4] * (-cy - ty)
    m[2] += cx
    m[5] += cy
    return m


def _rotate_matrix(angle: float, w: int, h: int) -> List[float]:
    """Pillow's ``Image.rotate(angle, NEAREST, expand=False, center=None)`` matrix; the tables give 1..30 degrees either way, so
    its 0 / 90 / 180 / 270 shortcuts cannot occur."""
    angle = angle % 360.0
    cx, cy = w / 2.0, h / 2.0
    a = -math.radians(angle)
    m = [round(math.cos(a), 15), round(math.sin(a), 15), 0.0, round(-math.sin(a), 15), round(math.cos(a), 15), 0.0]
    m[2] = m[0] * -cx + m[1] * -cy + m[2]
    m[5] = m[3] * -cx + m[4] * -cy + m[5]
    m[2] += cx
    m[5] += cy
    return m


def _fix(v: float) -> int:
    return int(math.floor(v * 65536.0 + 0.5))


def affine_fixed(op_name: str, magnitude: float, w: int, h: int) -> List[int]:
    """The six 16.16 integers [a0 .. a5] of Pillow's nearest affine sampler for ShearX / TranslateX / Rotate at ``magnitude`` (the
    Python float that reaches ``_apply_op``) on a ``w`` x ``h`` image: x_in = (a2 + a1 y + a0 x) >> 16, y_in = (a5 + a4 y + a3 x) >> 16."""
    if op_name == "ShearX":
        m = _inverse_affine_matrix([0, 0], 0.0, [0, 0], 1.0, [math.degrees(math.atan(magnitude)), 0.0])
    elif op_name == "TranslateX":
        m = _inverse_affine_matrix([w * 0.5, h * 0.5], 0.0, [int(magnitude), 0], 1.0, [0.0, 0.0])
    elif op_name == "Rotate":
        m = _rotate_matrix(magnitude, w, h)
    else:
        raise ValueError(f"affine_fixed: {op_name!r} is not a geometric op")
    return [_fix(m[0]), _fix(m[1]), _fix(m[2] + m[0] * 0.5 + m[1] * 0.5), _fix(m[3]), _fix(m[4]), _fix(m[5] + m[3] * 0.5 + m[4] * 0.5)]


_SLOT_TABLES: Dict[Tuple[int, int, int], Tuple[np.ndarray, np.ndarray]] = {}


def slot_tables(h: int, w: int, num_bins: int = 31) -> Tuple[np.ndarray, np.ndarray]:
    """Kernel arguments of every (op, bin, sign) at one image size -> (iarg int32 [13, num_bins, 2, 6], farg float32 [13, num_bins, 2]),
    cached.  The magnitude is ``float(table[bin])`` of the float32 torch table, negated for sign 1; ``1.0 + magnitude`` is formed in
    Python double and only then cast to float32, as upstream's blend factor is.
      ShearX / TranslateX / Rotate: iarg = affine_fixed;  Brightness / Color / Contrast / Sharpness: farg = 1 + magnitude;
      Posterize: iarg[0] = the bit mask;  Solarize: farg = the threshold;  the others take none."""
    key = (int(h), int(w), int(num_bins))
    if key not in _SLOT_TABLES:
        tabs = magnitude_tables(int(w), int(num_bins))
        ia = np.zeros((len(OPS), num_bins, 2, 6), np.int32)
        fa = np.zeros((len(OPS), num_bins, 2), np.float32)
        for o, name in enumerate(OPS):
            mags, signed = tabs[name]
            if mags.ndim == 0:
                continue
            for b in range(num_bins):
                for s in range(2):
                    m = float(mags[b].item())
                    if s and signed:
                        m *= -1.0
                    if name in ("ShearX", "TranslateX", "Rotate"):
                        ia[o, b, s] = affine_fixed(name, m, int(w), int(h))
                    elif name in ("Brightness", "Color", "Contrast", "Sharpness"):
                        fa[o, b, s] = np.float32(1.0 + m)
                    elif name == "Posterize":
                        ia[o, b, s, 0] = (0xFF << (8 - int(m))) & 0xFF
                    elif name == "Solarize":
                        fa[o, b, s] = np.float32(m)
        _SLOT_TABLES[key] = (ia, fa)
    return _SLOT_TABLES[key]


def slot_args(plan: AugPlan, h: int, w: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """A plan at one image size -> (slot_op int32 [n, num_ops], slot_iarg int32 [n, num_ops, 6], slot_farg float32 [n, num_ops])."""
    ia, fa = slot_tables(h, w, plan.num_magnitude_bins)
    s = plan.neg.astype(np.int64)
    return (np.ascontiguousarray(plan.op, dtype=np.int32), np.ascontiguousarray(ia[plan.op, plan.bin, s]),
            np.ascontiguousarray(fa[plan.op, plan.bin, s]))


def apply(images_u8, plan: AugPlan, output: str = "float", device=None):
    """Run ``plan`` on a uint8 RGB batch [N, H, W, 3] (numpy array, host tensor or device tensor; a host batch is uploaded to ``device``,
    default cuda:0) in one idb_randaug launch.
      output="u8":    uint8 [N, H, W, 3], the augmented PIL images;
      output="float": float32 [N, 3, H, W] = ToTensor + Normalize(0.5, 0.5), ``x.float().div(255).sub(0.5).div(0.5)`` with each step
                      rounded once in fp32: the tensor the reference's loader yields and ArcFace.__call__ takes;
      output="both":  the pair (u8, float).
    The input is not modified.  Sizes outside 8 <= H, W, H * W * 3 <= 49152 raise ValueError (the library itself answers
    IDB_EUNSUPPORTED)."""
    if output not in ("u8", "float", "both"):
        raise ValueError(f"apply: output must be 'u8', 'float' or 'both', got {output!r}")
    t = images_u8 if torch.is_tensor(images_u8) else torch.from_numpy(np.asarray(images_u8))
    if t.dtype != torch.uint8 or t.ndim != 4 or t.shape[3] != 3:
        raise ValueError(f"apply expects a uint8 RGB image batch [N, H, W, 3], got {t.dtype} {tuple(t.shape)}")
    if not t.is_contiguous():
        raise ValueError("apply expects a contiguous batch (NHWC in memory): call .contiguous() on it first")
    n, h, w = int(t.shape[0]), int(t.shape[1]), int(t.shape[2])
    if n < 1 or h < MIN_SIDE or w < MIN_SIDE or h * w * 3 > MAX_BYTES:
        raise ValueError(f"apply: batch {n} of {h} x {w} images is not supported: N >= 1, H, W >= {MIN_SIDE} and H * W * 3 <= {MAX_BYTES} "
                         f"(128 x 128)")
    if plan.n != n:
        raise ValueError(f"apply: the plan holds {plan.n} images, the batch {n}")
    if not t.is_cuda:
        t = t.to(torch.device(device if device is not None else "cuda:0"))
    lib = L.load()
    dev = t.device
    k = plan.num_ops
    sop, sia, sfa = slot_args(plan, h, w)
    flip = torch.from_numpy(plan.flip.astype(np.uint8)).to(dev)
    d_op = d_ia = d_fa = None
    if k:
        d_op, d_ia, d_fa = torch.from_numpy(sop).to(dev), torch.from_numpy(sia).to(dev), torch.from_numpy(sfa).to(dev)
    out_u8 = torch.empty((n, h, w, 3), dtype=torch.uint8, device=dev) if output != "float" else None
    out_f = torch.empty((n, 3, h, w), dtype=torch.float32, device=dev) if output != "u8" else None
    L.check(lib.idb_randaug(t.data_ptr(), n, h, w, flip.data_ptr(), d_op.data_ptr() if k else None, d_ia.data_ptr() if k else None,
                            d_fa.data_ptr() if k else None, k, out_u8.data_ptr() if out_u8 is not None else None,
                            out_f.data_ptr() if out_f is not None else None, torch.cuda.current_stream(dev).cuda_stream), "idb_randaug")
    return out_u8 if output == "u8" else out_f if output == "float" else (out_u8, out_f)


# ---- the reference's policy names -------------------------------------------------------------------------------------------------
_FLIP_ONLY = ("hf", "gan_hf", "nogan_hf")
_RA_4_16 = ("ra_4_16", "gan_ra_4_16", "nogan_ra_4_16")
SUPPORTED_POLICIES = _FLIP_ONLY + _RA_4_16 + ("num_mag_exp", "aug_operation_exp", "totensor")


class BatchTransform:
    """``t(images_u8, torch_generator=None, np_random=None) -> float32 NCHW`` on the device: [flip ->] RandAugment -> ToTensor ->
    Normalize of a uint8 [N, H, W, 3] batch, one launch.  ``flip_p`` None means no flip; ``randaug.num_ops`` 0 means no ops."""

    def __init__(self, randaug: RandAugment, flip_p: Optional[float]):
        self.randaug, self.flip_p = randaug, flip_p

    def __call__(self, images_u8, torch_generator: Optional[torch.Generator] = None,
                 np_random: Optional[np.random.RandomState] = None) -> torch.Tensor:
        plan = self.randaug.plan(int(images_u8.shape[0]), torch_generator, np_random, self.flip_p)
        return apply(images_u8, plan, "float")

    def __repr__(self) -> str:
        return f"BatchTransform(flip_p={self.flip_p}, num_ops={self.randaug.num_ops}, magnitude={self.randaug.magnitude})"


def get_conventional_aug_policy(aug_type: str, operation: str = "none", num_ops: int = 0, mag: int = 0) -> BatchTransform:
    """The reference's ``get_conventional_aug_policy`` (utils/augmentation.py:115-148) as a batch transform; names match
    case-insensitively, as upstream.
      hf, gan_hf, nogan_hf:                  flip only
      ra_4_16, gan_ra_4_16, nogan_ra_4_16:   flip + RandAugment(4, 16)
      num_mag_exp:                           flip + RandAugment(num_ops, mag)
      aug_operation_exp:                     flip + RandAugment(1, 9) — upstream ignores ``operation``: the restricted return of its
                                             ``_augmentation_space`` is commented out, so all 13 ops stay available
      totensor:                              no flip, no ops
    moco, faa_casia, faa_imgnet and mag_totensor (other transforms, FAA policies, an un-normalised tensor) are not built: ValueError."""
    aug = aug_type.lower()
    if aug in _FLIP_ONLY:
        return BatchTransform(RandAugment(0, 16), 0.5)
    if aug in _RA_4_16:
        return BatchTransform(RandAugment(4, 16), 0.5)
    if aug == "num_mag_exp":
        return BatchTransform(RandAugment(num_ops, mag), 0.5)
    if aug == "aug_operation_exp":
        return BatchTransform(RandAugment(1, 9), 0.5)
    if aug == "totensor":
        return BatchTransform(RandAugment(0, 16), None)
    raise ValueError(f"augmentation policy {aug_type!r} is not supported; supported: {', '.join(SUPPORTED_POLICIES)}")
