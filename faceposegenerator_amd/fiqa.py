"""CR-FIQA face-image quality scores — the "CR-FIQA (higher is better)" numbers of the reference's tables, computed there by
Evaluation/CR-FIQA/getQualityScore_FR_ID-Booth_12-2024.py (one score per image) and reduced by run_CRFIQA_ID-Booth.ipynb to a
``{"mean", "std"}`` record per dataset.

The script reads every image with ``cv2.imread`` (BGR), squashes the WHOLE image to 112x112 with ``cv2.resize`` (no detector, no
alignment, aspect ratio ignored), normalises by ``(x/255 - 0.5)/0.5`` and runs ``iresnet50(num_features=512, qs=1, use_se=False)`` of
Evaluation/CR-FIQA/iresnet.py: the ArcFace IResNet with one more layer, ``qs = Linear(512, 1)`` on the ``features`` BatchNorm1d output.
It returns ``(sklearn normalize(features), qs)`` and writes ``path + " " + str(qs)`` per image.

Engine (every step a HIP kernel of libidb_kernels.so):
  * idb_resize_linear_u8: OpenCV's 8-bit INTER_LINEAR, bit-exact with its fixed-point arithmetic as restated in
    tests/fiqa_oracle.py, with the RGB -> BGR swap on the way out.  The per-axis coefficient tables are built here on the host
    (``coef_tables``) in OpenCV's float32 / float64 types; the kernel is integer arithmetic only.  PARITY WITH A cv2 BINARY IS
    UNPINNED (cv2 is not a dependency of this project).
  * stem, blocks and head: the ArcFace code paths of arcface.py, unchanged (``FaceQuality`` subclasses ``ArcFace``).
  * idb_fiqa_tail: ``qs`` and the l2 normalisation, accumulated in double in a fixed order.

A stated difference: the reference runs this network in fp32 (``fp16=False``); this engine runs f16 (or bf16) operands with fp32
accumulation, as for ArcFace.  The deviation of the quality score this causes is printed by tests/test_fiqa_gpu.py for synthetic
weights and recorded in DESIGN.md; its effect with trained weights is unmeasured, and the notebook's 3-decimal record is NOT claimed to
be reproduced.  Trained weights are not shipped: PARITY WITH THE TRAINED NETWORK IS UNPINNED.

The host policy of the script and the notebook (natural sort, the seeded sample of 10 000 images, the score-file format, the mean / std
record) is restated below without cv2, sklearn, tqdm, pandas or seaborn; none of it touches the global random state."""
from __future__ import annotations

import os
import random
import re
from collections import OrderedDict
from typing import Dict, List, Sequence, Tuple

import numpy as np
import torch

from . import _hipnet as N
from . import _lib as L
from . import arcface as A

SD = Dict[str, torch.Tensor]

ARCHS = {k: A.ARCHS[k] for k in ("r18", "r34", "r50", "r100")}      # the reference runs iresnet50; iresnet100 is its other option
EMBED = A.EMBED
SIZE = A.SIZE
COEF_BITS = 11                                                      # OpenCV's INTER_RESIZE_COEF_BITS


def _check_arch(arch: str) -> None:
    if arch not in ARCHS:
        raise ValueError(f"unknown CR-FIQA arch {arch!r}; one of {sorted(ARCHS)}")


def param_shapes(arch: str = "r50") -> "OrderedDict[str, Tuple[int, ...]]":
    """State-dict layout of ``iresnet{N}(qs=1, use_se=False)``: arcface.param_shapes plus the quality head."""
    _check_arch(arch)
    out = A.param_shapes(arch)
    out["qs.weight"] = (1, EMBED)
    out["qs.bias"] = (1,)
    return out


def synth_weights(arch: str = "r50", seed: int = 0) -> SD:
    """arcface.synth_weights plus a quality head: ``qs.weight`` ~ randn / sqrt(512), ``qs.bias`` near 2 (scores of order 2, the range
    of the reference's tables)."""
    _check_arch(arch)
    sd = A.synth_weights(arch, seed)
    g = torch.Generator().manual_seed(seed + 7919)
    sd["qs.weight"] = torch.randn((1, EMBED), generator=g) * (1.0 / EMBED) ** 0.5
    sd["qs.bias"] = 2.0 + 0.1 * torch.randn((1,), generator=g)
    return sd


def check_state_dict(sd: SD, arch: str) -> None:
    """Strict keys and shapes (ValueError naming what is missing / unexpected).  SE blocks are refused: the reference never sets
    ``use_se``, and this engine has no kernel for them."""
    _check_arch(arch)
    se = sorted(k for k in sd if "se_block" in k)
    if se:
        raise ValueError(f"CR-FIQA {arch} state dict: se_block keys {se[:4]}{'...' if len(se) > 4 else ''} — SE blocks (use_se=True) are "
                         f"not supported")
    N.check_state_dict(sd, param_shapes(arch), f"CR-FIQA {arch}")


# ---- resize ---------------------------------------------------------------------------------------------------------------------
_TABLES: Dict[Tuple[int, int], Tuple[np.ndarray, np.ndarray]] = {}


def coef_tables(s: int, d: int) -> Tuple[np.ndarray, np.ndarray]:
    """OpenCV's INTER_LINEAR tables of one axis with ``s`` source and ``d`` destination samples -> (offsets int32 [d], coefficients
    int16 [d][2]), cached per (s, d).  In OpenCV's order and types: the position (i + 0.5) s / d - 0.5 in double, rounded to float32;
    its floor; the float32 fraction; both clamped at the ends (fraction 0 there); the taps (1 - f) 2048 and f 2048 as float32 products,
    rounded half to even."""
    s, d = int(s), int(d)
    if s < 1 or d < 1:
        raise ValueError(f"coef_tables: sizes must be >= 1, got {s} -> {d}")
    if (s, d) not in _TABLES:
        scale = np.float64(s) / np.float64(d)
        f = ((np.arange(d, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
        fl = np.floor(f)
        f = (f - fl).astype(np.float32)
        o = fl.astype(np.int64)
        f[o < 0] = 0
        o[o < 0] = 0
        f[o >= s - 1] = 0
        o[o >= s - 1] = s - 1
        one = np.float32(1 << COEF_BITS)
        c = np.stack([np.rint((np.float32(1) - f) * one), np.rint(f * one)], axis=1)
        assert c.dtype == np.float32
        _TABLES[(s, d)] = (o.astype(np.int32), c.astype(np.int16))
    return _TABLES[(s, d)]


_DEV_TABLES: Dict[Tuple[int, int, str], Tuple[torch.Tensor, torch.Tensor]] = {}


def _device_tables(s: int, d: int, device: torch.device) -> Tuple[torch.Tensor, torch.Tensor]:
    key = (s, d, str(device))
    if key not in _DEV_TABLES:
        o, c = coef_tables(s, d)
        _DEV_TABLES[key] = (torch.from_numpy(o).to(device), torch.from_numpy(c).to(device))
    return _DEV_TABLES[key]


def resize_linear_u8(images, dh: int, dw: int, swap_rb: bool = False, device=None) -> torch.Tensor:
    """``cv2.resize(img, (dw, dh))`` (INTER_LINEAR) of a uint8 NHWC batch [B, H, W, 3] -> uint8 [B, dh, dw, 3] on the GPU; ``swap_rb``
    exchanges channels 0 and 2 on the way out.  A host batch is uploaded to ``device`` (default cuda:0)."""
    t = images if torch.is_tensor(images) else torch.from_numpy(np.ascontiguousarray(images))
    if t.dtype != torch.uint8 or t.ndim != 4 or t.shape[3] != 3 or min(t.shape[:3]) < 1:
        raise ValueError(f"resize_linear_u8 expects a uint8 image batch [B, H, W, 3], got {t.dtype} {tuple(t.shape)}")
    if dh < 1 or dw < 1:
        raise ValueError(f"resize_linear_u8: destination size must be >= 1, got {dh} x {dw}")
    if not t.is_cuda:
        t = t.to(torch.device(device if device is not None else "cuda:0"))
    t = t.contiguous()
    lib = L.load()
    B, H, W = int(t.shape[0]), int(t.shape[1]), int(t.shape[2])
    ox, cx = _device_tables(W, int(dw), t.device)
    oy, cy = _device_tables(H, int(dh), t.device)
    out = torch.empty((B, int(dh), int(dw), 3), dtype=torch.uint8, device=t.device)
    step = 65535                                                   # the launch takes the batch as a grid dimension
    for b0 in range(0, B, step):
        n = min(step, B - b0)
        L.check(lib.idb_resize_linear_u8(t[b0:b0 + n].data_ptr(), n, H, W, ox.data_ptr(), cx.data_ptr(), oy.data_ptr(), cy.data_ptr(),
                                         int(dh), int(dw), int(bool(swap_rb)), out[b0:b0 + n].data_ptr(),
                                         torch.cuda.current_stream(t.device).cuda_stream), "idb_resize_linear_u8")
    return out


# ---- the network ----------------------------------------------------------------------------------------------------------------
def fold_weights(sd: SD, arch: str = "r50") -> Dict[str, torch.Tensor]:
    """arcface.fold_weights of the IResNet keys, plus ``qs.w`` [512] and ``qs.b`` [1] (fp32, as they are)."""
    check_state_dict(sd, arch)
    f = A.fold_weights({k: v for k, v in sd.items() if not k.startswith("qs.")}, arch)
    f["qs.w"] = sd["qs.weight"].float().reshape(EMBED).contiguous()
    f["qs.b"] = sd["qs.bias"].float().reshape(1).contiguous()
    return f


class FaceQuality(A.ArcFace):
    """Drop-in for the reference's ``feat, qs = self.model(imgs)``: float [B,3,112,112] (already (x/255 - 0.5)/0.5, BGR as the
    reference feeds it) -> (features [B,512] fp32, qs [B,1] fp32), and for its ``get_batch_feature`` on decoded images.

    ``FaceQuality.from_pretrained(path, arch="r50")`` loads a local ``.pth``; ``.to("cuda:N")`` uploads the folded weights.  The
    reference runs this network in fp32; here the convolutions take f16 (default) or bf16 operands with fp32 accumulation, the head
    and the tail are fp32 / double (see the module docstring: the quality-score deviation is recorded, not claimed away)."""

    NAME = "FaceQuality"

    def __init__(self, sd: SD, arch: str = "r50", torch_dtype: torch.dtype = torch.float16, chunk: int = 256):
        N.HipNet.__init__(self, torch_dtype, chunk)
        check_state_dict(sd, arch)
        self.arch = arch
        self._sd = {k: v.detach().cpu() for k, v in sd.items()}
        self._fw = fold_weights(self._sd, arch)

    @classmethod
    def from_state_dict(cls, sd: SD, arch: str = "r50", torch_dtype: torch.dtype = torch.float16) -> "FaceQuality":
        return cls(sd, arch, torch_dtype)

    @classmethod
    def from_pretrained(cls, path: str, arch: str = "r50", torch_dtype: torch.dtype = torch.float16) -> "FaceQuality":
        sd = torch.load(path, weights_only=True, map_location="cpu")
        return cls(sd, arch, torch_dtype)

    @classmethod
    def from_synthetic(cls, arch: str = "r50", seed: int = 0, torch_dtype: torch.dtype = torch.float16) -> "FaceQuality":
        return cls(synth_weights(arch, seed), arch, torch_dtype)

    # ---- device side ----------------------------------------------------------------------------------------------------------
    def tail(self, emb: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """embeddings fp32 [B,512] (the head's output) -> (l2-normalised embeddings [B,512], qs [B,1]), fp32."""
        self._need_device()
        emb = emb.to(self.device, dtype=torch.float32).contiguous()
        B, D = emb.shape
        qs = torch.empty((B, 1), dtype=torch.float32, device=self.device)
        nrm = torch.empty_like(emb)
        L.check(self.lib.idb_fiqa_tail(emb.data_ptr(), self.w["qs.w"].data_ptr(), self.w["qs.b"].data_ptr(), B, D, qs.data_ptr(),
                                       nrm.data_ptr(), self._stream()), "idb_fiqa_tail")
        return nrm, qs

    def resize(self, images: torch.Tensor) -> torch.Tensor:
        """uint8 RGB [B,H,W,3] on the device -> uint8 BGR [B,112,112,3]: cv2.imread's channel order and cv2.resize(image, (112, 112))."""
        return resize_linear_u8(images, SIZE, SIZE, swap_rb=True)

    def __call__(self, x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """float [B,3,112,112] normalised as (x/255 - 0.5)/0.5 -> (features [B,512] fp32, qs [B,1] fp32)."""
        if not torch.is_tensor(x) or x.ndim != 4 or tuple(x.shape[1:]) != (3, SIZE, SIZE) or x.shape[0] < 1:
            raise ValueError(f"FaceQuality expects [B,3,{SIZE},{SIZE}] input (the fc fixes 7x7), got {tuple(getattr(x, 'shape', ()))}")
        self._need_device()

        def run(xc):
            emb = self._forward(xc.to(self.device, dtype=torch.float32).contiguous(), False)
            return emb, self.tail(emb)[1]
        return self._chunked(x, run)

    def get_batch_feature(self, images_u8) -> Tuple[torch.Tensor, torch.Tensor]:
        """uint8 RGB NHWC images [B,H,W,3] (any H, W >= 1; host or device) -> (l2-normalised features [B,512], quality [B,1]), fp32 on
        the device: the reference's ``get_batch_feature`` from the decoded images on.  Runs in chunks of ``chunk`` images; a host
        batch is uploaded chunk by chunk."""
        t = images_u8 if torch.is_tensor(images_u8) else torch.from_numpy(np.ascontiguousarray(images_u8))
        if t.dtype != torch.uint8 or t.ndim != 4 or t.shape[3] != 3 or min(t.shape[:3]) < 1:
            raise ValueError(f"get_batch_feature expects a uint8 RGB image batch [B, H, W, 3], got {t.dtype} {tuple(t.shape)}")
        self._need_device()
        return self._chunked(t, lambda xc: self.tail(self._forward(self.resize(xc.to(self.device)), True)))


# ---- host policy of the script and the notebook ----------------------------------------------------------------------------------
def natural_keys(text: str) -> list:
    """The script's sort key: digit runs compare as integers (``re.split(r'(\\d+)', text)`` with the digit parts converted)."""
    return [int(c) if c.isdigit() else c for c in re.split(r"(\d+)", text)]


def list_images(folder: str) -> List[str]:
    """``os.listdir(folder)`` sorted by ``natural_keys``, joined to the folder (every entry, as the script takes them)."""
    return [os.path.join(folder, n) for n in sorted(os.listdir(folder), key=natural_keys)]


def sample_paths(paths: Sequence[str], n: int = 10000, seed: int = 7) -> List[str]:
    """What ``random.seed(seed); random.sample(paths, n)`` returns when there are more than ``n`` paths, else all of them unchanged.
    ``random.Random(seed)`` draws the same sample without touching the global generator."""
    paths = list(paths)
    return random.Random(seed).sample(paths, n) if len(paths) > n else paths


def load_image_rgb(path: str) -> np.ndarray:
    """One image file -> uint8 RGB [H, W, 3], decoded with Pillow and ``convert("RGB")``.  The reference decodes with ``cv2.imread``:
    PNG decoding is exact in both, but decoder parity for JPEG (the IDCT and chroma upsampling of the two libraries) is unpinned."""
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im.convert("RGB"))


def write_scores(path: str, image_paths: Sequence[str], quality) -> None:
    """The script's score file: ``image_path + " " + str(numpy.float32 score) + "\\n"`` per image."""
    q = np.asarray(quality.detach().cpu() if torch.is_tensor(quality) else quality, dtype=np.float32).reshape(-1)
    if q.shape[0] != len(image_paths):
        raise ValueError(f"write_scores: {len(image_paths)} paths for {q.shape[0]} scores")
    with open(path, "w") as f:
        for p, s in zip(image_paths, q):
            f.write(p.rstrip() + " " + str(s) + "\n")


def read_scores(path: str) -> List[float]:
    """The notebook's reader: ``float(line.split(" ")[-1])`` per line."""
    with open(path) as f:
        return [float(line.split(" ")[-1]) for line in f.readlines()]


def quality_summary(scores) -> Dict[str, float]:
    """The notebook's record: ``{"mean", "std"}`` of the scores in float64, the std with ddof = 1 (pandas' default; NaN for a single
    score), both rounded with ``np.round(., 3)``."""
    v = np.asarray(scores, dtype=np.float64).reshape(-1)
    mean = v.sum() / v.shape[0] if v.shape[0] else np.float64("nan")
    std = np.sqrt(((v - mean) ** 2).sum() / (v.shape[0] - 1)) if v.shape[0] > 1 else np.float64("nan")
    return {"mean": float(np.round(mean, 3)), "std": float(np.round(std, 3))}


def score_folder(model: FaceQuality, folder: str, out_txt: str, n: int = 10000, seed: int = 7, batch: int = 256) -> Dict[str, float]:
    """The script's loop for one dataset folder: list, sample, decode, ``get_batch_feature``, ``write_scores`` -> the summary of the
    written scores.  Images are scored ``batch`` at a time; a batch ends early where the image size changes (every image is squashed
    to 112x112 on its own, so sizes may differ)."""
    paths = sample_paths(list_images(folder), n, seed)
    if not paths:
        raise ValueError(f"score_folder: no files in {folder}")
    scores: List[torch.Tensor] = []
    pending: List[np.ndarray] = []

    def flush():
        if pending:
            scores.append(model.get_batch_feature(np.stack(pending))[1].reshape(-1).cpu())
            pending.clear()

    for p in paths:
        img = load_image_rgb(p)
        if pending and (len(pending) >= batch or pending[0].shape != img.shape):
            flush()
        pending.append(img)
    flush()
    write_scores(out_txt, paths, torch.cat(scores))
    return quality_summary(read_scores(out_txt))
