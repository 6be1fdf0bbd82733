"""DINOv2 ViT image features — the encoder behind the reference's dgm-eval run (Evaluation/dgm-eval/main_DGM_EVAL.ipynb:
``python -m dgm_eval ... --model dinov2 --metrics prdc vendi fd kd authpct``).  dgm-eval loads ``dinov2_vitl14`` from the hub, feeds
every image through ``Resize((224, 224), BICUBIC)`` on the PIL image, ``ToTensor`` and the ImageNet ``Normalize`` (its ``transform``
with ``clean_resize=False``) and stores ``model(x)`` — the final LayerNorm's class token, ``head = Identity`` — as one float32
``[N, D]`` matrix; all five metrics are CPU code over that matrix in the reference.  Here ``metrics.py`` computes them from that
matrix: PRDC, KD and AuthPct on the GPU (``idb_pair_*``), FD and per-class Vendi as float64 host code.

Neither ``dinov2`` nor ``dgm_eval`` is part of this project.  The state-dict layout, the position-embedding interpolation and the
block order below restate facebookresearch/dinov2's published ``vision_transformer.py`` (ViT-S/B/L with 14x14 patches, LayerScale,
no registers); no trained checkpoint is available to this project, so PARITY WITH TRAINED WEIGHTS IS UNPINNED.  The HIP path is checked
against tests/dinov2_oracle.py, a float64 restatement that is itself checked against transformers' ``Dinov2Model``, with seeded
synthetic weights.

Engine (every layer a HIP kernel of libidb_kernels.so), M = B * 257 rows in the operand dtype:
  * idb_resize_bicubic_aa_u8: Pillow-exact antialiased bicubic resize of the uint8 images to 224
  * idb_vit_patchify: ToTensor + Normalize fused, one 588-value row per 14x14 patch (K order [c][ky][kx]), zero-padded to K = 640
  * idb_gemm: the patch embedding (weight padded alike) with bias; idb_vit_tokens: class token and position embedding (interpolated
    from the checkpoint's 37x37 grid to 16x16 once at load, as upstream's interpolate_pos_encoding does per call)
  * per block: idb_layernorm (eps 1e-6), idb_gemm qkv with bias, idb_attention (non-causal, q / k / v as column slices of the qkv
    buffer), idb_gemm proj with the residual epilogue, idb_layernorm, idb_gemm fc1 with exact GELU, idb_gemm fc2 with the residual
    epilogue.  LayerScale is folded into proj and fc2 at load (W' = diag(gamma) W, b' = gamma b).
  * idb_vit_head: the final LayerNorm on the class-token rows alone, fp32 out.
"""
from __future__ import annotations

import math
from collections import OrderedDict
from typing import Dict, Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from . import _hipnet as N
from . import _lib as L

SD = Dict[str, torch.Tensor]

SIZE = 224
PATCH = 14
GRID = SIZE // PATCH                      # 16
NPATCH = GRID * GRID                      # 256
KPATCH = 3 * PATCH * PATCH                # 588
KPAD = 640                                # K of the patch-embedding GEMM (a multiple of 64)
HEAD_DIM = 64
EPS = 1e-6
MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
ARCHS = {"vits14": (384, 12, 6), "vitb14": (768, 12, 12), "vitl14": (1024, 24, 16)}      # name: (dim, depth, heads)
POS_GRID = 37                             # the checkpoints' position grid (518 / 14)


def gflops(dim: int, depth: int) -> float:
    """Multiply-adds x 2 of one image (patch embedding, blocks with attention), in GFLOP."""
    n = NPATCH + 1
    return (2 * NPATCH * KPATCH * dim + depth * (2 * n * 12 * dim * dim + 4 * n * n * dim)) / 1e9


def param_shapes(dim: int, depth: int, n0: int = POS_GRID * POS_GRID) -> "OrderedDict[str, Tuple[int, ...]]":
    """State-dict layout of DinoVisionTransformer (no registers, MLP ffn); mask_token is accepted and ignored."""
    out: "OrderedDict[str, Tuple[int, ...]]" = OrderedDict()
    out["cls_token"] = (1, 1, dim)
    out["pos_embed"] = (1, 1 + n0, dim)
    out["patch_embed.proj.weight"] = (dim, 3, PATCH, PATCH)
    out["patch_embed.proj.bias"] = (dim,)
    for i in range(depth):
        p = f"blocks.{i}."
        for n in ("norm1", "norm2"):
            out[p + n + ".weight"] = (dim,)
            out[p + n + ".bias"] = (dim,)
        out[p + "attn.qkv.weight"] = (3 * dim, dim)
        out[p + "attn.qkv.bias"] = (3 * dim,)
        out[p + "attn.proj.weight"] = (dim, dim)
        out[p + "attn.proj.bias"] = (dim,)
        out[p + "ls1.gamma"] = (dim,)
        out[p + "ls2.gamma"] = (dim,)
        out[p + "mlp.fc1.weight"] = (4 * dim, dim)
        out[p + "mlp.fc1.bias"] = (4 * dim,)
        out[p + "mlp.fc2.weight"] = (dim, 4 * dim)
        out[p + "mlp.fc2.bias"] = (dim,)
    out["norm.weight"] = (dim,)
    out["norm.bias"] = (dim,)
    return out


def synth_weights(seed: int = 0, arch: str = "vits14", depth: Optional[int] = None) -> SD:
    """Seeded synthetic weights in upstream's layout: linear / conv weights ~ N(0, 1 / fan_in), LayerNorm gamma ~ U(0.5, 1.5) and
    beta ~ N(0, 0.1), LayerScale gamma ~ U(0.05, 0.5), pos_embed (37x37 grid) and cls_token ~ N(0, 0.02), small biases."""
    if arch not in ARCHS:
        raise ValueError(f"unknown DINOv2 arch {arch!r}: one of {sorted(ARCHS)}")
    dim, full_depth, _ = ARCHS[arch]
    g = torch.Generator().manual_seed(seed)
    sd: SD = {}
    for name, shp in param_shapes(dim, depth or full_depth).items():
        if name in ("cls_token", "pos_embed"):
            sd[name] = 0.02 * torch.randn(shp, generator=g)
        elif name.endswith(".gamma"):
            sd[name] = 0.05 + 0.45 * torch.rand(shp, generator=g)
        elif ".norm" in name or name.startswith("norm."):
            sd[name] = 0.5 + torch.rand(shp, generator=g) if name.endswith("weight") else 0.1 * torch.randn(shp, generator=g)
        elif name.endswith(".weight"):
            sd[name] = torch.randn(shp, generator=g) * (1.0 / int(np.prod(shp[1:]))) ** 0.5
        else:
            sd[name] = 0.05 * torch.randn(shp, generator=g)
    sd["mask_token"] = torch.zeros(1, dim)
    return sd


def _normalize_keys(sd: SD) -> SD:
    """Flatten the chunked spelling ``blocks.{c}.{i}.`` (block_chunks > 0 checkpoints) to ``blocks.{i}.``."""
    out: SD = {}
    for k, v in sd.items():
        p = k.split(".")
        if p[0] == "blocks" and len(p) > 3 and p[1].isdigit() and p[2].isdigit():
            k = ".".join(["blocks", p[2]] + p[3:])
        out[k] = v
    return out


def infer_arch(sd: SD, num_heads: Optional[int] = None) -> Tuple[int, int, int, int]:
    """(dim, depth, heads, n0) from the shapes; raises ValueError for the variants this engine does not run."""
    sd = _normalize_keys(sd)
    if any(k.endswith("mlp.w12.weight") or k.endswith("mlp.w3.weight") for k in sd):
        raise ValueError("DINOv2 state dict has SwiGLU ffn keys (mlp.w12 / mlp.w3: vitg14); only the MLP variants vits14 / vitb14 / vitl14 run here")
    if "register_tokens" in sd:
        raise ValueError("DINOv2 state dict has register_tokens: the register-token variants are not supported")
    if "cls_token" not in sd or "pos_embed" not in sd or sd["cls_token"].ndim != 3 or sd["pos_embed"].ndim != 3:
        raise ValueError("DINOv2 state dict: missing keys ['cls_token' / 'pos_embed'] (or not 3-d)")
    dim = int(sd["cls_token"].shape[-1])
    known = {d: h for d, _, h in ARCHS.values()}
    heads = num_heads if num_heads is not None else known.get(dim)
    if heads is None:
        raise ValueError(f"DINOv2 state dict: embed dim {dim} is none of {sorted(known)} (vits14 / vitb14 / vitl14), so its head count is "
                         f"unknown; the attention kernel needs head_dim {HEAD_DIM}")
    if heads <= 0 or dim % heads or dim // heads != HEAD_DIM:
        raise ValueError(f"DINOv2: embed dim {dim} with {heads} heads gives head_dim {dim / heads:g}; the attention kernel needs head_dim {HEAD_DIM}")
    idx = {int(k.split(".")[1]) for k in sd if k.startswith("blocks.") and k.split(".")[1].isdigit()}
    depth = max(idx) + 1 if idx else 0
    if depth < 1:
        raise ValueError("DINOv2 state dict: missing keys ['blocks.0.*']")
    n0 = int(sd["pos_embed"].shape[1]) - 1
    if n0 < 1 or int(math.isqrt(n0)) ** 2 != n0:
        raise ValueError(f"DINOv2 state dict: pos_embed has {n0} patch positions, not a square grid")
    return dim, depth, heads, n0


def check_state_dict(sd: SD, num_heads: Optional[int] = None) -> Tuple[int, int, int, int]:
    """Strict keys and shapes of the inferred architecture: missing / unexpected / wrong-shaped keys raise ValueError naming them;
    mask_token is accepted and ignored.  Returns (dim, depth, heads, n0)."""
    arch = infer_arch(sd, num_heads)
    dim, depth, _, n0 = arch
    flat = {k: v for k, v in _normalize_keys(sd).items() if k != "mask_token"}
    N.check_state_dict(flat, param_shapes(dim, depth, n0), "DINOv2")
    return arch


def interpolate_pos_embed(pos: torch.Tensor, grid: int = GRID) -> torch.Tensor:
    """upstream's interpolate_pos_encoding for a grid x grid input, in the dtype of ``pos`` ([1, 1 + N0, D]): the identity when
    N0 == grid^2; else bicubic F.interpolate of the patch positions with scale_factor (grid + 0.1) / sqrt(N0), no antialias, the class
    position untouched."""
    n0 = pos.shape[1] - 1
    if n0 == grid * grid:
        return pos
    m = int(math.isqrt(n0))
    dim = pos.shape[-1]
    s = float(grid + 0.1) / math.sqrt(n0)
    pp = F.interpolate(pos[:, 1:].reshape(1, m, m, dim).permute(0, 3, 1, 2), scale_factor=(s, s), mode="bicubic", antialias=False)
    if tuple(pp.shape[-2:]) != (grid, grid):
        raise ValueError(f"position embedding {m}x{m} interpolates to {tuple(pp.shape[-2:])}, expected {grid}x{grid}")
    return torch.cat([pos[:, :1], pp.permute(0, 2, 3, 1).reshape(1, grid * grid, dim)], dim=1)


def fold_weights(sd: SD, num_heads: Optional[int] = None) -> Dict[str, torch.Tensor]:
    """The fp32 tensors the engine uploads (CPU; folding in float64).  Keys: ``patch.w`` [D][640] (the conv weight flattened [c][ky][kx],
    columns 588..639 zero) / ``patch.b``, ``cls`` [D], ``pos`` [257][D] (interpolated in fp32 as upstream does), per block ``{i}.ln1.g/b``,
    ``{i}.qkv.w/b``, ``{i}.proj.w/b`` and ``{i}.fc2.w/b`` (LayerScale folded in), ``{i}.ln2.g/b``, ``{i}.fc1.w/b``, and ``norm.g/b``.
    The engine rounds the ``.w`` matrices to the operand dtype."""
    dim, depth, _, _ = check_state_dict(sd, num_heads)
    sd = _normalize_keys(sd)
    f: Dict[str, torch.Tensor] = {}
    w = torch.zeros((dim, KPAD), dtype=torch.float64)
    w[:, :KPATCH] = sd["patch_embed.proj.weight"].double().reshape(dim, KPATCH)
    f["patch.w"], f["patch.b"] = w, sd["patch_embed.proj.bias"].double()
    pos = interpolate_pos_embed(sd["pos_embed"].float())
    f["cls"], f["pos"] = sd["cls_token"].double().reshape(dim), pos.reshape(NPATCH + 1, dim)
    for i in range(depth):
        p = f"blocks.{i}."
        for n, q in (("norm1", "ln1"), ("norm2", "ln2")):
            f[f"{i}.{q}.g"], f[f"{i}.{q}.b"] = sd[p + n + ".weight"].double(), sd[p + n + ".bias"].double()
        f[f"{i}.qkv.w"], f[f"{i}.qkv.b"] = sd[p + "attn.qkv.weight"].double(), sd[p + "attn.qkv.bias"].double()
        f[f"{i}.fc1.w"], f[f"{i}.fc1.b"] = sd[p + "mlp.fc1.weight"].double(), sd[p + "mlp.fc1.bias"].double()
        for lin, ls, q in (("attn.proj", "ls1", "proj"), ("mlp.fc2", "ls2", "fc2")):
            g = sd[p + ls + ".gamma"].double()
            f[f"{i}.{q}.w"] = g[:, None] * sd[p + lin + ".weight"].double()
            f[f"{i}.{q}.b"] = g * sd[p + lin + ".bias"].double()
    f["norm.g"], f["norm.b"] = sd["norm.weight"].double(), sd["norm.bias"].double()
    return {k: v.float().contiguous() for k, v in f.items()}


class DinoV2(N.HipNet):
    """Drop-in for the hub's ``dinov2_vit{s,b,l}14``: ``model(x)`` maps normalised fp32 [B,3,224,224] to the fp32 [B, D] class-token
    features of upstream's ``forward(x)``; ``features_u8(images)`` maps uint8 RGB [B,S,S,3] images through dgm-eval's transform
    (bicubic resize to 224, ToTensor, ImageNet Normalize) to the same.  ``DinoV2.from_pretrained(path)`` loads a local ``.pth``; nothing
    is ever downloaded.  Batches of any size >= 1 run in chunks of ``chunk`` images."""

    NAME = "DinoV2"

    def __init__(self, sd: SD, torch_dtype: torch.dtype = torch.float16, chunk: int = 64, num_heads: Optional[int] = None):
        super().__init__(torch_dtype, chunk)
        sd = {k: v.detach().cpu() for k, v in sd.items()}
        self.dim, self.depth, self.heads, _ = check_state_dict(sd, num_heads)
        self._fw = fold_weights(sd, num_heads)

    @classmethod
    def from_state_dict(cls, sd: SD, torch_dtype: torch.dtype = torch.float16, chunk: int = 64, num_heads: Optional[int] = None) -> "DinoV2":
        return cls(sd, torch_dtype, chunk, num_heads)

    @classmethod
    def from_pretrained(cls, path: str, torch_dtype: torch.dtype = torch.float16, chunk: int = 64) -> "DinoV2":
        return cls(torch.load(path, weights_only=True, map_location="cpu"), torch_dtype, chunk)

    @classmethod
    def from_synthetic(cls, seed: int = 0, arch: str = "vits14", depth: Optional[int] = None, torch_dtype: torch.dtype = torch.float16,
                       chunk: int = 64) -> "DinoV2":
        return cls(synth_weights(seed, arch, depth), torch_dtype, chunk)

    # ---- device side ----------------------------------------------------------------------------------------------------------
    def _operand(self, key: str) -> bool:
        return key.endswith(".w")

    def linear(self, x: torch.Tensor, key: str, act: int = 0, residual: Optional[torch.Tensor] = None) -> torch.Tensor:
        """x [M][K] operand dtype -> x W^T + b (+ residual, or exact GELU with act = 1) [M][n]: one idb_gemm."""
        wt, bt = self.w[key + ".w"], self.w[key + ".b"]
        n, k = wt.shape
        m = x.shape[0]
        out = torch.empty((m, n), dtype=self.tdt, device=self.device)
        self._gemm([(x.data_ptr(), k, 1, 1, 1)], wt.data_ptr(), n, m, 1, 1, bias=bt.data_ptr(), out=out.data_ptr(), out_ld=n, act=act,
                   residual=None if residual is None else residual.data_ptr())
        return out

    def layernorm(self, x: torch.Tensor, key: str) -> torch.Tensor:
        out = torch.empty_like(x)
        L.check(self.lib.idb_layernorm(x.data_ptr(), out.data_ptr(), x.shape[0], x.shape[1], EPS, self.w[key + ".g"].data_ptr(),
                                       self.w[key + ".b"].data_ptr(), self.dt, self._stream()), "idb_layernorm")
        return out

    def resize(self, images: torch.Tensor) -> torch.Tensor:
        """uint8 [B,S,S,3] -> Pillow bicubic resize to [B,224,224,3] uint8."""
        images = images.contiguous()
        B, S = images.shape[0], images.shape[1]
        out = torch.empty((B, SIZE, SIZE, 3), dtype=torch.uint8, device=self.device)
        L.check(self.lib.idb_resize_bicubic_aa_u8(images.data_ptr(), B, S, SIZE, out.data_ptr(), self._stream()), "idb_resize_bicubic_aa_u8")
        return out

    def patchify(self, x: torch.Tensor, u8: bool) -> torch.Tensor:
        """uint8 [B,224,224,3] (u8) or normalised fp32 [B,3,224,224] -> [B * 256][640] operand dtype."""
        x = x.contiguous()
        B = x.shape[0]
        out = torch.empty((B * NPATCH, KPAD), dtype=self.tdt, device=self.device)
        L.check(self.lib.idb_vit_patchify(x.data_ptr(), int(u8), B, out.data_ptr(), self.dt, self._stream()), "idb_vit_patchify")
        return out

    def patch_tokens(self, x: torch.Tensor, u8: bool) -> torch.Tensor:
        """Patch embedding, class token and position embedding: -> [B * 257][D] operand dtype."""
        B = x.shape[0]
        pe = self.linear(self.patchify(x, u8), "patch")
        out = torch.empty((B * (NPATCH + 1), self.dim), dtype=self.tdt, device=self.device)
        L.check(self.lib.idb_vit_tokens(pe.data_ptr(), self.w["cls"].data_ptr(), self.w["pos"].data_ptr(), out.data_ptr(), B, NPATCH, self.dim,
                                        self.dt, self._stream()), "idb_vit_tokens")
        return out

    def block(self, i: int, x: torch.Tensor) -> torch.Tensor:
        """Block i on x [B * 257][D]."""
        d, n = self.dim, NPATCH + 1
        B = x.shape[0] // n
        qkv = self.linear(self.layernorm(x, f"{i}.ln1"), f"{i}.qkv")
        o = torch.empty((B * n, d), dtype=self.tdt, device=self.device)
        p, es = qkv.data_ptr(), qkv.element_size()
        L.check(self.lib.idb_attention(p, 3 * d, p + d * es, p + 2 * d * es, 3 * d, o.data_ptr(), d, B, self.heads, n, n, n, HEAD_DIM ** -0.5,
                                       0, self.dt, self._stream()), "idb_attention")
        x = self.linear(o, f"{i}.proj", residual=x)
        m = self.linear(self.layernorm(x, f"{i}.ln2"), f"{i}.fc1", act=1)
        return self.linear(m, f"{i}.fc2", residual=x)

    def head(self, x: torch.Tensor) -> torch.Tensor:
        """[B * 257][D] -> the final LayerNorm of each image's class token, fp32 [B, D]."""
        B = x.shape[0] // (NPATCH + 1)
        out = torch.empty((B, self.dim), dtype=torch.float32, device=self.device)
        L.check(self.lib.idb_vit_head(x.data_ptr(), NPATCH + 1, B, self.dim, self.w["norm.g"].data_ptr(), self.w["norm.b"].data_ptr(), EPS,
                                      out.data_ptr(), self.dt, self._stream()), "idb_vit_head")
        return out

    def _forward(self, x: torch.Tensor, u8: bool) -> Tuple[torch.Tensor]:
        t = self.patch_tokens(self.resize(x) if u8 else x, u8)
        for i in range(self.depth):
            t = self.block(i, t)
        return (self.head(t),)

    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        """float [B,3,224,224] normalised with the ImageNet mean / std -> class-token features [B, D] fp32."""
        if not torch.is_tensor(x) or x.ndim != 4 or tuple(x.shape[1:]) != (3, SIZE, SIZE) or x.shape[0] < 1:
            raise ValueError(f"DinoV2 expects [B,3,{SIZE},{SIZE}] input, got {tuple(getattr(x, 'shape', ()))}")
        self._need_device()
        return self._chunked(x.to(self.device, dtype=torch.float32).contiguous(), lambda xc: self._forward(xc, False))[0]

    def features_u8(self, images) -> torch.Tensor:
        """uint8 RGB [B,S,S,3] (numpy or tensor) -> class-token features [B, D] fp32, through dgm-eval's transform."""
        t = torch.as_tensor(np.asarray(images)) if not torch.is_tensor(images) else images
        if t.dtype != torch.uint8 or t.ndim != 4 or t.shape[-1] != 3 or t.shape[0] < 1:
            raise ValueError(f"features_u8 expects uint8 [B,S,S,3] images, got {t.dtype} {tuple(t.shape)}")
        if t.shape[1] != t.shape[2]:
            raise ValueError(f"features_u8 expects square images, got {t.shape[1]}x{t.shape[2]}")
        if resize_taps(int(t.shape[1])) > RESIZE_TAPS:
            raise ValueError(f"features_u8: the bicubic resize {t.shape[1]} -> {SIZE} needs {resize_taps(int(t.shape[1]))} taps, the kernel "
                             f"holds {RESIZE_TAPS}")
        self._need_device()
        return self._chunked(t.to(self.device).contiguous(), lambda xc: self._forward(xc, True))[0]


RESIZE_TAPS = 16                          # RS_KMAX of csrc/idb_pose.hip


def resize_taps(s: int, d: int = SIZE) -> int:
    """Taps per axis of Pillow's bicubic resize s -> d (Resample.c's ksize)."""
    return int(math.ceil(2.0 * max(s / d, 1.0))) * 2 + 1
