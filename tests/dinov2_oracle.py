"""float64 torch / numpy restatement of the DINOv2 feature path (facebookresearch/dinov2 DinoVisionTransformer as dgm-eval runs it),
on the hub's state-dict layout and written from the architecture alone: a numpy restatement of Pillow's antialiased bicubic resize,
ToTensor + Normalize, the position-embedding interpolation, the patch embedding as an unfold + matmul, pre-LN blocks with UNFOLDED
LayerScale, and the final LayerNorm's class token.  test_dinov2_cpu.py checks it against transformers' Dinov2Model.

``emulate`` = torch.float16 / torch.bfloat16 rounds to that dtype at exactly the points where the device stores an operand-dtype
tensor: the patchify output, every GEMM / attention / LayerNorm output (the token assembly included) and the GEMM weights — proj and
fc2 with LayerScale folded in first, as the engine folds them.  Everything between two such points stays float64, so the difference to
the plain float64 run is the error of the storage format alone; the GPU tests size their bounds with it."""
from __future__ import annotations

import math
from typing import Optional

import numpy as np
import torch
import torch.nn.functional as F

PREC = 22
SIZE, PATCH, GRID = 224, 14, 16
EPS = 1e-6
MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)


def _r(x: torch.Tensor, emulate: Optional[torch.dtype]) -> torch.Tensor:
    return x if emulate is None else x.to(emulate).double()


# ---- Pillow resize (libImaging/Resample.c, 8 bits per channel, BICUBIC), restated ------------------------------------------------
def _bicubic(x: float) -> float:
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def resize_coeffs(insz: int, outsz: int) -> np.ndarray:
    """Integer coefficient matrix [out][in] (fixed point, PREC fraction bits) of one axis."""
    scale = insz / outsz
    fs = max(scale, 1.0)
    support, ss = 2.0 * fs, 1.0 / fs
    K = np.zeros((outsz, insz), dtype=np.int64)
    for o in range(outsz):
        center = (o + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), insz)
        w = [_bicubic((x + xmin - center + 0.5) * ss) for x in range(xmax - xmin)]
        tot = 0.0
        for v in w:
            tot += v
        for x, v in enumerate(w):
            v = v / tot if tot != 0.0 else v
            K[o, xmin + x] = int(-0.5 + v * (1 << PREC)) if v < 0 else int(0.5 + v * (1 << PREC))
    return K


def _pass(img: np.ndarray, K: np.ndarray) -> np.ndarray:
    """Resample axis 1 of [A][in][3] with K -> [A][out][3] clipped to 0..255."""
    acc = np.einsum("oi,aic->aoc", K, img.astype(np.int64), optimize=True) + (1 << (PREC - 1))
    return np.clip(acc >> PREC, 0, 255)


def resize_pil_u8(img: np.ndarray, size: int = SIZE) -> np.ndarray:
    """uint8 [S][S][3] -> Image.resize((size, size), BICUBIC) equivalent, uint8 [size][size][3]."""
    K = resize_coeffs(img.shape[0], size)
    h = _pass(img, K)                                  # [S rows][size][3]: horizontal pass, clipped to 8 bits
    v = _pass(h.transpose(1, 0, 2), K)                 # [size cols][size rows][3]: vertical pass
    return v.transpose(1, 0, 2).astype(np.uint8)


def smooth_images(n: int = 4, seed: int = 3, size: int = 512) -> np.ndarray:
    """Smooth random uint8 RGB images [n][size][size][3] (upsampled 6x6 noise)."""
    low = torch.rand(n, 3, 6, 6, generator=torch.Generator().manual_seed(seed))
    up = F.interpolate(low, size=size, mode="bilinear", align_corners=False).permute(0, 2, 3, 1) * 255
    return np.ascontiguousarray(up.round().clamp(0, 255).to(torch.uint8).numpy())


def to_tensor_normalized(img_u8: np.ndarray) -> torch.Tensor:
    """uint8 [B][H][W][3] -> ToTensor + Normalize(ImageNet), float64 NCHW."""
    x = torch.from_numpy(np.ascontiguousarray(img_u8)).permute(0, 3, 1, 2).double() / 255.0
    return (x - torch.tensor(MEAN, dtype=torch.float64).view(1, 3, 1, 1)) / torch.tensor(STD, dtype=torch.float64).view(1, 3, 1, 1)


def transform(images_u8: np.ndarray) -> torch.Tensor:
    """dgm-eval's transform with clean_resize=False on uint8 [B][S][S][3]: bicubic resize to 224, ToTensor, Normalize."""
    return to_tensor_normalized(np.stack([resize_pil_u8(im) for im in images_u8]))


# ---- network ------------------------------------------------------------------------------------------------------------------
def interpolate_pos(pos: torch.Tensor, grid: int = GRID) -> torch.Tensor:
    """interpolate_pos_encoding for a grid x grid input on pos_embed [1][1 + N0][D], float64."""
    pos = pos.double()
    n0 = pos.shape[1] - 1
    if n0 == grid * grid:
        return pos
    m = int(round(math.sqrt(n0)))
    sx = float(grid + 0.1) / math.sqrt(n0)
    pp = pos[:, 1:].reshape(1, m, m, -1).permute(0, 3, 1, 2)
    pp = F.interpolate(pp, scale_factor=(sx, sx), mode="bicubic", antialias=False)
    assert pp.shape[-1] == grid and pp.shape[-2] == grid
    return torch.cat([pos[:, :1], pp.permute(0, 2, 3, 1).reshape(1, grid * grid, -1)], dim=1)


def patchify(x: torch.Tensor) -> torch.Tensor:
    """[B,3,224,224] -> [B,256,588]: patches in row-major order, each flattened [c][ky][kx]."""
    B = x.shape[0]
    p = x.reshape(B, 3, GRID, PATCH, GRID, PATCH).permute(0, 2, 4, 1, 3, 5)
    return p.reshape(B, GRID * GRID, 3 * PATCH * PATCH)


def patch_tokens(sd, x: torch.Tensor, emulate=None) -> torch.Tensor:
    """Normalised [B,3,224,224] -> tokens [B,257,D]: patch embedding, class token, position embedding."""
    w = sd["patch_embed.proj.weight"].double()
    D = w.shape[0]
    p = _r(patchify(x.double()), emulate)
    pe = _r(p @ _r(w.reshape(D, -1), emulate).T + sd["patch_embed.proj.bias"].double(), emulate)
    pos = interpolate_pos(sd["pos_embed"])
    cls = sd["cls_token"].double().expand(x.shape[0], -1, -1)
    return _r(torch.cat([cls, pe], dim=1) + pos, emulate)


def _ln(x, sd, key):
    return F.layer_norm(x, (x.shape[-1],), sd[key + ".weight"].double(), sd[key + ".bias"].double(), EPS)


def block(sd, i: int, x: torch.Tensor, heads: int, emulate=None) -> torch.Tensor:
    """Block i on tokens [B,n,D] (float64)."""
    p = f"blocks.{i}."
    B, n, D = x.shape
    g1, g2 = sd[p + "ls1.gamma"].double(), sd[p + "ls2.gamma"].double()
    wp, bp = sd[p + "attn.proj.weight"].double(), sd[p + "attn.proj.bias"].double()
    w2, b2 = sd[p + "mlp.fc2.weight"].double(), sd[p + "mlp.fc2.bias"].double()
    h = _r(_ln(x, sd, p + "norm1"), emulate)
    qkv = _r(h @ _r(sd[p + "attn.qkv.weight"].double(), emulate).T + sd[p + "attn.qkv.bias"].double(), emulate)
    q, k, v = qkv.reshape(B, n, 3, heads, D // heads).permute(2, 0, 3, 1, 4)
    a = torch.softmax(q @ k.transpose(-1, -2) * (D // heads) ** -0.5, dim=-1) @ v
    o = _r(a.transpose(1, 2).reshape(B, n, D), emulate)
    if emulate is None:
        x = x + g1 * (o @ wp.T + bp)
    else:                                              # the engine's form: LayerScale folded, the folded weight rounded
        x = _r(o @ _r(g1[:, None] * wp, emulate).T + g1 * bp + x, emulate)
    h = _r(_ln(x, sd, p + "norm2"), emulate)
    m = _r(F.gelu(h @ _r(sd[p + "mlp.fc1.weight"].double(), emulate).T + sd[p + "mlp.fc1.bias"].double()), emulate)
    if emulate is None:
        return x + g2 * (m @ w2.T + b2)
    return _r(m @ _r(g2[:, None] * w2, emulate).T + g2 * b2 + x, emulate)


def head(sd, x: torch.Tensor) -> torch.Tensor:
    """Tokens [B,n,D] -> the final LayerNorm's class token [B,D] (x_norm_clstoken; head = Identity)."""
    return _ln(x[:, 0], sd, "norm")


def depth_of(sd) -> int:
    return 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("blocks."))


def forward(sd, x: torch.Tensor, heads: int, emulate=None) -> torch.Tensor:
    """Normalised [B,3,224,224] -> features [B,D], float64."""
    t = patch_tokens(sd, x, emulate)
    for i in range(depth_of(sd)):
        t = block(sd, i, t, heads, emulate)
    return head(sd, t)


def features_u8(sd, images_u8: np.ndarray, heads: int, emulate=None) -> torch.Tensor:
    return forward(sd, transform(images_u8), heads, emulate)
