"""ArcFace IResNet identity embeddings for aligned 112x112 face crops — the network behind every identity measurement of the
reference (extract_ArcFace_embeds.py, the genuine/impostor scoring of Evaluation/PyEER_analysis, the identity loss of
train_ID-Booth.py), loaded there by ArcFace_functions.prepare_locked_ArcFace_model and run under fp16 autocast.

Architecture (insightface arcface_torch ``iresnet.py``, restated): stem conv 3->64 + BN + PReLU; four stages of ``IBasicBlock``
(planes 64/128/256/512, first block stride 2); block = BN -> conv3x3 -> BN -> PReLU -> conv3x3 (stride s) -> BN, plus the identity
or a 1x1 stride-s conv + BN; head BN -> flatten (NCHW) -> fc 25088->512 in fp32 -> BatchNorm1d.  Trained weights are not shipped:
PARITY WITH THE TRAINED NETWORK IS UNPINNED; the HIP path is checked against tests/arcface_oracle.py with seeded synthetic weights.

Engine (every layer a HIP kernel of libidb_kernels.so):
  * stem: idb_arcface_stem (VALU; uint8 crops with the preprocessing fused, or normalised fp32 NCHW)
  * block conv1 (+bn2, PReLU): idb_gemm with act = 2, reading the block's ``bn1(x)``
  * block conv2 (+bn3) + identity: idb_gemm with the residual, or with the downsample as a second, stride-2 1x1 K segment; its
    second output ``out2`` is the NEXT block's bn1 applied to the rounded x — bn1 sits before a zero-padded conv, so its shift
    cannot fold into a bias (the padded taps must see 0, not the shift)
  * head: bn2, fc and features folded into one fp32 [512][25088] matrix (columns in NHWC order), idb_arcface_head.
"""
from __future__ import annotations

from collections import OrderedDict
from functools import partial
from typing import Dict, List, Sequence, Tuple

import numpy as np
import torch

from . import _hipnet as N
from . import _lib as L

SD = Dict[str, torch.Tensor]

ARCHS = {"r18": [2, 2, 2, 2], "r34": [3, 4, 6, 3], "r50": [3, 4, 14, 3], "r100": [3, 13, 30, 3], "r200": [6, 26, 60, 6]}
PLANES = [64, 128, 256, 512]
EMBED = 512
SIZE = 112
EPS = 1e-5
_BN = ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")


def _check_arch(arch: str) -> List[int]:
    if arch not in ARCHS:
        raise ValueError(f"unknown ArcFace arch {arch!r}; one of {sorted(ARCHS)}")
    return ARCHS[arch]


def _bn_shapes(out, key: str, c: int) -> None:
    for f in _BN:
        out[f"{key}.{f}"] = () if f == "num_batches_tracked" else (c,)


def trunk_param_shapes(layers: Sequence[int]) -> "OrderedDict[str, Tuple[int, ...]]":
    """Key names and shapes of the trunk (everything of ``param_shapes`` in front of ``bn2``) for a list of block counts."""
    out: "OrderedDict[str, Tuple[int, ...]]" = OrderedDict()
    out["conv1.weight"] = (64, 3, 3, 3)
    _bn_shapes(out, "bn1", 64)
    out["prelu.weight"] = (64,)
    cin = 64
    for i, (nb, planes) in enumerate(zip(layers, PLANES)):
        for j in range(nb):
            k = f"layer{i + 1}.{j}"
            c = cin if j == 0 else planes
            _bn_shapes(out, f"{k}.bn1", c)
            out[f"{k}.conv1.weight"] = (planes, c, 3, 3)
            _bn_shapes(out, f"{k}.bn2", planes)
            out[f"{k}.prelu.weight"] = (planes,)
            out[f"{k}.conv2.weight"] = (planes, planes, 3, 3)
            _bn_shapes(out, f"{k}.bn3", planes)
            if j == 0:
                out[f"{k}.downsample.0.weight"] = (planes, c, 1, 1)
                _bn_shapes(out, f"{k}.downsample.1", planes)
        cin = planes
    return out


def param_shapes(arch: str = "r100") -> "OrderedDict[str, Tuple[int, ...]]":
    """State-dict layout of ``iresnet{N}`` (key names and shapes of the module; num_batches_tracked is a 0-d buffer)."""
    out = trunk_param_shapes(_check_arch(arch))
    _bn_shapes(out, "bn2", 512)
    out["fc.weight"] = (EMBED, 512 * 49)
    out["fc.bias"] = (EMBED,)
    _bn_shapes(out, "features", EMBED)
    return out


def synth_weights(arch: str = "r100", seed: int = 0) -> SD:
    """Seeded synthetic weights that keep all residual blocks stable.  Uses fan-in-scaled convs, damped bn3 gammas and running
    variances in [0.5, 2].  Every BN shift is non-zero, and the bn1 shifts are large (|beta| 0.5-2) so that a folded-bias
    implementation of bn1 shows on the border ring.  PReLU slopes are in [0.05, 0.4].  (The reference's own N(0, 0.1) init explodes.)"""
    g = torch.Generator().manual_seed(seed)
    sd: SD = {}
    for name, shp in param_shapes(arch).items():
        if name.endswith("num_batches_tracked"):
            sd[name] = torch.tensor(0, dtype=torch.int64)
            continue
        if name.endswith("running_var"):
            sd[name] = 0.5 + 1.5 * torch.rand(shp, generator=g)
        elif name.endswith("running_mean"):
            sd[name] = 0.2 * torch.randn(shp, generator=g)
        elif "prelu" in name:
            sd[name] = 0.05 + 0.35 * torch.rand(shp, generator=g)
        elif name == "fc.bias":
            sd[name] = 0.1 * torch.randn(shp, generator=g)
        elif name.endswith(".weight") and len(shp) >= 2:
            fan = int(np.prod(shp[1:]))
            sd[name] = torch.randn(shp, generator=g) * (1.0 / fan) ** 0.5
        elif name.endswith(".weight"):                            # BN gammas
            damp = 0.15 if name.endswith("bn3.weight") else 1.0
            sd[name] = damp * (0.8 + 0.4 * torch.rand(shp, generator=g))
        else:                                                     # BN betas: non-zero, large for bn1
            sign = torch.where(torch.rand(shp, generator=g) < 0.5, -1.0, 1.0)
            if name.endswith("bn1.bias") and name.startswith("layer"):
                sd[name] = sign * (0.5 + 1.5 * torch.rand(shp, generator=g))
            else:
                sd[name] = sign * (0.05 + 0.2 * torch.rand(shp, generator=g))
    return sd


def check_state_dict(sd: SD, arch: str) -> None:
    """Strict keys and shapes: missing / unexpected keys raise ValueError naming them; num_batches_tracked is accepted and ignored."""
    N.check_state_dict(sd, param_shapes(arch), f"ArcFace {arch}")


_affine = partial(N.bn_affine, eps=EPS)          # eval-mode BatchNorm as y = a x + b (float64)
_pack = N.pack_conv


def fold_weights(sd: SD, arch: str = "r100") -> Dict[str, torch.Tensor]:
    """The fp32 tensors the engine uploads (CPU, folded in float64).  Keys:
      stem.{w [64][27], b, slope, out2_scale, out2_shift}         conv1 + bn1 folded; out2 = layer1.0.bn1
      layer{i}.{j}.conv1.{w [planes][9 cin], b, slope}            bn2 folded into conv1, PReLU slope
      layer{i}.{j}.conv2.{w [planes][9 planes (+ cin)], b}        bn3 folded; first block: the downsample conv + BN as a second K
                                                                  segment, bias = the sum of the two shifts
      layer{i}.{j}.out2_{scale,shift}                             the NEXT block's bn1 (absent on the last block)
      fc.{w [512][25088], b}                                      head bn2, fc and features in one matrix, columns in NHWC order
    Conv weights are in idb_gemm's [n][tap][channel] layout; the engine rounds them to the operand dtype."""
    check_state_dict(sd, arch)
    layers = ARCHS[arch]
    f: Dict[str, torch.Tensor] = {}
    blocks = [f"layer{i + 1}.{j}" for i, nb in enumerate(layers) for j in range(nb)]
    a, b = _affine(sd, "bn1")
    f["stem.w"] = _pack(sd["conv1.weight"].double() * a[:, None, None, None])
    f["stem.b"] = b
    f["stem.slope"] = sd["prelu.weight"].double()
    f["stem.out2_scale"], f["stem.out2_shift"] = _affine(sd, f"{blocks[0]}.bn1")
    for bi, k in enumerate(blocks):
        a2, b2 = _affine(sd, f"{k}.bn2")
        f[f"{k}.conv1.w"] = _pack(sd[f"{k}.conv1.weight"].double() * a2[:, None, None, None])
        f[f"{k}.conv1.b"] = b2
        f[f"{k}.conv1.slope"] = sd[f"{k}.prelu.weight"].double()
        a3, b3 = _affine(sd, f"{k}.bn3")
        w2 = _pack(sd[f"{k}.conv2.weight"].double() * a3[:, None, None, None])
        if f"{k}.downsample.0.weight" in sd:
            ad, bd = _affine(sd, f"{k}.downsample.1")
            w2 = torch.cat([w2, _pack(sd[f"{k}.downsample.0.weight"].double() * ad[:, None, None, None])], dim=1)
            b3 = b3 + bd
        f[f"{k}.conv2.w"], f[f"{k}.conv2.b"] = w2, b3
        if bi + 1 < len(blocks):
            f[f"{k}.out2_scale"], f[f"{k}.out2_shift"] = _affine(sd, f"{blocks[bi + 1]}.bn1")
    # head: features(fc(bn2(x))) = s (W (a x + c) + bfc) + t, with x in NCHW-flattened order k = ch*49 + p
    ah, ch = _affine(sd, "bn2")
    s, t = _affine(sd, "features")
    W = sd["fc.weight"].double().view(EMBED, 512, 49)                            # [n][ch][p]
    bias = s * (torch.einsum("ncp,c->n", W, ch) + sd["fc.bias"].double()) + t
    Wf = W * ah[None, :, None] * s[:, None, None]
    f["fc.w"] = Wf.permute(0, 2, 1).reshape(EMBED, 49 * 512)                     # NHWC order: p*512 + ch
    f["fc.b"] = bias
    return {k: v.float().contiguous() for k, v in f.items()}


class ArcFace(N.HipNet):
    """Drop-in for the reference's ``arcface_model(img)``: float [B,3,112,112] (already (x/255 - 0.5)/0.5) -> [B,512] fp32.

    ``ArcFace.from_pretrained(path)`` loads a local ``.pth`` (e.g. ArcFace_r100_ms1mv3_backbone.pth); ``.to("cuda:N")`` uploads the
    folded weights; ``embed_u8(crops)`` takes uint8 NHWC [B,112,112,3] crops (face_align.norm_crop output) with the preprocessing on
    the GPU.  Batches of any size >= 1 run in chunks of ``chunk`` faces."""

    NAME = "ArcFace"
    DTYPES = "float16 (the reference's autocast dtype) or bfloat16"

    def __init__(self, sd: SD, arch: str = "r100", torch_dtype: torch.dtype = torch.float16, chunk: int = 256):
        super().__init__(torch_dtype, chunk)
        check_state_dict(sd, arch)
        self.arch = arch
        self._sd = {k: v.detach().cpu() for k, v in sd.items()}
        self._fw = fold_weights(self._sd, arch)

    @classmethod
    def from_state_dict(cls, sd: SD, arch: str = "r100", torch_dtype: torch.dtype = torch.float16) -> "ArcFace":
        return cls(sd, arch, torch_dtype)

    @classmethod
    def from_pretrained(cls, path: str, arch: str = "r100", torch_dtype: torch.dtype = torch.float16) -> "ArcFace":
        sd = torch.load(path, weights_only=True, map_location="cpu")
        return cls(sd, arch, torch_dtype)

    @classmethod
    def from_synthetic(cls, arch: str = "r100", seed: int = 0, torch_dtype: torch.dtype = torch.float16) -> "ArcFace":
        return cls(synth_weights(arch, seed), arch, torch_dtype)

    # ---- device side ----------------------------------------------------------------------------------------------------------
    def _operand(self, key: str) -> bool:
        return key.endswith("conv1.w") or key.endswith("conv2.w")

    def gemm(self, srcs, w, n, batch, oh, ow, bias, stride=1, slope=None, residual=None, out2=None, split_k=0, tile=0):
        """One idb_gemm: srcs = [(tensor NHWC, channels, taps, in_h, in_w)].  Returns (out, out2 or None)."""
        out = torch.empty((batch, oh, ow, n), dtype=self.tdt, device=self.device)
        f = dict(bias=bias.data_ptr(), out=out.data_ptr(), stride=stride, split_k=split_k, tile=tile)
        if slope is not None:
            f.update(act=2, act_slope=slope.data_ptr())
        if residual is not None:
            f["residual"] = residual.data_ptr()
        o2 = None
        if out2 is not None:
            o2 = torch.empty_like(out)
            f.update(out2=o2.data_ptr(), out2_scale=out2[0].data_ptr(), out2_shift=out2[1].data_ptr())
        self._gemm([(t.data_ptr(), *rest) for t, *rest in srcs], w.data_ptr(), n, batch, oh, ow, **f)
        return out, o2

    def stem(self, x: torch.Tensor, u8: bool) -> Tuple[torch.Tensor, torch.Tensor]:
        """-> (x0, layer1.0.bn1(x0)) NHWC [B,112,112,64]"""
        B = x.shape[0]
        w = self.w
        out = torch.empty((B, SIZE, SIZE, 64), dtype=self.tdt, device=self.device)
        out2 = torch.empty_like(out)
        L.check(self.lib.idb_arcface_stem(x.data_ptr(), int(u8), B, SIZE, SIZE, w["stem.w"].data_ptr(), w["stem.b"].data_ptr(),
                                          w["stem.slope"].data_ptr(), w["stem.out2_scale"].data_ptr(), w["stem.out2_shift"].data_ptr(),
                                          out.data_ptr(), out2.data_ptr(), self.dt, self._stream()), "idb_arcface_stem")
        return out, out2

    def block(self, i: int, j: int, x: torch.Tensor, xb: torch.Tensor):
        """IBasicBlock layer{i+1}.{j} on NHWC x and its bn1(x) -> (out, next bn1(out) or None)."""
        w, k = self.w, f"layer{i + 1}.{j}"
        B, H, W_, cin = x.shape
        planes = PLANES[i]
        h, _ = self.gemm([(xb, cin, 9, H, W_)], w[f"{k}.conv1.w"], planes, B, H, W_, w[f"{k}.conv1.b"], slope=w[f"{k}.conv1.slope"])
        o2 = (w[f"{k}.out2_scale"], w[f"{k}.out2_shift"]) if f"{k}.out2_scale" in w else None
        if j == 0:
            oh, ow = (H + 1) // 2, (W_ + 1) // 2
            return self.gemm([(h, planes, 9, H, W_), (x, cin, 1, H, W_)], w[f"{k}.conv2.w"], planes, B, oh, ow, w[f"{k}.conv2.b"],
                             stride=2, out2=o2)
        return self.gemm([(h, planes, 9, H, W_)], w[f"{k}.conv2.w"], planes, B, H, W_, w[f"{k}.conv2.b"], residual=x, out2=o2)

    def stage(self, i: int, x: torch.Tensor, xb: torch.Tensor):
        for j in range(ARCHS[self.arch][i]):
            x, xb = self.block(i, j, x, xb)
        return x, xb

    def head(self, x: torch.Tensor) -> torch.Tensor:
        B = x.shape[0]
        k = x[0].numel()
        y = torch.empty((B, EMBED), dtype=torch.float32, device=self.device)
        need = self.lib.idb_arcface_head_workspace_bytes(B, EMBED, k)
        ws = self._workspace(need)
        L.check(self.lib.idb_arcface_head(x.data_ptr(), self.w["fc.w"].data_ptr(), self.w["fc.b"].data_ptr(), y.data_ptr(), B, EMBED, k,
                                          self.dt, ws.data_ptr(), need, self._stream()), "idb_arcface_head")
        return y

    def _forward(self, x: torch.Tensor, u8: bool) -> torch.Tensor:
        x, xb = self.stem(x, u8)
        for i in range(4):
            x, xb = self.stage(i, x, xb)
        return self.head(x)

    def _run(self, x: torch.Tensor, u8: bool) -> torch.Tensor:
        return self._chunked(x, lambda xc: (self._forward(xc, u8),))[0]

    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        """float [B,3,112,112] normalised as (x/255 - 0.5)/0.5 -> [B,512] fp32."""
        if not torch.is_tensor(x) or x.ndim != 4 or tuple(x.shape[1:]) != (3, SIZE, SIZE) or x.shape[0] < 1:
            raise ValueError(f"ArcFace expects [B,3,{SIZE},{SIZE}] input (the fc fixes 7x7), got {tuple(getattr(x, 'shape', ()))}")
        self._need_device()
        return self._run(x.to(self.device, dtype=torch.float32).contiguous(), False)

    def embed_u8(self, crops) -> torch.Tensor:
        """uint8 NHWC [B,112,112,3] aligned crops -> [B,512] fp32, the (x/255 - 0.5)/0.5 preprocessing on the GPU."""
        t = torch.as_tensor(np.asarray(crops)) if not torch.is_tensor(crops) else crops
        if t.dtype != torch.uint8 or t.ndim != 4 or tuple(t.shape[1:]) != (SIZE, SIZE, 3) or t.shape[0] < 1:
            raise ValueError(f"embed_u8 expects uint8 [B,{SIZE},{SIZE},3] crops, got {t.dtype} {tuple(t.shape)}")
        self._need_device()
        return self._run(t.to(self.device).contiguous(), True)

    def _features(self, x: torch.Tensor, u8: bool) -> torch.Tensor:
        x, xb = self.stem(x, u8)
        for i in range(4):
            x, xb = self.stage(i, x, xb)
        return x

    def features_map(self, x: torch.Tensor) -> torch.Tensor:
        """float [B,3,112,112] as __call__ takes it -> layer4's output, NHWC [B,7,7,512] in the operand dtype: what the embedding
        stage (frtail.EmbeddingStage) starts from.  The trunk is the folded eval network."""
        if not torch.is_tensor(x) or x.ndim != 4 or tuple(x.shape[1:]) != (3, SIZE, SIZE) or x.shape[0] < 1:
            raise ValueError(f"ArcFace expects [B,3,{SIZE},{SIZE}] input (the fc fixes 7x7), got {tuple(getattr(x, 'shape', ()))}")
        self._need_device()
        return self._chunked(x.to(self.device, dtype=torch.float32).contiguous(), lambda xc: (self._features(xc, False),))[0]

    def features_map_u8(self, crops) -> torch.Tensor:
        """uint8 NHWC [B,112,112,3] aligned crops -> NHWC [B,7,7,512], the preprocessing on the GPU."""
        t = torch.as_tensor(np.asarray(crops)) if not torch.is_tensor(crops) else crops
        if t.dtype != torch.uint8 or t.ndim != 4 or tuple(t.shape[1:]) != (SIZE, SIZE, 3) or t.shape[0] < 1:
            raise ValueError(f"features_map_u8 expects uint8 [B,{SIZE},{SIZE},3] crops, got {t.dtype} {tuple(t.shape)}")
        self._need_device()
        return self._chunked(t.to(self.device).contiguous(), lambda xc: (self._features(xc, True),))[0]


def embed_faces(images_u8, mtcnn, arcface: ArcFace):
    """detect(..., landmarks=True) -> norm_crop of the first (largest) face -> embed_u8, for a uint8 NHWC image batch.
    Returns (embeddings [B,512] fp32, has_face bool [B]); images without a face get a zero row and has_face False."""
    from .face_align import norm_crop
    t = images_u8 if torch.is_tensor(images_u8) else torch.from_numpy(np.ascontiguousarray(images_u8))
    if t.dtype != torch.uint8 or t.ndim != 4 or t.shape[-1] != 3:
        raise ValueError("embed_faces expects a uint8 image batch [B, H, W, 3]")
    _, _, lms = mtcnn.detect(t, landmarks=True)
    B = t.shape[0]
    has = np.array([lm is not None for lm in lms], dtype=bool)
    emb = torch.zeros((B, EMBED), dtype=torch.float32, device=arcface.device)
    if has.any():
        sel = np.nonzero(has)[0]
        imgs = t.to(arcface.device)[torch.from_numpy(sel).to(arcface.device)]
        crops = norm_crop(imgs, np.stack([lms[b][0] for b in sel]))          # the first (largest) face, as the reference takes
        emb[torch.from_numpy(sel).to(arcface.device)] = arcface.embed_u8(crops)
    return emb, torch.from_numpy(has)
