"""6DRepNet head pose (pitch, yaw, roll) of generated faces — the measurement of the reference's
Evaluation/PoseEstimation/estimate_head_pose_ID-Booth.ipynb, which runs ``sixdrepnet.SixDRepNet().predict(img)`` on every image
(read with cv2, a 30-pixel black border added by ``copyMakeBorder``) and reports the pitch / yaw / roll lists, overall and per
identity (``pose_summary``).

The ``sixdrepnet`` package is not part of this project.  What follows restates its ``SixDRepNet_Detector`` from memory of its source;
only what the notebook itself shows (the 30-pixel border, ``predict`` on the whole padded image, the JSON schema) is verified.  Key
names, the transform and the head math below are UNVERIFIED restatements:
  * transform: RGB, torchvision ``Resize(224)`` on a PIL image (= ``Image.resize((224, 224), BILINEAR)`` with Pillow's antialiasing
    for square input), ``CenterCrop(224)`` (a no-op), ``ToTensor``, ``Normalize(ImageNet mean / std)``; no face detector;
  * network: RepVGG-B1g2 in deploy form — every block one ``Conv2d(3x3, padding 1, bias)`` + ReLU; ``layer0`` 3->64 stride 2, then
    ``layer1``..``layer4`` with widths 128 / 256 / 512 / 2048 and 4 / 6 / 16 / 1 blocks (first of each stage stride 2); blocks 2, 4,
    ..., 26 (counted from 1 after layer0) have groups = 2; ``AdaptiveAvgPool2d(1)``, ``linear_reg`` 2048 -> 6;
  * head: the 6D output -> rotation matrix by Gram-Schmidt (columns x, y, z) -> Euler angles in degrees.
Trained weights (6DRepNet_300W_LP_AFLW2000.pth) are not shipped: PARITY WITH THE TRAINED NETWORK IS UNPINNED.  The HIP path is
checked against tests/headpose_oracle.py, an independent fp32 restatement, with seeded synthetic weights.

Engine (every layer a HIP kernel of libidb_kernels.so):
  * idb_resize_aa_u8: zero border + Pillow-exact antialiased bilinear resize of the uint8 images
  * idb_pose_stem: ToTensor + Normalize fused into layer0 (3->64, stride 2) + ReLU (VALU)
  * layer1..layer4: one idb_gemm per block with act = 3 (ReLU in the epilogue, or in the reduce launch of a split-K plan).  A grouped
    block (groups G = 2) is G idb_gemm calls, one per group, each reading its own input tensor and writing its output channels at
    column offset g n / G of one full tensor (out_ld = n); the dense block in front of it therefore writes its output as G separate
    tensors of n / G channels (G calls on the row slices of its weight).  No block-diagonal weights: the MFMA work is the grouped one.
  * idb_pose_head: average pool, linear_reg, Gram-Schmidt and Euler angles in fp32.
"""
from __future__ import annotations

from collections import OrderedDict
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _hipnet as N
from . import _lib as L

SD = Dict[str, torch.Tensor]

SIZE = 224
PAD = 30
EPS = 1e-5
MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
WIDTHS = [128, 256, 512, 2048]
DEPTHS = [4, 6, 16, 1]
GROUPED = set(range(2, 27, 2))          # block indices (from 1 after layer0) with groups = 2
GROUPS = 2
_BN = ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")


def blocks() -> List[Tuple[str, int, int, int, int]]:
    """(module key, cin, cout, stride, groups) of the 28 convs, layer0 first."""
    out = [("layer0", 3, 64, 2, 1)]
    cin, idx = 64, 1
    for s, (w, nb) in enumerate(zip(WIDTHS, DEPTHS)):
        for j in range(nb):
            out.append((f"layer{s + 1}.{j}", cin, w, 2 if j == 0 else 1, GROUPS if idx in GROUPED else 1))
            cin, idx = w, idx + 1
    return out


def gflops(size: int = SIZE) -> float:
    """Multiply-adds x 2 of one image (convs + linear_reg), in GFLOP."""
    total, h = 0, size
    for _, cin, cout, stride, g in blocks():
        h = (h + stride - 1) // stride
        total += 2 * h * h * cout * (cin // g) * 9
    return (total + 2 * 2048 * 6) / 1e9


def param_shapes(deploy: bool = True) -> "OrderedDict[str, Tuple[int, ...]]":
    """State-dict layout of SixDRepNet: deploy form (``rbr_reparam``) or training form (``rbr_dense`` / ``rbr_1x1`` / ``rbr_identity``
    with BatchNorms; num_batches_tracked is a 0-d buffer)."""
    out: "OrderedDict[str, Tuple[int, ...]]" = OrderedDict()

    def bn(key, c):
        for f in _BN:
            out[f"{key}.{f}"] = () if f == "num_batches_tracked" else (c,)

    for key, cin, cout, stride, g in blocks():
        if deploy:
            out[f"{key}.rbr_reparam.weight"] = (cout, cin // g, 3, 3)
            out[f"{key}.rbr_reparam.bias"] = (cout,)
            continue
        if cin == cout and stride == 1:
            bn(f"{key}.rbr_identity", cin)
        out[f"{key}.rbr_dense.conv.weight"] = (cout, cin // g, 3, 3)
        bn(f"{key}.rbr_dense.bn", cout)
        out[f"{key}.rbr_1x1.conv.weight"] = (cout, cin // g, 1, 1)
        bn(f"{key}.rbr_1x1.bn", cout)
    out["linear_reg.weight"] = (6, 2048)
    out["linear_reg.bias"] = (6,)
    return out


def synth_weights(seed: int = 0, deploy: bool = True) -> SD:
    """Seeded synthetic weights.  Convs are He-scaled (std sqrt(2 / fan_in)) with small biases, so the activations keep their scale
    over 28 ReLU layers; training-form BatchNorms are near identity (gammas 0.4-0.7 per branch, running variances 0.5-2).
    ``linear_reg`` is scaled so that the 6D outputs, and with them the angles, spread over tens of degrees."""
    g = torch.Generator().manual_seed(seed)
    sd: SD = {}
    for name, shp in param_shapes(deploy).items():
        if name.endswith("num_batches_tracked"):
            sd[name] = torch.tensor(0, dtype=torch.int64)
        elif name.endswith("running_var"):
            sd[name] = 0.5 + 1.5 * torch.rand(shp, generator=g)
        elif name.endswith("running_mean"):
            sd[name] = 0.1 * torch.randn(shp, generator=g)
        elif name == "linear_reg.weight":
            sd[name] = torch.randn(shp, generator=g) * (1.0 / shp[1]) ** 0.5
        elif name == "linear_reg.bias":
            sd[name] = torch.tensor([1.0, 0.0, 0.0, 0.0, 1.0, 0.0]) + 0.3 * torch.randn(shp, generator=g)
        elif len(shp) == 4:
            fan = int(np.prod(shp[1:]))
            scale = (2.0 / fan) ** 0.5 * (1.0 if deploy or shp[-1] == 3 else 0.5)
            sd[name] = torch.randn(shp, generator=g) * scale
        elif name.endswith(".weight"):                                  # BN gammas (3 branches add up)
            sd[name] = 0.4 + 0.3 * torch.rand(shp, generator=g)
        else:                                                           # conv / BN biases
            sd[name] = 0.05 * torch.randn(shp, generator=g)
    return sd


def _normalize_keys(sd: SD) -> SD:
    """Unwrap ``model_state_dict`` and strip a ``module.`` prefix (DataParallel checkpoints)."""
    if "model_state_dict" in sd and isinstance(sd["model_state_dict"], dict):
        sd = sd["model_state_dict"]
    return {(k[7:] if k.startswith("module.") else k): v for k, v in sd.items()}


def is_deploy(sd: SD) -> bool:
    return any(k.endswith("rbr_reparam.weight") for k in sd)


def check_state_dict(sd: SD) -> None:
    """Strict keys and shapes of the deploy or training form (chosen by the keys present): missing / unexpected / wrong-shaped keys
    raise ValueError naming them; num_batches_tracked is accepted and ignored."""
    sd = _normalize_keys(sd)
    deploy = is_deploy(sd)
    N.check_state_dict(sd, param_shapes(deploy), f"6DRepNet ({'deploy' if deploy else 'training'} form)")


def _fuse_bn(w: torch.Tensor, sd: SD, key: str) -> Tuple[torch.Tensor, torch.Tensor]:
    t, b = N.bn_affine(sd, key, EPS)
    return w * t[:, None, None, None], b


def reparam_block(sd: SD, key: str, cin: int, cout: int, groups: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """RepVGGBlock.get_equivalent_kernel_bias in float64: dense 3x3 + BN, 1x1 + BN padded to the centre tap, identity BN."""
    k, b = _fuse_bn(sd[f"{key}.rbr_dense.conv.weight"].double(), sd, f"{key}.rbr_dense.bn")
    k1, b1 = _fuse_bn(sd[f"{key}.rbr_1x1.conv.weight"].double(), sd, f"{key}.rbr_1x1.bn")
    k = k.clone()
    k[:, :, 1:2, 1:2] += k1
    b = b + b1
    if f"{key}.rbr_identity.weight" in sd:
        cpg = cin // groups
        idk = torch.zeros((cout, cpg, 3, 3), dtype=torch.float64)
        idk[torch.arange(cout), torch.arange(cout) % cpg, 1, 1] = 1.0
        ki, bi = _fuse_bn(idk, sd, f"{key}.rbr_identity")
        k, b = k + ki, b + bi
    return k, b


def deploy_state_dict(sd: SD) -> SD:
    """Any accepted state dict -> the deploy form in float64 (training-form blocks folded on the CPU)."""
    check_state_dict(sd)
    sd = _normalize_keys(sd)
    if is_deploy(sd):
        return {k: v.double() for k, v in sd.items() if not k.endswith("num_batches_tracked")}
    out: SD = {}
    for key, cin, cout, _, g in blocks():
        out[f"{key}.rbr_reparam.weight"], out[f"{key}.rbr_reparam.bias"] = reparam_block(sd, key, cin, cout, g)
    out["linear_reg.weight"] = sd["linear_reg.weight"].double()
    out["linear_reg.bias"] = sd["linear_reg.bias"].double()
    return out


_pack = N.pack_conv


def fold_weights(sd: SD) -> Dict[str, torch.Tensor]:
    """The fp32 tensors the engine uploads (CPU).  Keys: ``{module}.w`` (layer0: [64][27] as [cout][ky][kx][cin]; blocks: idb_gemm's
    [n][9 cin/groups]) and ``{module}.b``, ``linear_reg.w`` [6][2048], ``linear_reg.b`` [6].  The engine rounds the block weights to
    the operand dtype."""
    d = deploy_state_dict(sd)
    f: Dict[str, torch.Tensor] = {}
    for key, *_ in blocks():
        f[f"{key}.w"] = _pack(d[f"{key}.rbr_reparam.weight"])
        f[f"{key}.b"] = d[f"{key}.rbr_reparam.bias"]
    f["linear_reg.w"] = d["linear_reg.weight"]
    f["linear_reg.b"] = d["linear_reg.bias"]
    return {k: v.float().contiguous() for k, v in f.items()}


def pose_summary(names: Sequence[str], pitch, yaw, roll) -> dict:
    """The notebook's JSON record: ``yaw`` / ``pitch`` / ``roll`` lists in image order and ``*_per_id`` dicts of lists keyed by
    ``name.split("_")[0]`` (host-side)."""
    p, y, r = (np.asarray(torch.as_tensor(v).detach().cpu(), dtype=np.float64).reshape(-1) for v in (pitch, yaw, roll))
    if not (len(names) == len(p) == len(y) == len(r)):
        raise ValueError("pose_summary: names, pitch, yaw and roll must have the same length")
    res = {"yaw": [], "yaw_per_id": {}, "pitch": [], "pitch_per_id": {}, "roll": [], "roll_per_id": {}}
    for name, pv, yv, rv in zip(names, p, y, r):
        tid = name.split("_")[0]
        for k, v in (("yaw", yv), ("pitch", pv), ("roll", rv)):
            res[k].append(float(v))
            res[f"{k}_per_id"].setdefault(tid, []).append(float(v))
    return res


class HeadPose(N.HipNet):
    """Drop-in for SixDRepNet: ``model(x)`` maps normalised fp32 [B,3,224,224] to rotation matrices [B,3,3] (``SixDRepNet.forward``);
    ``predict_u8(images, pad=30)`` maps uint8 RGB [B,S,S,3] images to (pitch, yaw, roll) fp32 degree tensors [B] — the notebook's
    ``model.predict`` on the image with its 30-pixel border.  ``HeadPose.from_pretrained(path)`` loads a local ``.pth`` (deploy or
    training form); nothing is ever downloaded.  Batches of any size >= 1 run in chunks of ``chunk`` images."""

    NAME = "HeadPose"

    def __init__(self, sd: SD, torch_dtype: torch.dtype = torch.float16, chunk: int = 256):
        super().__init__(torch_dtype, chunk)
        self._fw = fold_weights({k: v.detach().cpu() for k, v in _normalize_keys(sd).items()})

    @classmethod
    def from_state_dict(cls, sd: SD, torch_dtype: torch.dtype = torch.float16) -> "HeadPose":
        return cls(sd, torch_dtype)

    @classmethod
    def from_pretrained(cls, path: str, torch_dtype: torch.dtype = torch.float16) -> "HeadPose":
        return cls(torch.load(path, weights_only=True, map_location="cpu"), torch_dtype)

    @classmethod
    def from_synthetic(cls, seed: int = 0, torch_dtype: torch.dtype = torch.float16, deploy: bool = True) -> "HeadPose":
        return cls(synth_weights(seed, deploy), torch_dtype)

    # ---- device side ----------------------------------------------------------------------------------------------------------
    def _operand(self, key: str) -> bool:
        return key.endswith(".w") and key.startswith("layer") and key != "layer0.w"

    def gemm(self, src: int, cin: int, h: int, w_: int, batch: int, weight: int, bias: int, n: int, out: int, out_ld: int, stride: int = 1,
             act: int = 3, split_k: int = 0, tile: int = 0) -> None:
        """One 3x3 pad-1 idb_gemm on raw device pointers: src NHWC [batch][h][w_][cin] -> out rows of out_ld elements."""
        oh, ow = (h + stride - 1) // stride, (w_ + stride - 1) // stride
        self._gemm([(src, cin, 9, h, w_)], weight, n, batch, oh, ow, stride=stride, bias=bias, out=out, out_ld=out_ld, act=act,
                   split_k=split_k, tile=tile)

    def block(self, i: int, x, split_out: bool):
        """Block i (1..27) of blocks().  x: a full NHWC tensor [B,H,W,cin] (dense block) or [G,B,H,W,cin/G] (grouped block).
        Returns [B,H',W',n], or [G,B,H',W',n/G] when split_out (the next block is grouped)."""
        key, cin, n, stride, g = blocks()[i]
        wt, bt = self.w[f"{key}.w"], self.w[f"{key}.b"]
        if g > 1:
            _, B, H, W_, _ = x.shape
        else:
            B, H, W_, _ = x.shape
        oh, ow = (H + stride - 1) // stride, (W_ + stride - 1) // stride
        es = wt.element_size()
        if g > 1:                                  # one call per group: own input tensor, weight rows, output column slice
            out = torch.empty((B, oh, ow, n), dtype=self.tdt, device=self.device)
            ng, K = n // g, wt.shape[1]
            for q in range(g):
                self.gemm(x[q].data_ptr(), cin // g, H, W_, B, wt.data_ptr() + q * ng * K * es, bt.data_ptr() + q * ng * 4, ng,
                          out.data_ptr() + q * ng * es, n, stride)
            return out
        if split_out:                              # the next block is grouped: its G inputs as separate tensors
            out = torch.empty((GROUPS, B, oh, ow, n // GROUPS), dtype=self.tdt, device=self.device)
            ng, K = n // GROUPS, wt.shape[1]
            for q in range(GROUPS):
                self.gemm(x.data_ptr(), cin, H, W_, B, wt.data_ptr() + q * ng * K * es, bt.data_ptr() + q * ng * 4, ng, out[q].data_ptr(),
                          ng, stride)
            return out
        out = torch.empty((B, oh, ow, n), dtype=self.tdt, device=self.device)
        self.gemm(x.data_ptr(), cin, H, W_, B, wt.data_ptr(), bt.data_ptr(), n, out.data_ptr(), n, stride)
        return out

    def stem(self, x: torch.Tensor, u8: bool) -> torch.Tensor:
        x = x.contiguous()
        B, h, w_ = (x.shape[0], x.shape[1], x.shape[2]) if u8 else (x.shape[0], x.shape[2], x.shape[3])
        out = torch.empty((B, (h + 1) // 2, (w_ + 1) // 2, 64), dtype=self.tdt, device=self.device)
        L.check(self.lib.idb_pose_stem(x.data_ptr(), int(u8), B, h, w_, self.w["layer0.w"].data_ptr(), self.w["layer0.b"].data_ptr(),
                                       out.data_ptr(), self.dt, self._stream()), "idb_pose_stem")
        return out

    def head(self, x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """[B,H,W,2048] -> (R [B,3,3], angles [B,3] pitch / yaw / roll in degrees)."""
        x = x.contiguous()
        B = x.shape[0]
        R = torch.empty((B, 3, 3), dtype=torch.float32, device=self.device)
        ang = torch.empty((B, 3), dtype=torch.float32, device=self.device)
        L.check(self.lib.idb_pose_head(x.data_ptr(), B, x.shape[1] * x.shape[2], x.shape[3], self.w["linear_reg.w"].data_ptr(),
                                       self.w["linear_reg.b"].data_ptr(), R.data_ptr(), ang.data_ptr(), self.dt, self._stream()),
                "idb_pose_head")
        return R, ang

    def resize(self, images: torch.Tensor, pad: int) -> torch.Tensor:
        """uint8 [B,S,S,3] -> zero border of pad -> Pillow bilinear resize to [B,224,224,3] uint8."""
        images = images.contiguous()
        B, S = images.shape[0], images.shape[1]
        out = torch.empty((B, SIZE, SIZE, 3), dtype=torch.uint8, device=self.device)
        L.check(self.lib.idb_resize_aa_u8(images.data_ptr(), B, S, pad, SIZE, out.data_ptr(), self._stream()), "idb_resize_aa_u8")
        return out

    def features(self, x: torch.Tensor, u8: bool, stages_out: Optional[List[torch.Tensor]] = None) -> torch.Tensor:
        """Stem and the 27 blocks -> [B,7,7,2048].  stages_out, if given, receives the stem output and each stage's output (NHWC)."""
        x = self.stem(x, u8)
        if stages_out is not None:
            stages_out.append(x)
        bl = blocks()
        for i in range(1, len(bl)):
            nxt = i + 1 < len(bl) and bl[i + 1][4] > 1
            x = self.block(i, x, nxt)
            if stages_out is not None and (i + 1 == len(bl) or bl[i + 1][0].endswith(".0")):
                stages_out.append(x)
        return x

    def _run(self, x: torch.Tensor, u8: bool, pad: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
        return self._chunked(x, lambda xc: self.head(self.features(self.resize(xc, pad) if u8 else xc, u8)))

    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        """float [B,3,224,224] normalised with the ImageNet mean / std -> rotation matrices [B,3,3] fp32."""
        if not torch.is_tensor(x) or x.ndim != 4 or tuple(x.shape[1:]) != (3, SIZE, SIZE) or x.shape[0] < 1:
            raise ValueError(f"HeadPose expects [B,3,{SIZE},{SIZE}] input, got {tuple(getattr(x, 'shape', ()))}")
        self._need_device()
        return self._run(x.to(self.device, dtype=torch.float32).contiguous(), False)[0]

    def predict_u8(self, images, pad: int = PAD) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """uint8 RGB [B,S,S,3] -> (pitch, yaw, roll) fp32 tensors [B] in degrees, on the padded image as the notebook does."""
        t = torch.as_tensor(np.asarray(images)) if not torch.is_tensor(images) else images
        if t.dtype != torch.uint8 or t.ndim != 4 or t.shape[-1] != 3 or t.shape[0] < 1:
            raise ValueError(f"predict_u8 expects uint8 [B,S,S,3] images, got {t.dtype} {tuple(t.shape)}")
        if t.shape[1] != t.shape[2]:
            raise ValueError(f"predict_u8 expects square images, got {t.shape[1]}x{t.shape[2]}")
        if pad < 0:
            raise ValueError("pad must be >= 0")
        self._need_device()
        _, a = self._run(t.to(self.device).contiguous(), True, int(pad))
        return a[:, 0], a[:, 1], a[:, 2]
