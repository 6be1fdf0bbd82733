"""The embedding stage of the reference's face-recognition backbone in training, forward and backward: the last lines of
``IResNet.forward`` (``FR_training/backbones/iresnet.py``: ``bn2`` -> ``flatten(1)`` -> ``Dropout(p=0.4)`` -> ``fc`` -> ``features``)
and the loop's ``F.normalize`` (``train_FR.py:279``), with batch statistics, dropout and the running statistics, then what
``accelerator.backward`` leaves in the stage's five trainable tensors, ``clip_grad_norm_(model.parameters(), 5)`` and
``opt_backbone.step()`` (SGD, momentum 0.9, weight decay 5e-4).  ``csrc/idb_tail.hip``: fp32 state, the three products on the exact
f32-input MFMA, statistics in double, bit-identical from run to run.

The regime.  Upstream never freezes the trunk.  What is reproduced here is upstream's loop with the convolutional trunk's parameters
at ``requires_grad=False`` and the trunk in ``eval()`` (the folded network of ``arcface.py``): ``clip_grad_norm_`` skips parameters
without ``.grad``, so it sees exactly this stage's five trainable tensors (``bn2.weight``, ``bn2.bias``, ``fc.weight``, ``fc.bias``,
``features.bias``; ``features.weight`` is frozen upstream), and weight decay applies to all five (upstream's single param group).
The gradient with respect to the trunk's output is handed out (``StageGrad.input``) for whatever trains the trunk.

Layout.  ``feature_map`` is NHWC ``[B, 7, 7, ch]`` as ``ArcFace.features_map`` returns it.  ``fc.weight`` lives on the device as
``[n][hw * ch]`` with column ``p * ch + c`` (``fold_weights``' order); ``state_dict`` / ``fc_weight_upstream`` convert to upstream's
``c * hw + p``.  ``keep`` is given in upstream's flatten order and converted once.

Dropout: without ``keep`` the mask is drawn on the device with ``bernoulli_(1 - p)``: upstream's distribution, NOT upstream's random
stream (torch's dropout kernel consumes its Philox stream differently; nothing here reproduces it).

Refused, each with a message that names the reason: a batch of one in training mode (upstream's BatchNorm1d raises), a feature map or
keep-mask of the wrong shape or dtype, non-finite input (found on the device, by the statistics launch in training mode and by the
per-row launch in eval mode: the call raises after it, and the running statistics and batch counters are left as they were), a channel
or feature whose batch variance is exactly 0 together with eps = 0, SE or bottleneck checkpoints, CPU devices (there is no CPU
fallback), a trunk in training mode, and ``auto_schedule``'s ``ReduceLROnPlateau`` in ``learning_rate``.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._frtrain import ClippedSGD, hip_device
from .frhead import HeadGrad, HeadLoss, HeaderSGD, MarginHeader

STAGE_KEYS = ("bn2.weight", "bn2.bias", "bn2.running_mean", "bn2.running_var", "bn2.num_batches_tracked", "fc.weight", "fc.bias",
              "features.weight", "features.bias", "features.running_mean", "features.running_var", "features.num_batches_tracked")
TRAINABLE = ("bn2.weight", "bn2.bias", "fc.weight", "fc.bias", "features.bias")      # model.parameters() order, features.weight frozen
_DT = {torch.float16: _lib.IDB_F16, torch.bfloat16: _lib.IDB_BF16, torch.float32: _lib.IDB_F32}
MAX_B = 1024


class StageOut:
    """embeddings: the unit rows, fp32 [B, n]; norms: |features(...)| per row before F.normalize, float64 [B]; the saved context of
    the backward (_ctx) is private."""
    __slots__ = ("embeddings", "norms", "_ctx")

    def __init__(self, embeddings: torch.Tensor, norms: torch.Tensor, ctx: dict):
        self.embeddings, self.norms, self._ctx = embeddings, norms, ctx


class StageGrad(NamedTuple):
    """Gradients of the five trainable tensors (fc_weight in device order [n][hw * ch], column p * ch + c) and `input`, the gradient
    with respect to the feature map, fp32 NHWC (None with need_input_grad=False); hw, ch: the stage's geometry."""
    bn2_weight: torch.Tensor
    bn2_bias: torch.Tensor
    fc_weight: torch.Tensor
    fc_bias: torch.Tensor
    features_bias: torch.Tensor
    input: Optional[torch.Tensor]
    hw: int
    ch: int

    def fc_weight_upstream(self) -> torch.Tensor:
        """fc.weight.grad as upstream stores it: [n, ch * hw], column c * hw + p."""
        n = self.fc_weight.shape[0]
        return self.fc_weight.view(n, self.hw, self.ch).permute(0, 2, 1).reshape(n, self.ch * self.hw).contiguous()


def to_device_order(w: torch.Tensor, ch: int, hw: int) -> torch.Tensor:
    """[..., ch * hw] in upstream's flatten order (c * hw + p) -> [..., hw * ch] in NHWC order (p * ch + c)."""
    lead = w.shape[:-1]
    return w.reshape(*lead, ch, hw).transpose(-1, -2).reshape(*lead, hw * ch).contiguous()


def to_upstream_order(w: torch.Tensor, ch: int, hw: int) -> torch.Tensor:
    lead = w.shape[:-1]
    return w.reshape(*lead, hw, ch).transpose(-1, -2).reshape(*lead, ch * hw).contiguous()


class EmbeddingStage:
    """bn2, dropout, fc, features of an IResNet (plain IBasicBlock networks; eps 1e-5, momentum 0.1 as upstream builds them)."""

    def __init__(self, sd: Dict[str, torch.Tensor], dropout: float = 0.4, eps: float = 1e-5, momentum: float = 0.1):
        missing = [k for k in STAGE_KEYS if k not in sd and not k.endswith("num_batches_tracked")]
        if missing:
            raise ValueError(f"EmbeddingStage: the state dict lacks {missing}")
        se = [k for k in sd if ".se." in k or k.endswith("conv3.weight")]
        if se:
            raise NotImplementedError(f"EmbeddingStage: an SE or bottleneck checkpoint ({se[0]}): only plain IBasicBlock networks are built")
        w = sd["fc.weight"]
        if w.ndim != 2 or sd["bn2.weight"].ndim != 1 or w.shape[1] % sd["bn2.weight"].shape[0] != 0:
            raise ValueError(f"EmbeddingStage: fc.weight {tuple(w.shape)} does not fit bn2 of {tuple(sd['bn2.weight'].shape)} channels")
        self.n, self.ch = int(w.shape[0]), int(sd["bn2.weight"].shape[0])
        self.hw = int(w.shape[1]) // self.ch
        if _lib_shapes_refused(2, self.ch, self.hw, self.n):
            raise ValueError(f"EmbeddingStage: ch {self.ch} (% 64 == 0, <= 2048), hw {self.hw} (1..64), n {self.n} (% 64 == 0, <= 1024)")
        for k, size in (("bn2.weight", self.ch), ("bn2.bias", self.ch), ("bn2.running_mean", self.ch), ("bn2.running_var", self.ch),
                        ("fc.bias", self.n), ("features.weight", self.n), ("features.bias", self.n), ("features.running_mean", self.n),
                        ("features.running_var", self.n)):
            if tuple(sd[k].shape) != (size,):
                raise ValueError(f"EmbeddingStage: {k} expected ({size},), got {tuple(sd[k].shape)}")
        self.p, self.eps, self.momentum = float(dropout), float(eps), float(momentum)
        if not 0.0 <= self.p < 1.0:
            raise ValueError("EmbeddingStage: dropout in [0, 1)")
        if not (0.0 <= self.eps <= 1.0 and 0.0 <= self.momentum <= 1.0):
            raise ValueError("EmbeddingStage: eps in [0, 1], momentum in [0, 1]")
        f32 = lambda k: sd[k].detach().to("cpu", torch.float32).contiguous().clone()      # noqa: E731
        self.t: Dict[str, torch.Tensor] = {k: f32(k) for k in STAGE_KEYS if not k.endswith("num_batches_tracked") and k != "fc.weight"}
        self.t["fc.weight"] = to_device_order(f32("fc.weight"), self.ch, self.hw)
        self.tracked = {k: int(sd[f"{k}.num_batches_tracked"]) if f"{k}.num_batches_tracked" in sd else 0 for k in ("bn2", "features")}
        self.training = True
        self.device: Optional[torch.device] = None

    # ---- construction ---------------------------------------------------------------------------------------------------------
    @classmethod
    def from_state_dict(cls, sd, dropout: float = 0.4, **kw) -> "EmbeddingStage":
        """`sd`: a backbone state dict; only the stage's 12 keys are read."""
        return cls(sd, dropout, **kw)

    @classmethod
    def from_pretrained(cls, path: str, dropout: float = 0.4, **kw) -> "EmbeddingStage":
        """`path`: a <step>_backbone.pth as CallBackModelCheckpointOld writes it."""
        return cls(torch.load(path, weights_only=True, map_location="cpu"), dropout, **kw)

    @classmethod
    def from_backbone(cls, arcface, dropout: float = 0.4, **kw) -> "EmbeddingStage":
        return cls(arcface._sd, dropout, **kw)

    @classmethod
    def from_synthetic(cls, seed: int, ch: int = 512, hw: int = 49, n: int = 512, dropout: float = 0.4, **kw) -> "EmbeddingStage":
        g = torch.Generator().manual_seed(seed)
        sd = {"bn2.weight": 0.8 + 0.4 * torch.rand(ch, generator=g), "bn2.bias": 0.2 * torch.randn(ch, generator=g),
              "bn2.running_mean": 0.2 * torch.randn(ch, generator=g), "bn2.running_var": 0.5 + 1.5 * torch.rand(ch, generator=g),
              "fc.weight": torch.randn(n, ch * hw, generator=g) * (1.0 / (ch * hw)) ** 0.5, "fc.bias": 0.1 * torch.randn(n, generator=g),
              "features.weight": torch.ones(n), "features.bias": 0.1 * torch.randn(n, generator=g),
              "features.running_mean": 0.2 * torch.randn(n, generator=g), "features.running_var": 0.5 + 1.5 * torch.rand(n, generator=g)}
        return cls(sd, dropout, **kw)

    def to(self, device) -> "EmbeddingStage":
        dev = hip_device(device, "EmbeddingStage")
        _lib.load()
        self.t = {k: v.to(dev).contiguous() for k, v in self.t.items()}
        self.device = dev
        return self

    def train(self, mode: bool = True) -> "EmbeddingStage":
        self.training = bool(mode)
        return self

    def eval(self) -> "EmbeddingStage":
        return self.train(False)

    def state_dict(self) -> Dict[str, torch.Tensor]:
        """Upstream's key names and layouts (fc.weight [n, ch * hw], column c * hw + p), on the host."""
        sd = {k: v.detach().cpu().clone() for k, v in self.t.items() if k != "fc.weight"}
        sd["fc.weight"] = to_upstream_order(self.t["fc.weight"].detach().cpu(), self.ch, self.hw)
        for k in ("bn2", "features"):
            sd[f"{k}.num_batches_tracked"] = torch.tensor(self.tracked[k], dtype=torch.int64)
        return {k: sd[k] for k in STAGE_KEYS}

    def merged_into(self, backbone_sd) -> Dict[str, torch.Tensor]:
        """A full backbone state dict with this stage's tensors replaced (for ArcFace.from_state_dict / frbench)."""
        mine = self.state_dict()
        missing = [k for k in mine if k not in backbone_sd and not k.endswith("num_batches_tracked")]
        if missing:
            raise ValueError(f"merged_into: the backbone state dict lacks {missing}")
        out = {k: v.detach().cpu().clone() for k, v in backbone_sd.items()}
        for k, v in mine.items():
            if k in out and tuple(out[k].shape) != tuple(v.shape):
                raise ValueError(f"merged_into: {k} is {tuple(out[k].shape)} in the backbone, {tuple(v.shape)} here")
            if k in out or not k.endswith("num_batches_tracked"):
                out[k] = v
        return out

    def plan(self, batch: int):
        """(k_slices, row_tiles) of the fc forward for a batch: idb_tail_workspace_bytes' geometry."""
        ks, rt = C.c_int32(0), C.c_int32(0)
        if _lib.load().idb_tail_workspace_bytes(int(batch), self.ch, self.hw, self.n, C.byref(ks), C.byref(rt)) == 0:
            raise ValueError(f"batch {batch}: expected 1..{MAX_B}")
        return ks.value, rt.value

    # ---- calls ----------------------------------------------------------------------------------------------------------------
    def _desc(self, x: torch.Tensor, keep: Optional[torch.Tensor], training: bool) -> _lib.TailDesc:
        d, t = _lib.TailDesc(), self.t
        d.b, d.ch, d.hw, d.n = int(x.shape[0]), self.ch, self.hw, self.n
        d.x_dtype, d.training, d.p, d.eps2, d.eps1, d.momentum = _DT[x.dtype], int(training), self.p, self.eps, self.eps, self.momentum
        d.x, d.keep = x.data_ptr(), (keep.data_ptr() if keep is not None else None)
        d.bn2_weight, d.bn2_bias, d.bn2_mean, d.bn2_var = (t[f"bn2.{k}"].data_ptr() for k in ("weight", "bias", "running_mean", "running_var"))
        d.fc_weight, d.fc_bias = t["fc.weight"].data_ptr(), t["fc.bias"].data_ptr()
        d.feat_weight, d.feat_bias, d.feat_mean, d.feat_var = (t[f"features.{k}"].data_ptr()
                                                               for k in ("weight", "bias", "running_mean", "running_var"))
        return d

    def __call__(self, feature_map: torch.Tensor, keep=None, generator: Optional[torch.Generator] = None) -> StageOut:
        if self.device is None:
            raise _lib.IdbError("EmbeddingStage is not on a device: call .to('cuda:0') first (there is no CPU fallback)")
        x = feature_map
        if not torch.is_tensor(x) or x.dtype not in _DT:
            raise ValueError(f"feature_map: expected a float16, bfloat16 or float32 tensor, got {getattr(x, 'dtype', type(x))}")
        if not ((x.ndim == 4 and x.shape[1] * x.shape[2] == self.hw and x.shape[3] == self.ch) or
                (x.ndim == 3 and tuple(x.shape[1:]) == (self.hw, self.ch))) or x.shape[0] < 1:
            raise ValueError(f"feature_map: expected NHWC [B, h, w, {self.ch}] with h * w = {self.hw}, got {tuple(x.shape)}")
        b = int(x.shape[0])
        if b > MAX_B:
            raise ValueError(f"batch {b}: expected 1..{MAX_B}")
        if self.training and b < 2:
            raise ValueError("a batch of one in training mode: upstream's BatchNorm1d raises (there is no batch variance)")
        dev, K = self.device, self.hw * self.ch
        k = None
        if keep is not None:
            if not self.training:
                raise ValueError("keep: a dropout mask in eval mode")
            k = keep if torch.is_tensor(keep) else torch.from_numpy(np.ascontiguousarray(keep))
            if k.dtype not in (torch.bool, torch.uint8) or tuple(k.shape) != (b, K):
                raise ValueError(f"keep: expected bool or uint8 [{b}, {K}] in upstream's flatten order (c * hw + p), got {k.dtype} "
                                 f"{tuple(k.shape)}")
        if x.device != self.device:
            raise ValueError(f"feature_map: on {x.device}, the stage is on {self.device} (there is no CPU fallback)")
        x = x.contiguous()
        mask = None
        if k is not None:
            mask = to_device_order((k != 0).to(device=dev, dtype=torch.uint8), self.ch, self.hw)
        elif self.training and self.p > 0.0:
            mask = torch.empty((b, K), dtype=torch.uint8, device=dev).bernoulli_(1.0 - self.p, generator=generator)
        lib = _lib.load()
        d = self._desc(x, mask, self.training)
        need = lib.idb_tail_workspace_bytes(b, self.ch, self.hw, self.n, None, None)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        f64 = dict(dtype=torch.float64, device=dev)
        f32 = dict(dtype=torch.float32, device=dev)
        ctx = dict(x=x, keep=mask, b=b, emb=torch.empty((b, self.n), **f32), norms=torch.empty(b, **f64),
                   bn2_stat=torch.empty((2, self.ch), **f64), affine=torch.empty((2, self.ch), **f32), z=torch.empty((b, self.n), **f32),
                   feat_stat=torch.empty((2, self.n), **f64), f=torch.empty((b, self.n), **f32), training=self.training, stage=self)
        flags = torch.zeros(4, dtype=torch.int32, device=dev)
        running = ("bn2.running_mean", "bn2.running_var", "features.running_mean", "features.running_var")
        saved = {key: self.t[key].clone() for key in running} if self.training else {}      # put back if the call is refused
        _lib.check(lib.idb_tail_forward(C.byref(d), ctx["emb"].data_ptr(), ctx["norms"].data_ptr(), ctx["bn2_stat"].data_ptr(),
                                        ctx["affine"].data_ptr(), ctx["z"].data_ptr(), ctx["feat_stat"].data_ptr(), ctx["f"].data_ptr(),
                                        flags.data_ptr(), ws.data_ptr(), need, torch.cuda.current_stream(dev).cuda_stream), "idb_tail_forward")
        fl = flags.cpu().tolist()
        if any(fl[:3]):
            for key, v in saved.items():                       # a refused call leaves the stage as it was
                self.t[key].copy_(v)
        if fl[1]:                                              # checked first: its infinite invstd makes everything after it NaN
            raise ValueError("a bn2 channel whose batch variance is exactly 0 together with eps = 0 (upstream divides by zero)")
        if fl[2]:                                              # likewise: that feature's rows come out NaN
            raise ValueError("a feature whose batch variance is exactly 0 together with eps = 0 (upstream divides by zero)")
        if fl[0]:
            raise ValueError("feature_map: non-finite values (a NaN or an infinity reached the batch statistics in training mode, or a "
                             "row's norm in eval mode; found on the device; the running statistics are left as they were)")
        if self.training:
            self.tracked["bn2"] += 1
            self.tracked["features"] += 1
        return StageOut(ctx["emb"], ctx["norms"], ctx)

    def backward(self, out: StageOut, grad_embeddings: torch.Tensor, renormalised: bool = False, need_input_grad: bool = True) -> StageGrad:
        """What autograd leaves in the stage's parameters for a cotangent `grad_embeddings` on the unit rows.  renormalised: the
        cotangent is that of the loop's AdaFace branch, `torch.div(features, torch.norm(features, 2, 1, True))`, whose norm is not
        detached."""
        ctx = out._ctx
        if ctx.get("stage") is not self:
            raise ValueError("backward: `out` was not produced by this stage")
        if not ctx["training"]:
            raise ValueError("backward: `out` comes from an eval-mode forward (the backward built is that of the batch statistics)")
        b, dev = ctx["b"], self.device
        g = grad_embeddings
        if not torch.is_tensor(g) or g.dtype != torch.float32 or tuple(g.shape) != (b, self.n):
            raise ValueError(f"grad_embeddings: expected fp32 [{b}, {self.n}], got {getattr(g, 'dtype', type(g))} "
                             f"{tuple(getattr(g, 'shape', ()))}")
        g = g.to(dev).contiguous()
        lib = _lib.load()
        d = self._desc(ctx["x"], ctx["keep"], True)
        need = lib.idb_tail_workspace_bytes(b, self.ch, self.hw, self.n, None, None)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        f32 = dict(dtype=torch.float32, device=dev)
        K = self.hw * self.ch
        gw2, gb2, gfb, gff = (torch.empty(self.ch, **f32), torch.empty(self.ch, **f32), torch.empty(self.n, **f32), torch.empty(self.n, **f32))
        gw = torch.empty((self.n, K), **f32)
        gx = torch.empty((b, self.hw, self.ch), **f32) if need_input_grad else None
        _lib.check(lib.idb_tail_backward(C.byref(d), g.data_ptr(), ctx["emb"].data_ptr(), ctx["norms"].data_ptr(), ctx["bn2_stat"].data_ptr(),
                                         ctx["affine"].data_ptr(), ctx["z"].data_ptr(), ctx["feat_stat"].data_ptr(), ctx["f"].data_ptr(),
                                         int(bool(renormalised)), gw2.data_ptr(), gb2.data_ptr(), gw.data_ptr(), gfb.data_ptr(),
                                         gff.data_ptr(), gx.data_ptr() if gx is not None else None, ws.data_ptr(), need,
                                         torch.cuda.current_stream(dev).cuda_stream), "idb_tail_backward")
        if gx is not None and ctx["x"].ndim == 4:
            gx = gx.view(ctx["x"].shape)
        return StageGrad(gw2, gb2, gw, gfb, gff, gx, self.hw, self.ch)


def _lib_shapes_refused(b: int, ch: int, hw: int, n: int) -> bool:
    return not (ch % 64 == 0 and 64 <= ch <= 2048 and 1 <= hw <= 64 and n % 64 == 0 and 64 <= n <= 1024 and 1 <= b <= MAX_B)


class StageSGD(ClippedSGD):
    """The loop's `clip_grad_norm_(model.parameters(), max_norm)` and `opt_backbone.step()` (torch.optim.SGD, momentum, weight decay on
    every tensor) over the stage's five trainable tensors with one joint norm (idb_sgd_clip_step).  `lr` may be reassigned between
    steps (the loop's scheduler: `learning_rate`).  State dict: {"lr", "momentum", "weight_decay", "max_norm", "steps",
    "momentum_buffers" ({name: fp32 on the host}, fc.weight in upstream's order; None before a step)}."""

    def __init__(self, stage: EmbeddingStage, lr: float, momentum: float = 0.9, weight_decay: float = 5e-4, max_norm: float = 5.0):
        if not isinstance(stage, EmbeddingStage):
            raise TypeError("StageSGD: stage must be an EmbeddingStage")
        super().__init__(lr, momentum, weight_decay, max_norm)
        self.stage = stage

    def _new_buffers(self) -> Dict[str, torch.Tensor]:
        return {k: torch.empty_like(self.stage.t[k]) for k in TRAINABLE}

    def _buffers_out(self, bufs):
        st = self.stage
        return {k: to_upstream_order(v, st.ch, st.hw) if k == "fc.weight" else v.clone() for k, v in bufs.items()}

    def _buffers_in(self, bufs) -> Dict[str, torch.Tensor]:
        st = self.stage
        if sorted(bufs) != sorted(TRAINABLE):
            raise ValueError(f"StageSGD state dict: momentum_buffers expected {sorted(TRAINABLE)}")
        new = {}
        for k in TRAINABLE:
            v = bufs[k].detach().to(torch.float32)
            want = (st.n, st.ch * st.hw) if k == "fc.weight" else tuple(st.t[k].shape)
            if tuple(v.shape) != want:
                raise ValueError(f"StageSGD state dict: momentum buffer {k} expected {want}")
            v = to_device_order(v, st.ch, st.hw) if k == "fc.weight" else v.contiguous().clone()
            new[k] = v.to(st.device) if st.device is not None else v
        return new

    def step(self, grad: StageGrad) -> float:
        """One clipped SGD step on the five tensors.  Returns the joint gradient norm before clipping, as clip_grad_norm_ does."""
        st = self.stage
        if st.device is None:
            raise _lib.IdbError("StageSGD.step: the stage is not on a device: call .to('cuda:0') first (there is no CPU fallback)")
        if not isinstance(grad, StageGrad):
            raise TypeError("StageSGD.step: expected the StageGrad of EmbeddingStage.backward")
        dev = st.device
        gs = {"bn2.weight": grad.bn2_weight, "bn2.bias": grad.bn2_bias, "fc.weight": grad.fc_weight, "fc.bias": grad.fc_bias,
              "features.bias": grad.features_bias}
        for k in TRAINABLE:
            if gs[k].dtype != torch.float32 or tuple(gs[k].shape) != tuple(st.t[k].shape) or gs[k].device != dev:
                raise ValueError(f"StageSGD.step: gradient of {k} expected fp32 {tuple(st.t[k].shape)} on {dev}")
            gs[k] = gs[k].contiguous()
        first = self._begin(dev)
        n = len(TRAINABLE)
        arr = lambda ts: (C.c_void_p * n)(*[t.data_ptr() for t in ts])      # noqa: E731
        numel = (C.c_int64 * n)(*[st.t[k].numel() for k in TRAINABLE])
        ws = torch.empty(_lib.IDB_SGD_CLIP_WS_BYTES, dtype=torch.uint8, device=dev)
        total = torch.zeros(1, dtype=torch.float64, device=dev)
        _lib.check(_lib.load().idb_sgd_clip_step(n, arr([st.t[k] for k in TRAINABLE]), arr([gs[k] for k in TRAINABLE]),
                                                 arr([self._buf[k] for k in TRAINABLE]), numel, self.lr, self.momentum, self.weight_decay,
                                                 self.max_norm, 1 if first else 0, total.data_ptr(), ws.data_ptr(),
                                                 _lib.IDB_SGD_CLIP_WS_BYTES, torch.cuda.current_stream(dev).cuda_stream), "idb_sgd_clip_step")
        return self._finish(float(total.item()))


def loss_backward(stage: EmbeddingStage, header: MarginHeader, out: StageOut, labels) -> Tuple[HeadLoss, HeadGrad, StageGrad]:
    """The loop's lines between the model and the optimisers (train_FR.py:280-290): the header's loss and gradients on the stage's
    unit rows, then the stage's backward.  AdaFace follows the loop's literal lines (`norm = torch.norm(features, 2, 1, True)`,
    `torch.div(features, norm)`), so the cotangent passes the second projection (renormalised=True)."""
    features = out.embeddings
    ada = header.loss_name == "AdaFace"
    if ada:
        norm = torch.norm(features, 2, 1, True)
        hl, hg = header.loss_and_grad(torch.div(features, norm), labels, norms=norm)
    else:
        hl, hg = header.loss_and_grad(features, labels)
    return hl, hg, stage.backward(out, hg.embeddings, renormalised=ada)


def train_step(stage: EmbeddingStage, header: MarginHeader, opt_stage: StageSGD, opt_header: HeaderSGD, feature_map, labels, keep=None,
               generator: Optional[torch.Generator] = None) -> Dict[str, object]:
    """The loop body of train_FR.py:279-296 from `features = F.normalize(model(images))` down to the two `opt.step()` calls, the trunk's
    output given.  AdaFace follows the loop's literal lines (`norm = torch.norm(features, 2, 1, True)`, `torch.div(features, norm)`),
    so the cotangent passes the second projection (renormalised=True).  Returns {"loss", "acc", "correct", "grad_norm_stage",
    "grad_norm_header" (both before clipping), "grad_input" (fp32 NHWC)}; loss and accuracy are those before the step, as logged."""
    if not isinstance(stage, EmbeddingStage) or not isinstance(opt_stage, StageSGD) or opt_stage.stage is not stage:
        raise TypeError("train_step: expected an EmbeddingStage and the StageSGD built on it")
    if not isinstance(header, MarginHeader) or not isinstance(opt_header, HeaderSGD) or opt_header.header is not header:
        raise TypeError("train_step: expected a MarginHeader and the HeaderSGD built on it")
    if not stage.training:
        raise ValueError("train_step: the stage is in eval mode")
    hl, hg, grad = loss_backward(stage, header, stage(feature_map, keep=keep, generator=generator), labels)
    norm_stage = opt_stage.step(grad)
    norm_header = opt_header.step(hg.kernel)
    return {"loss": hl.loss, "acc": hl.acc, "correct": hl.correct, "grad_norm_stage": norm_stage, "grad_norm_header": norm_header,
            "grad_input": grad.input}


def train_step_images(backbone, stage: EmbeddingStage, header: MarginHeader, opt_stage: StageSGD, opt_header: HeaderSGD, images, labels,
                      keep=None, generator: Optional[torch.Generator] = None) -> Dict[str, object]:
    """train_step after `backbone.features_map(images)`; the trunk is the folded eval network and stays frozen."""
    if getattr(backbone, "training", False):
        raise NotImplementedError("a trunk in training mode (batch-statistics BatchNorm inside the blocks) is not built: the trunk is the "
                                  "folded eval network")
    return train_step(stage, header, opt_stage, opt_header, backbone.features_map(images), labels, keep=keep, generator=generator)


def learning_rate(epoch: int, base: float = 0.1, batch_size: int = 128, world: int = 1, schedule: Sequence[int] = (22, 30, 35),
                  auto_schedule: bool = False) -> float:
    """The loop's LambdaLR (train_FR.py:197-215): FR_config.lr_step_func(epoch) = 0.1 ** #{m in schedule: m - 1 <= epoch}, times the
    optimiser's lr = base / 512 * batch_size * world.  Host only."""
    if auto_schedule:
        raise NotImplementedError("auto_schedule's ReduceLROnPlateau depends on the validation history and is not built; pass the "
                                  "milestone schedule")
    if epoch < 0 or batch_size < 1 or world < 1:
        raise ValueError("learning_rate: expected epoch >= 0, batch_size >= 1, world >= 1")
    factor = 0.1 ** len([m for m in schedule if m - 1 <= epoch])
    return base / 512 * batch_size * world * factor
