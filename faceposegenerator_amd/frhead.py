"""The loss head of the reference's face-recognition training loop, forward and backward: the margin header (``FR_training/utils/losses.py``
``CosFace``, ``ArcFace``, ``AdaFace``), ``CrossEntropyLoss`` and ``multi_class_acc`` (``train_FR.py:279-302``, ``:373-377``), i.e. the
two numbers ``CallBackLogging`` prints at every step, for a checkpoint's ``<step>_backbone.pth`` / ``<step>_header.pth`` pair
(``CallBackModelCheckpointOld``, ``utils_callbacks.py:209-239``).

``MarginHeader.from_pretrained(path, loss)`` reads the header file; ``.to("cuda:0")`` uploads the kernel and packs it once
(``idb_head_pack``: transposed, every column L2-normalised in double); ``header(embeddings, label)`` / ``header(embeddings, norms,
label)`` return the ``thetas`` of upstream's ``forward``; ``header.loss(...)`` returns loss and top-1 without ever writing the B x C
matrix (``idb_head_loss``, ``csrc/idb_head.hip``: the cosine product on the exact f32-input MFMA, one log-sum-exp, one double target
logit and one argmax per row; bit-identical from run to run).  ``step_metrics`` is the loop body without the backward, ``validate``
averages it as the loop's ``AverageMeter``s do.  There is no CPU fallback.

Refused, each with a message that names the reason:
``ElasticCosFace`` -- its margins are ``torch.normal`` draws on the device, one per row and call: there is nothing to reproduce.
``NonLinearHeader`` -- the training loop never builds it.
A backbone in training mode (batch-statistics BatchNorm, dropout) -- the backbone here is the folded eval network, so what this module
reports is the validation loss of a checkpoint, not the training loss the loop logged while the weights were moving.
Also refused: labels outside [0, C) (upstream's headers skip ``-1`` but its ``CrossEntropyLoss`` then raises), a kernel with a zero or
non-finite column (upstream: ``0 / 0`` = NaN logits), non-finite or zero embedding rows (found on the device by the per-row launch:
the call raises after it, and a NaN norm leaves AdaFace's buffers unchanged), and AdaFace on a batch of one (the unbiased
standard deviation of one norm is NaN).

The backward: ``header.loss_and_grad(embeddings, label)`` returns the loss and what ``accelerator.backward(loss_v)``
(``train_FR.py:290``) leaves in ``header.kernel.grad`` and hands back through the embeddings (``idb_head_loss_grad``: the forward's
launches, then the softmax recomputed from the saved log-sum-exp and both gradient products on the f32 MFMA; no B x C matrix, no
floating-point atomics, bit-identical from run to run).  ``HeaderSGD`` is the loop's ``clip_grad_norm_(header.parameters(), 5)`` and
``opt_header.step()`` (SGD, momentum 0.9, weight decay 5e-4; ``train_FR.py:203-208``, ``:293``, ``:296``) with the kernel repacked
after every step, ``train_header_step`` the header's share of the loop body.  Off the target the derivative of
``cos(acos(c))`` is taken as its limit 1; upstream's autograd evaluates ``sin(acos c) / sqrt(1 - c^2)`` and gives NaN at a cosine of
exactly +-1.  A row whose target slope is not finite (an ArcFace target cosine of exactly +-1: upstream gives inf / NaN) is refused like
the bad rows above.

Out of scope: the convolutional trunk's backward (``dL/d embeddings`` is consumed by ``frtail.EmbeddingStage.backward``),
top-5 (the loop logs 0 for it), sharding C over several GPUs.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, Iterable, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._frtrain import ClippedSGD, hip_device

LOSSES = {"CosFace": _lib.IDB_HEAD_COSFACE, "ArcFace": _lib.IDB_HEAD_ARCFACE, "AdaFace": _lib.IDB_HEAD_ADAFACE}
DEFAULT_M = {"CosFace": 0.35, "ArcFace": 0.50, "AdaFace": 0.4}
MAX_B, MAX_D, MAX_C = 65536, 4096, 1 << 20
_REFUSED = {
    "ElasticCosFace": "ElasticCosFace draws its margins with torch.normal on the device at every call: there is no value to reproduce",
    "NonLinearHeader": "NonLinearHeader is not a margin header and the training loop never builds it",
}


_BAD_ROWS = ("embeddings: a zero or non-finite row, or a non-finite AdaFace norm (upstream returns NaN; found by the per-row launch, "
             "which marks such a row's target; AdaFace's buffers are left unchanged by NaN norms)")


class HeadLoss(NamedTuple):
    """loss: the mean, = CrossEntropyLoss()(thetas, label) (float); per_sample, lse, target_logit: float64 [B] on the device; pred:
    int32 [B]; correct: int; acc: multi_class_acc, round(100 * correct / B, 2); margin_scaler: float64 [B] (AdaFace, else zeros)."""
    loss: float
    per_sample: torch.Tensor
    lse: torch.Tensor
    target_logit: torch.Tensor
    pred: torch.Tensor
    correct: int
    acc: float
    margin_scaler: torch.Tensor


class HeadGrad(NamedTuple):
    """embeddings: dL/d embeddings, fp32 [B, D]; kernel: dL/d kernel, fp32 [D, C] (the layout of kernel.grad); target_slope: float64
    [B], dz_target / (s dcos_target) with the clamp (and AdaFace's clip) folded in: 0 where the target is clamped away."""
    embeddings: torch.Tensor
    kernel: torch.Tensor
    target_slope: torch.Tensor


_BAD_SLOPE = ("embeddings: a target cosine of exactly +-1 under ArcFace: the slope sin(acos(c) + m) / sqrt(1 - c^2) is not finite "
              "(upstream's autograd gives inf / NaN)")


def multi_class_acc(correct: int, batch: int) -> float:
    """train_FR.py:373-377 from the count: acc = correct / batch, then round(acc * 100, 2)."""
    acc = correct / batch
    return round(acc * 100, 2)


def dataset_labels(file_names: Sequence[str]) -> Tuple[np.ndarray, int]:
    """(labels int64 [N], num_classes) by ArcBiFaceGANDataset's rule (utils/dataset.py:255, :269): the label of a file is
    int(name.split("_")[0]), the number of classes the largest label + 1."""
    names = list(file_names)
    if not names:
        raise ValueError("dataset_labels: no file names")
    try:
        labels = np.array([int(str(n).split("_")[0]) for n in names], dtype=np.int64)
    except ValueError as e:
        raise ValueError(f"dataset_labels: a file name does not start with '<integer>_': {e}") from None
    if labels.min() < 0:
        raise ValueError("dataset_labels: negative label")
    return labels, int(labels.max()) + 1


def _check_loss(loss: str) -> str:
    if loss in _REFUSED:
        raise NotImplementedError(_REFUSED[loss])
    if loss not in LOSSES:
        raise ValueError(f"loss {loss!r}: expected one of {sorted(LOSSES)}")
    return loss


def _host_labels(label, batch: int, classes: int) -> torch.Tensor:
    t = label if torch.is_tensor(label) else torch.from_numpy(np.ascontiguousarray(label))
    if t.is_floating_point() or t.dtype == torch.bool or t.reshape(-1).shape[0] != batch:
        raise ValueError(f"label: expected {batch} integer labels, got {t.dtype} {tuple(t.shape)}")
    t = t.reshape(-1).cpu().to(torch.int64)
    if int(t.min()) < 0 or int(t.max()) >= classes:
        raise ValueError(f"label: values in [{int(t.min())}, {int(t.max())}], expected [0, {classes}) (upstream's CrossEntropyLoss raises "
                         f"on a label outside the classes, -1 included)")
    return t.to(torch.int32)


class MarginHeader:
    """A margin header of FR_training/utils/losses.py with upstream's constructor defaults; `kernel` is the [in_features, out_features]
    parameter.  AdaFace keeps upstream's buffers t, batch_mean, batch_std (`buffers`, default 0 / 20 / 100) and updates the last two on
    every call, in train and eval alike, as upstream does."""

    def __init__(self, kernel, loss: str, s: float = 64.0, m: Optional[float] = None, h: float = 0.333, t_alpha: float = 1.0,
                 buffers: Optional[Dict[str, float]] = None):
        self.loss_name = _check_loss(loss)
        k = kernel if torch.is_tensor(kernel) else torch.from_numpy(np.asarray(kernel))
        if k.ndim != 2 or not k.is_floating_point():
            raise ValueError(f"kernel: expected a floating-point [in_features, out_features] matrix, got {k.dtype} {tuple(k.shape)}")
        d, c = int(k.shape[0]), int(k.shape[1])
        if not (1 <= d <= MAX_D and 1 <= c <= MAX_C):
            raise ValueError(f"kernel {(d, c)}: in_features in 1..{MAX_D}, out_features in 1..{MAX_C}")
        k = k.detach().to("cpu", torch.float32).contiguous()
        norms = k.double().norm(dim=0)
        if not bool(torch.isfinite(norms).all()) or bool((norms == 0).any()):
            raise ValueError("kernel: a zero or non-finite column (upstream divides it by its norm: NaN logits)")
        self._kernel_host, self._kernel_stale = k, False
        self.in_features, self.out_features = d, c
        self.s = float(s)
        self.m = float(DEFAULT_M[loss] if m is None else m)
        self.h, self.t_alpha = float(h), float(t_alpha)
        if not (0.0 < self.s <= 1e4 and np.isfinite(self.m) and np.isfinite(self.h) and 0.0 <= self.t_alpha <= 1.0):
            raise ValueError("expected s in (0, 1e4], finite m and h, t_alpha in [0, 1]")
        b = dict(t=0.0, batch_mean=20.0, batch_std=100.0)
        b.update({key: float(torch.as_tensor(v).reshape(-1)[0]) for key, v in (buffers or {}).items()})
        if set(b) != {"t", "batch_mean", "batch_std"}:
            raise ValueError(f"buffers: expected t, batch_mean, batch_std, got {sorted(b)}")
        self.t = b["t"]
        self._state = torch.tensor([b["batch_mean"], b["batch_std"]], dtype=torch.float64)
        self.device: Optional[torch.device] = None
        self._kernel_dev = self._wn = self._col_norm = None

    # ---- construction ---------------------------------------------------------------------------------------------------------
    @classmethod
    def from_state_dict(cls, sd, loss: str, **kw) -> "MarginHeader":
        _check_loss(loss)
        if "kernel" not in sd:
            raise ValueError(f"header state dict without 'kernel' (keys: {sorted(sd)[:6]})")
        buffers = None
        if loss == "AdaFace":
            missing = [k for k in ("t", "batch_mean", "batch_std") if k not in sd]
            if missing:
                raise ValueError(f"AdaFace header state dict without {missing}")
            buffers = {k: sd[k] for k in ("t", "batch_mean", "batch_std")}
        return cls(sd["kernel"], loss, buffers=buffers, **kw)

    @classmethod
    def from_pretrained(cls, path: str, loss: str, **kw) -> "MarginHeader":
        """`path`: a <step>_header.pth as CallBackModelCheckpointOld writes it (header.state_dict())."""
        _check_loss(loss)
        return cls.from_state_dict(torch.load(path, weights_only=True, map_location="cpu"), loss, **kw)

    @classmethod
    def from_synthetic(cls, in_features: int, out_features: int, seed: int, loss: str, **kw) -> "MarginHeader":
        """normal(std=0.01), as upstream initialises CosFace and ArcFace (AdaFace's own initialisation is a uniform draw renormalised
        per row; the direction statistics of the columns are the same)."""
        g = torch.Generator().manual_seed(seed)
        return cls(torch.randn(int(in_features), int(out_features), generator=g) * 0.01, loss, **kw)

    @property
    def kernel(self) -> torch.Tensor:
        """The parameter, fp32 [in_features, out_features] on the host; after a HeaderSGD step it is fetched from the device."""
        if self._kernel_stale:
            self._kernel_host, self._kernel_stale = self._kernel_dev.cpu(), False
        return self._kernel_host

    def state_dict(self) -> Dict[str, torch.Tensor]:
        sd = {"kernel": self.kernel.clone()}
        if self.loss_name == "AdaFace":
            mean, std = self._state.cpu().tolist()
            sd.update(t=torch.tensor([self.t]), batch_mean=torch.tensor([mean]), batch_std=torch.tensor([std]))
        return sd

    @property
    def batch_mean(self) -> float:
        return float(self._state[0])

    @property
    def batch_std(self) -> float:
        return float(self._state[1])

    def set_buffers(self, batch_mean: float, batch_std: float) -> None:
        self._state.copy_(torch.tensor([float(batch_mean), float(batch_std)], dtype=torch.float64))

    def to(self, device) -> "MarginHeader":
        dev = hip_device(device, "MarginHeader")
        lib = _lib.load()
        self.device = dev
        self._kernel_dev = self.kernel.to(dev)
        self._state = self._state.to(dev)
        d, c = self.in_features, self.out_features
        self._wn = torch.empty((c, d), dtype=torch.float32, device=dev)
        self._col_norm = torch.empty(c, dtype=torch.float64, device=dev)
        bad = torch.empty(1, dtype=torch.int32, device=dev)
        _lib.check(lib.idb_head_pack(self._kernel_dev.data_ptr(), d, c, self._wn.data_ptr(), self._col_norm.data_ptr(), bad.data_ptr(),
                                     torch.cuda.current_stream(dev).cuda_stream), "idb_head_pack")
        if int(bad.item()) != 0:
            raise ValueError(f"kernel: {int(bad.item())} zero or non-finite column(s)")
        return self

    # ---- calls ----------------------------------------------------------------------------------------------------------------
    def _desc(self, embeddings, label, norms):
        ada = self.loss_name == "AdaFace"
        if not torch.is_tensor(embeddings):
            embeddings = torch.from_numpy(np.ascontiguousarray(embeddings))
        if embeddings.ndim != 2 or not embeddings.is_floating_point() or embeddings.shape[1] != self.in_features:
            raise ValueError(f"embeddings: expected a floating-point [B, {self.in_features}] matrix, got {embeddings.dtype} "
                             f"{tuple(embeddings.shape)}")
        b = int(embeddings.shape[0])
        if not 1 <= b <= MAX_B:
            raise ValueError(f"batch {b}: expected 1..{MAX_B}")
        if ada and b < 2:
            raise ValueError("AdaFace needs a batch of at least 2: the unbiased standard deviation of one norm is NaN")
        if ada == (norms is None):
            raise ValueError("AdaFace takes (embeddings, norms, label), CosFace and ArcFace take (embeddings, label)")
        lab = _host_labels(label, b, self.out_features)
        if ada:
            if not torch.is_tensor(norms):
                norms = torch.from_numpy(np.ascontiguousarray(norms))
            if not norms.is_floating_point() or norms.numel() != b:
                raise ValueError(f"norms: expected {b} floating-point values, got {norms.dtype} {tuple(norms.shape)}")
        if self.device is None:
            raise _lib.IdbError("MarginHeader is not on a device: call .to('cuda:0') first (it packs the kernel; there is no CPU fallback)")
        dev = self.device
        e = embeddings.to(device=dev, dtype=torch.float32).contiguous()
        n = norms.to(device=dev, dtype=torch.float32).reshape(-1).contiguous() if ada else None
        lab = lab.to(dev)
        d = _lib.HeadDesc()
        d.kind, d.b, d.d, d.c = LOSSES[self.loss_name], b, self.in_features, self.out_features
        d.s, d.m, d.h, d.t_alpha = self.s, self.m, self.h, self.t_alpha
        d.emb, d.norms, d.label = e.data_ptr(), (n.data_ptr() if ada else None), lab.data_ptr()
        d.kernel, d.wn, d.col_norm = self._kernel_dev.data_ptr(), self._wn.data_ptr(), self._col_norm.data_ptr()
        d.ada_state = self._state.data_ptr() if ada else None
        lib = _lib.load()
        need = lib.idb_head_workspace_bytes(b, d.d, d.c, None, None)
        if need == 0:
            raise _lib.IdbError(f"idb_head_workspace_bytes({b}, {d.d}, {d.c}) refused its arguments")
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        return lib, d, (e, n, lab, ws), need

    def plan(self, batch: int) -> Tuple[int, int]:
        """(row tiles, column blocks) of the loss launch for a batch: idb_head_workspace_bytes' geometry."""
        rt, cb = C.c_int32(0), C.c_int32(0)
        if _lib.load().idb_head_workspace_bytes(int(batch), self.in_features, self.out_features, C.byref(rt), C.byref(cb)) == 0:
            raise ValueError(f"batch {batch}: expected 1..{MAX_B}")
        return rt.value, cb.value

    def __call__(self, embeddings, *args) -> torch.Tensor:
        """header(embeddings, label) for CosFace / ArcFace, header(embeddings, norms, label) for AdaFace: thetas [B, C] fp32."""
        if len(args) not in (1, 2):
            raise TypeError("header(embeddings, label) or header(embeddings, norms, label)")
        norms, label = (args[0], args[1]) if len(args) == 2 else (None, args[0])
        lib, d, keep, need = self._desc(embeddings, label, norms)
        dev = self.device
        thetas = torch.empty((d.b, d.c), dtype=torch.float32, device=dev)
        rows = torch.empty((5, d.b), dtype=torch.float64, device=dev)
        _lib.check(lib.idb_head_logits(C.byref(d), thetas.data_ptr(), rows.data_ptr(), keep[3].data_ptr(), need,
                                       torch.cuda.current_stream(dev).cuda_stream), "idb_head_logits")
        if not bool(torch.isfinite(rows[2]).all()):
            raise ValueError(_BAD_ROWS)
        return thetas

    def loss(self, embeddings, label, norms=None) -> HeadLoss:
        """Loss and top-1 of a batch without the B x C matrix.  AdaFace: norms is required (and the buffers are updated)."""
        lib, d, keep, need = self._desc(embeddings, label, norms)
        dev = self.device
        rows = torch.empty((5, d.b), dtype=torch.float64, device=dev)
        pred = torch.empty(d.b, dtype=torch.int32, device=dev)
        both = torch.zeros(16, dtype=torch.uint8, device=dev)      # bytes 0-7 the mean loss (double), 8-11 the count (int32): one read
        _lib.check(lib.idb_head_loss(C.byref(d), rows.data_ptr(), pred.data_ptr(), both.data_ptr(), both.data_ptr() + 8, keep[3].data_ptr(),
                                     need, torch.cuda.current_stream(dev).cuda_stream), "idb_head_loss")
        host = both.cpu()
        mean, n_ok = float(host[:8].view(torch.float64)[0]), int(host[8:12].view(torch.int32)[0])
        if not math.isfinite(mean):                            # the prep launch gives a bad row a NaN target, which the mean carries
            raise ValueError(_BAD_ROWS)
        return HeadLoss(mean, rows[1], rows[0], rows[2], pred, n_ok, multi_class_acc(n_ok, d.b), rows[4])

    def grad_plan(self, batch: int) -> Tuple[int, int, int]:
        """(row tiles, class blocks, D chunks) of the backward's dX launch for a batch: idb_head_grad_workspace_bytes' geometry."""
        rt, cb, ch = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        if _lib.load().idb_head_grad_workspace_bytes(int(batch), self.in_features, self.out_features, C.byref(rt), C.byref(cb),
                                                     C.byref(ch)) == 0:
            raise ValueError(f"batch {batch} x {self.in_features} x {self.out_features} classes: outside 1..{MAX_B}, or more than 2^27 "
                             f"floats of dX partials (class blocks x batch x in_features)")
        return rt.value, cb.value, ch.value

    def loss_and_grad(self, embeddings, label, norms=None) -> Tuple[HeadLoss, "HeadGrad"]:
        """header.loss(...) and the gradients of its mean loss w.r.t. the embeddings and the kernel, in one call (AdaFace's buffers
        advance once, `norms` is detached as upstream).  Neither the probabilities nor their gradient are ever written."""
        lib, d, keep, _ = self._desc(embeddings, label, norms)
        dev = self.device
        need = lib.idb_head_grad_workspace_bytes(d.b, d.d, d.c, None, None, None)
        if need == 0:
            raise ValueError(f"loss_and_grad: batch {d.b} x {d.d} x {d.c} classes needs more than 2^27 floats of dX partials (class "
                             f"blocks x batch x in_features): split the batch")
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        rows = torch.empty((5, d.b), dtype=torch.float64, device=dev)
        grad_rows = torch.empty((3, d.b), dtype=torch.float64, device=dev)
        pred = torch.empty(d.b, dtype=torch.int32, device=dev)
        d_emb = torch.empty((d.b, d.d), dtype=torch.float32, device=dev)
        d_kernel = torch.empty((d.d, d.c), dtype=torch.float32, device=dev)
        both = torch.zeros(16, dtype=torch.uint8, device=dev)
        _lib.check(lib.idb_head_loss_grad(C.byref(d), rows.data_ptr(), pred.data_ptr(), both.data_ptr(), both.data_ptr() + 8,
                                          grad_rows.data_ptr(), d_emb.data_ptr(), d_kernel.data_ptr(), ws.data_ptr(), need,
                                          torch.cuda.current_stream(dev).cuda_stream), "idb_head_loss_grad")
        host = both.cpu()
        mean, n_ok = float(host[:8].view(torch.float64)[0]), int(host[8:12].view(torch.int32)[0])
        if not math.isfinite(mean):
            raise ValueError(_BAD_ROWS)
        if not bool(torch.isfinite(grad_rows[0]).all()):
            raise ValueError(_BAD_SLOPE)
        out = HeadLoss(mean, rows[1], rows[0], rows[2], pred, n_ok, multi_class_acc(n_ok, d.b), rows[4])
        return out, HeadGrad(d_emb, d_kernel, grad_rows[0])


class HeaderSGD(ClippedSGD):
    """The header's optimiser of train_FR.py: clip_grad_norm_(header.parameters(), max_norm) (:293), then torch.optim.SGD(lr, momentum,
    weight_decay).step() (:203-208, :296) on header.kernel, fp32 state as torch, one call (idb_head_sgd_step); the header is repacked
    inside it, so the next forward sees the stepped kernel.  `lr` may be reassigned between steps (the loop's scheduler).  State dict:
    {"lr", "momentum", "weight_decay", "max_norm", "steps", "momentum_buffer" (fp32 [D, C] on the host, None before a step)}."""
    _KEY = "momentum_buffer"
    _EXIST = "a momentum buffer exists"

    def __init__(self, header: MarginHeader, lr: float, momentum: float = 0.9, weight_decay: float = 5e-4, max_norm: float = 5.0):
        if not isinstance(header, MarginHeader):
            raise TypeError("HeaderSGD: header must be a MarginHeader")
        super().__init__(lr, momentum, weight_decay, max_norm)
        self.header = header

    def _shape(self):
        return (self.header.in_features, self.header.out_features)

    def _new_buffers(self) -> torch.Tensor:
        return torch.empty(self._shape(), dtype=torch.float32, device=self.header.device)

    def _buffers_out(self, buf: torch.Tensor) -> torch.Tensor:
        return buf.clone()

    def _buffers_in(self, buf) -> torch.Tensor:
        if not torch.is_tensor(buf) or tuple(buf.shape) != self._shape():
            raise ValueError(f"HeaderSGD state dict: momentum_buffer expected {self._shape()}")
        return buf.detach().to(torch.float32).contiguous().clone()

    def step(self, grad_kernel: torch.Tensor) -> float:
        """One clipped SGD step on header.kernel with `grad_kernel` (fp32 [D, C], HeadGrad.kernel).  Returns the gradient's L2 norm
        before clipping, as clip_grad_norm_ does."""
        hd = self.header
        if hd.device is None:
            raise _lib.IdbError("HeaderSGD.step: the header is not on a device: call .to('cuda:0') first (there is no CPU fallback)")
        shape = self._shape()
        if not torch.is_tensor(grad_kernel) or tuple(grad_kernel.shape) != shape or grad_kernel.dtype != torch.float32:
            raise ValueError(f"HeaderSGD.step: grad_kernel expected fp32 {shape}")
        dev = hd.device
        g = grad_kernel.to(dev).contiguous()
        first = self._begin(dev)
        ws = torch.empty(_lib.IDB_HEAD_SGD_WS_BYTES, dtype=torch.uint8, device=dev)
        both = torch.zeros(16, dtype=torch.uint8, device=dev)      # bytes 0-7 the norm (double), 8-11 the bad columns (int32): one read
        lib = _lib.load()
        _lib.check(lib.idb_head_sgd_step(hd._kernel_dev.data_ptr(), g.data_ptr(), self._buf.data_ptr(), shape[0], shape[1], self.lr,
                                         self.momentum, self.weight_decay, self.max_norm, 1 if first else 0, hd._wn.data_ptr(),
                                         hd._col_norm.data_ptr(), both.data_ptr() + 8, both.data_ptr(), ws.data_ptr(),
                                         _lib.IDB_HEAD_SGD_WS_BYTES, torch.cuda.current_stream(dev).cuda_stream), "idb_head_sgd_step")
        hd._kernel_stale = True
        self.steps += 1
        host = both.cpu()
        norm, bad = float(host[:8].view(torch.float64)[0]), int(host[8:12].view(torch.int32)[0])
        if bad != 0 or not math.isfinite(norm):
            raise ValueError(f"HeaderSGD.step: the step left {bad} zero or non-finite kernel column(s) (gradient norm {norm})")
        return norm


def train_header_step(header: MarginHeader, opt: HeaderSGD, embeddings, labels, norms=None) -> Dict[str, object]:
    """The header's share of the loop body (train_FR.py:286-298): forward, loss, backward, clip_grad_norm_, opt_header.step().  Returns
    {"loss", "acc", "correct", "grad_embeddings" (fp32 [B, D], for whatever trains the backbone), "grad_norm" (before clipping)}; the
    loss and accuracy are those of the kernel BEFORE the step, as the loop logs them."""
    if not isinstance(header, MarginHeader) or not isinstance(opt, HeaderSGD) or opt.header is not header:
        raise TypeError("train_header_step: expected a MarginHeader and the HeaderSGD built on it")
    out, grad = header.loss_and_grad(embeddings, labels, norms=norms)
    norm = opt.step(grad.kernel)
    return {"loss": out.loss, "acc": out.acc, "correct": out.correct, "grad_embeddings": grad.embeddings, "grad_norm": norm}


def step_metrics(backbone, header: MarginHeader, images, labels, training: bool = False) -> Dict[str, float]:
    """The loop body of train_FR.py:279-302 without the backward: features = F.normalize(backbone(images)), the header, the loss and
    multi_class_acc.  Returns {"loss", "acc", "correct", "features"}.

    AdaFace follows the loop literally: the loop takes `norm = torch.norm(features, 2, 1, True)` of the ALREADY normalised features, so
    every norm is 1 up to fp32 rounding, the batch standard deviation is rounding noise and the adaptive margin with it
    (margin_scaler = clip((norm - mean) / (std + 1e-3) * h, -1, 1) of values ~1e-8 apart).  The general path with true feature norms
    is header.loss(embeddings, label, norms=...).

    training=True, or a backbone whose `.training` is set, is refused: the backbone here is the folded eval network."""
    if training or getattr(backbone, "training", False):
        raise NotImplementedError("a backbone in training mode (batch-statistics BatchNorm, dropout) is not built: the backbone is the "
                                  "folded eval network, so this is the validation loss of a checkpoint, not the logged training loss")
    if not isinstance(header, MarginHeader):
        raise TypeError("step_metrics: header must be a MarginHeader")
    features = torch.nn.functional.normalize(backbone(images))
    if header.loss_name == "AdaFace":
        norm = torch.norm(features, 2, 1, True)
        out = header.loss(torch.div(features, norm), labels, norms=norm)
    else:
        out = header.loss(features, labels)
    return {"loss": out.loss, "acc": out.acc, "correct": out.correct, "features": features}


def average_meters(losses: Iterable[float], accs: Iterable[float]) -> Dict[str, float]:
    """The loop's AverageMeters (utils_logging.py:8-29): losses.update(loss, 1) and top1.update(acc) per step; avg = sum / count with
    the sum accumulated one step at a time."""
    loss_sum, acc_sum, count = 0, 0, 0
    for lv, av in zip(losses, accs):
        loss_sum += lv * 1
        acc_sum += av * 1
        count += 1
    if count == 0:
        raise ValueError("validate: no batch")
    return {"loss": loss_sum / count, "top1": acc_sum / count, "steps": count}


def validate(backbone, header: MarginHeader, batches) -> Dict[str, float]:
    """{"loss", "top1", "steps"} over an iterable of (images, labels): the per-step loss averaged with weight 1 and the per-step
    ROUNDED accuracy averaged, exactly as the loop's AverageMeters do (not the loss per sample, nor correct / total)."""
    steps = [step_metrics(backbone, header, images, labels) for images, labels in batches]
    return average_meters([s["loss"] for s in steps], [s["acc"] for s in steps])
