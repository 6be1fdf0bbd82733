"""The convolutional trunk of the reference's face-recognition backbone in training, forward and backward: the stem lines of
``IResNet.forward`` (``conv1`` -> ``bn1`` -> ``prelu``) and ``IBasicBlock`` (``FR_training/backbones/iresnet.py``) with batch
statistics and running statistics, what ``accelerator.backward`` leaves in every trainable tensor, and the loop's joint
``clip_grad_norm_(model.parameters(), 5)`` + ``opt_backbone.step()`` over the whole backbone (``train_FR.py``).  With
``frtail.EmbeddingStage`` and ``frhead.MarginHeader`` this is the loop body with nothing frozen (``train_step_full``).
``csrc/idb_block.hip``: fp32 state, every product on the exact f32-input MFMA, statistics in double, bit-identical from run to run.

Layout.  Activations and their gradients are NHWC ``[B, H, W, C]`` fp32.  Conv weights live on the device as ``[cout][ky][kx][cin]``
(``conv_to_device`` / ``conv_to_upstream`` convert); gradients come in that layout too, and ``state_dict`` returns upstream's.  The
stem reads a 4-channel repack of the float NCHW batch (``augment.apply(output="float")``), its weight padded to ``cin = 4``.

The backward of a block uses the parameters as they are when it is called: run it before the optimiser step, as the loop does.

Refused, each with a message: SE blocks and ``IBottleneck`` checkpoints, dilation, sharding, backward of an eval-mode forward, CPU
devices (there is no CPU fallback), non-finite input and a batch variance of exactly 0 with eps = 0 (found on the device; the running
statistics and batch counters are then left as they were), shapes outside the kernels' bounds.
"""
from __future__ import annotations

import ctypes as C
from collections import OrderedDict
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import _lib
from ._frtrain import ClippedSGD, hip_device
from .arcface import _BN, ARCHS, PLANES, trunk_param_shapes
from .frhead import HeaderSGD, MarginHeader
from .frtail import TRAINABLE as STAGE_TRAINABLE
from .frtail import EmbeddingStage, StageGrad, loss_backward, to_device_order, to_upstream_order

EPS, MOMENTUM = 1e-5, 0.1
MAX_B, MAX_HW, MAX_C = 1024, 128, 2048


def conv_to_device(w: torch.Tensor) -> torch.Tensor:
    """[cout][cin][ky][kx] (upstream) -> [cout][ky][kx][cin]."""
    return w.permute(0, 2, 3, 1).contiguous()


def conv_to_upstream(w: torch.Tensor) -> torch.Tensor:
    return w.permute(0, 3, 1, 2).contiguous()


def _is_buffer(key: str) -> bool:
    return key.endswith(("running_mean", "running_var", "num_batches_tracked"))


def _refuse_unbuilt(sd, what: str) -> None:
    for k in sd:
        if ".se." in k or ".se_block." in k:
            raise NotImplementedError(f"{what}: an SE checkpoint ({k}): SE blocks are not built")
        if k.endswith("conv3.weight"):
            raise NotImplementedError(f"{what}: an IBottleneck checkpoint ({k}; iresnet50_2): only IBasicBlock networks are built")


def _device(device) -> torch.device:
    return hip_device(device, "the trunk")


def _stream(dev) -> int:
    return torch.cuda.current_stream(dev).cuda_stream


def conv_out(h: int, ksize: int, stride: int) -> int:
    return (h + 2 * (1 if ksize == 3 else 0) - ksize) // stride + 1


def conv_plan(b: int, h: int, w: int, cin: int, cout: int, ksize: int, stride: int) -> Tuple[int, int, int]:
    """(workspace bytes, wgrad slices, dgrad row tiles) of one convolution: idb_blk_conv_workspace_bytes' geometry."""
    sl, rt = C.c_int32(0), C.c_int32(0)
    need = _lib.load().idb_blk_conv_workspace_bytes(b, h, w, cin, cout, ksize, stride, C.byref(sl), C.byref(rt))
    if need == 0:
        raise ValueError(f"convolution b {b}, {h} x {w}, {cin} -> {cout}, ksize {ksize}, stride {stride}: outside the kernels' bounds "
                         f"(b <= {MAX_B}, h and w in 1..{MAX_HW}, cin 4 or % 64 == 0, cout % 64 == 0, both <= {MAX_C})")
    return int(need), sl.value, rt.value


# ---- the kernels, one call each ----------------------------------------------------------------------------------------------------
def _ptr(t: Optional[torch.Tensor]):
    return t.data_ptr() if t is not None else None


def _conv_desc(x, affine, slope, w, stride) -> _lib.BlkConvDesc:
    d = _lib.BlkConvDesc()
    d.b, d.h, d.w, d.cin = (int(v) for v in x.shape)
    d.cout, d.ksize, d.stride = int(w.shape[0]), int(w.shape[1]), int(stride)
    d.x, d.affine, d.slope, d.weight = x.data_ptr(), _ptr(affine), _ptr(slope), w.data_ptr()
    return d


def _conv_fwd(x, affine, slope, w, stride) -> torch.Tensor:
    d = _conv_desc(x, affine, slope, w, stride)
    out = torch.empty((d.b, conv_out(d.h, d.ksize, d.stride), conv_out(d.w, d.ksize, d.stride), d.cout), dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().idb_blk_conv_forward(C.byref(d), out.data_ptr(), _stream(x.device)), "idb_blk_conv_forward")
    return out


def _conv_dgrad(x, affine, slope, w, stride, g) -> torch.Tensor:
    d = _conv_desc(x, affine, slope, w, stride)
    gi = torch.empty(tuple(x.shape), dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().idb_blk_conv_dgrad(C.byref(d), g.data_ptr(), gi.data_ptr(), _stream(x.device)), "idb_blk_conv_dgrad")
    return gi


def _conv_wgrad(x, affine, slope, w, stride, g) -> torch.Tensor:
    d = _conv_desc(x, affine, slope, w, stride)
    need, _, _ = conv_plan(d.b, d.h, d.w, d.cin, d.cout, d.ksize, d.stride)
    ws = torch.empty(need, dtype=torch.uint8, device=x.device)
    dw = torch.empty(tuple(w.shape), dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().idb_blk_conv_wgrad(C.byref(d), g.data_ptr(), dw.data_ptr(), ws.data_ptr(), need, _stream(x.device)),
               "idb_blk_conv_wgrad")
    return dw


def _bn_ws(rows: int, ch: int, dev) -> Tuple[torch.Tensor, int]:
    need = _lib.load().idb_blk_bn_workspace_bytes(rows, ch, None)
    if need == 0:
        raise ValueError(f"BatchNorm over {rows} rows of {ch} channels: outside the kernels' bounds")
    return torch.empty(need, dtype=torch.uint8, device=dev), int(need)


def _bn_fwd(t: Dict[str, torch.Tensor], key: str, x: torch.Tensor, training: bool, flags: torch.Tensor):
    """-> (stat double [2][ch], affine fp32 [2][ch]); the running statistics of `key` are updated in training."""
    ch = int(x.shape[-1])
    rows = x.numel() // ch
    ws, need = _bn_ws(rows, ch, x.device)
    stat = torch.empty((2, ch), dtype=torch.float64, device=x.device)
    aff = torch.empty((2, ch), dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().idb_blk_bn_forward(x.data_ptr(), rows, ch, int(training), EPS, MOMENTUM, t[f"{key}.weight"].data_ptr(),
                                              t[f"{key}.bias"].data_ptr(), t[f"{key}.running_mean"].data_ptr(),
                                              t[f"{key}.running_var"].data_ptr(), stat.data_ptr(), aff.data_ptr(), flags.data_ptr(),
                                              ws.data_ptr(), need, _stream(x.device)), "idb_blk_bn_forward")
    return stat, aff


def _bn_bwd(c, g, stat, aff, gamma, slope=None, add=None):
    """-> (g_c, d_gamma, d_beta, d_slope or None)."""
    ch = int(c.shape[-1])
    rows = c.numel() // ch
    ws, need = _bn_ws(rows, ch, c.device)
    f32 = dict(dtype=torch.float32, device=c.device)
    dg, db = torch.empty(ch, **f32), torch.empty(ch, **f32)
    dsl = torch.empty(ch, **f32) if slope is not None else None
    gc = torch.empty(tuple(c.shape), **f32)
    _lib.check(_lib.load().idb_blk_bn_backward(c.data_ptr(), g.data_ptr(), rows, ch, stat.data_ptr(), aff.data_ptr(), gamma.data_ptr(),
                                               _ptr(slope), _ptr(add), dg.data_ptr(), db.data_ptr(), _ptr(dsl), gc.data_ptr(), ws.data_ptr(),
                                               need, _stream(c.device)), "idb_blk_bn_backward")
    return gc, dg, db, dsl


def _affine(c, aff, slope=None, identity=None, id_aff=None) -> torch.Tensor:
    ch = int(c.shape[-1])
    out = torch.empty_like(c)
    _lib.check(_lib.load().idb_blk_affine(c.data_ptr(), aff.data_ptr(), _ptr(slope), _ptr(identity), _ptr(id_aff), c.numel() // ch, ch,
                                          out.data_ptr(), _stream(c.device)), "idb_blk_affine")
    return out


# ---- modules -----------------------------------------------------------------------------------------------------------------------
class BlockOut:
    """output: fp32 NHWC; ctx: the saved context of the backward (the input, the raw conv outputs c1, c2, cd, and per BatchNorm `stat`
    (double [2][ch] mean, invstd) and `affine` (fp32 [2][ch] sc, sh))."""
    __slots__ = ("output", "ctx")

    def __init__(self, output: torch.Tensor, ctx: dict):
        self.output, self.ctx = output, ctx


class BlockGrad:
    """params: {upstream key: gradient}, conv weights in the device layout [cout][ky][kx][cin] (`upstream()` converts); input: the
    gradient with respect to the module's input, fp32 NHWC (None for the stem)."""
    __slots__ = ("params", "input")

    def __init__(self, params: Dict[str, torch.Tensor], inp: Optional[torch.Tensor]):
        self.params, self.input = params, inp

    def upstream(self) -> Dict[str, torch.Tensor]:
        return grads_upstream(self.params)


def grads_upstream(grads: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """Gradients by upstream key in upstream's layouts (conv weights [cout][cin][ky][kx])."""
    return {k: conv_to_upstream(v) if v.ndim == 4 else v for k, v in grads.items()}


class _Module:
    """Shared plumbing of TrainBlock and TrainStem: tensors by upstream key (conv weights in the device layout), batch counters."""
    bns: Tuple[str, ...] = ()

    def _load(self, sd, shapes: Dict[str, Tuple[int, ...]], what: str) -> None:
        _refuse_unbuilt(sd, what)
        missing = [k for k in shapes if k not in sd and not k.endswith("num_batches_tracked")]
        if missing:
            raise ValueError(f"{what}: the state dict lacks {missing}")
        self.t: Dict[str, torch.Tensor] = {}
        self.tracked: Dict[str, int] = {}
        for k, shp in shapes.items():
            if k.endswith("num_batches_tracked"):
                self.tracked[k] = int(sd[k]) if k in sd else 0
                continue
            if tuple(sd[k].shape) != tuple(shp):
                raise ValueError(f"{what}: {k} expected {tuple(shp)}, got {tuple(sd[k].shape)}")
            v = sd[k].detach().to("cpu", torch.float32).contiguous().clone()
            self.t[k] = conv_to_device(v) if v.ndim == 4 else v
        self.training = True
        self.device: Optional[torch.device] = None

    def to(self, device):
        dev = _device(device)
        _lib.load()
        self.t = {k: v.to(dev).contiguous() for k, v in self.t.items()}
        self.device = dev
        return self

    def train(self, mode: bool = True):
        self.training = bool(mode)
        return self

    def eval(self):
        return self.train(False)

    def trainable(self) -> List[str]:
        """The trainable tensors' keys in upstream's model.parameters() order."""
        return [k for k in self.t if not _is_buffer(k)]

    def state_dict(self) -> Dict[str, torch.Tensor]:
        """Upstream's key names and layouts, on the host."""
        sd = {k: (conv_to_upstream(v.detach().cpu()) if v.ndim == 4 else v.detach().cpu().clone()) for k, v in self.t.items()}
        for k, n in self.tracked.items():
            sd[k] = torch.tensor(n, dtype=torch.int64)
        return {k: sd[k] for k in self._shapes}

    def _check_input(self, x, ch_axis: int, ch: int, what: str) -> None:
        if self.device is None:
            raise _lib.IdbError(f"{what} is not on a device: call .to('cuda:0') first (there is no CPU fallback)")
        if not torch.is_tensor(x) or x.dtype != torch.float32 or x.ndim != 4 or x.shape[ch_axis] != ch or x.shape[0] < 1:
            raise ValueError(f"{what}: expected a float32 tensor with {ch} channels on axis {ch_axis}, got {getattr(x, 'dtype', type(x))} "
                             f"{tuple(getattr(x, 'shape', ()))}")
        if x.device != self.device:
            raise ValueError(f"{what}: input on {x.device}, the module is on {self.device} (there is no CPU fallback)")
        hw = [int(x.shape[i]) for i in (1, 2, 3) if i != ch_axis]
        if x.shape[0] > MAX_B or not all(1 <= v <= MAX_HW for v in hw):
            raise ValueError(f"{what}: batch {x.shape[0]} (1..{MAX_B}), size {hw} (1..{MAX_HW})")
        if self.training and x.shape[0] * hw[0] * hw[1] < 2:
            raise ValueError(f"{what}: one value per channel in training mode (upstream's BatchNorm raises: no batch variance)")

    # a forward's BatchNorm launches raise flags on the device; a caller that chains modules checks them all at once (pending list)
    def _begin(self):
        flags = torch.zeros((len(self.bns), 2), dtype=torch.int32, device=self.device)
        saved = {}
        if self.training:
            for bn in self.bns:
                for f in ("running_mean", "running_var"):
                    saved[f"{bn}.{f}"] = self.t[f"{bn}.{f}"].clone()
        return flags, saved

    def _finish(self, flags, saved, pending) -> None:
        entry = (self, flags, saved, self.training)
        if pending is not None:
            pending.append(entry)
        else:
            _settle([entry])


def _settle(pending) -> None:
    """One device-to-host read of every pending forward's flags; any raised flag puts every running statistic back and raises."""
    if not pending:
        return
    fl = torch.cat([e[1] for e in pending]).cpu()
    if bool(fl.any()):
        for mod, _, saved, _ in pending:
            for k, v in saved.items():
                mod.t[k].copy_(v)
        if bool(fl[:, 1].any()):
            raise ValueError("a BatchNorm channel whose batch variance is exactly 0 together with eps = 0 (upstream divides by zero)")
        raise ValueError("non-finite values reached a BatchNorm's batch statistics (found on the device; the running statistics are left "
                         "as they were)")
    for mod, _, _, training in pending:
        if training:
            for bn in mod.bns:
                mod.tracked[f"{bn}.num_batches_tracked"] += 1


class TrainBlock(_Module):
    """One IBasicBlock in upstream's key names under `prefix` (bn1, conv1, bn2, prelu, conv2, bn3, optional downsample.0 / .1)."""

    def __init__(self, sd: Dict[str, torch.Tensor], prefix: str, cin: int, planes: int, stride: int, dilation: int = 1):
        if dilation != 1:
            raise NotImplementedError("TrainBlock: dilation is not built (upstream's IBasicBlock refuses it too)")
        if stride not in (1, 2):
            raise ValueError("TrainBlock: stride 1 or 2")
        p = prefix if (not prefix or prefix.endswith(".")) else prefix + "."
        self.prefix, self.cin, self.planes, self.stride = p, int(cin), int(planes), int(stride)
        self.has_ds = f"{p}downsample.0.weight" in sd
        if (stride != 1 or cin != planes) and not self.has_ds:
            raise ValueError(f"TrainBlock {p}: stride {stride}, {cin} -> {planes} needs the downsample branch ({p}downsample.0.weight)")
        shapes: "OrderedDict[str, Tuple[int, ...]]" = OrderedDict()

        def bn(key, c):
            for f in _BN:
                shapes[f"{p}{key}.{f}"] = () if f == "num_batches_tracked" else (c,)

        bn("bn1", cin)
        shapes[f"{p}conv1.weight"] = (planes, cin, 3, 3)
        bn("bn2", planes)
        shapes[f"{p}prelu.weight"] = (planes,)
        shapes[f"{p}conv2.weight"] = (planes, planes, 3, 3)
        bn("bn3", planes)
        self.bns = (f"{p}bn1", f"{p}bn2", f"{p}bn3")
        if self.has_ds:
            shapes[f"{p}downsample.0.weight"] = (planes, cin, 1, 1)
            bn("downsample.1", planes)
            self.bns += (f"{p}downsample.1",)
        for c in (cin, planes):
            if c % 64 != 0 or not 64 <= c <= MAX_C:
                raise ValueError(f"TrainBlock {p}: {c} channels (% 64 == 0, <= {MAX_C})")
        self._shapes = shapes
        self._load(sd, shapes, f"TrainBlock {p}")

    def __call__(self, x: torch.Tensor, _pending: Optional[list] = None) -> BlockOut:
        self._check_input(x, 3, self.cin, f"TrainBlock {self.prefix}")
        x = x.contiguous()
        p, t, tr, s = self.prefix, self.t, self.training, self.stride
        flags, saved = self._begin()
        st1, af1 = _bn_fwd(t, f"{p}bn1", x, tr, flags[0])
        c1 = _conv_fwd(x, af1, None, t[f"{p}conv1.weight"], 1)
        st2, af2 = _bn_fwd(t, f"{p}bn2", c1, tr, flags[1])
        c2 = _conv_fwd(c1, af2, t[f"{p}prelu.weight"], t[f"{p}conv2.weight"], s)
        st3, af3 = _bn_fwd(t, f"{p}bn3", c2, tr, flags[2])
        ctx = dict(x=x, c1=c1, c2=c2, cd=None, stat1=st1, affine1=af1, stat2=st2, affine2=af2, stat3=st3, affine3=af3, statd=None, affined=None,
                   training=tr, module=self)
        if self.has_ds:
            cd = _conv_fwd(x, None, None, t[f"{p}downsample.0.weight"], s)
            std, afd = _bn_fwd(t, f"{p}downsample.1", cd, tr, flags[3])
            ctx.update(cd=cd, statd=std, affined=afd)
            out = _affine(c2, af3, None, cd, afd)
        else:
            out = _affine(c2, af3, None, x, None)
        self._finish(flags, saved, _pending)
        return BlockOut(out, ctx)

    def backward(self, out: BlockOut, grad: torch.Tensor) -> BlockGrad:
        """What autograd leaves in the block's nine (twelve with the downsample branch) parameters for a cotangent `grad` on the
        output, and the gradient with respect to the input."""
        ctx = out.ctx
        if ctx.get("module") is not self:
            raise ValueError("backward: `out` was not produced by this block")
        if not ctx["training"]:
            raise ValueError("backward: `out` comes from an eval-mode forward (the backward built is that of the batch statistics)")
        g = _check_grad(grad, out.output)
        p, t, s, x, c1, c2 = self.prefix, self.t, self.stride, ctx["x"], ctx["c1"], ctx["c2"]
        slope, w1, w2 = t[f"{p}prelu.weight"], t[f"{p}conv1.weight"], t[f"{p}conv2.weight"]
        gr: Dict[str, torch.Tensor] = {}
        g_c2, gr[f"{p}bn3.weight"], gr[f"{p}bn3.bias"], _ = _bn_bwd(c2, g, ctx["stat3"], ctx["affine3"], t[f"{p}bn3.weight"])
        gr[f"{p}conv2.weight"] = _conv_wgrad(c1, ctx["affine2"], slope, w2, s, g_c2)
        g_a2 = _conv_dgrad(c1, ctx["affine2"], slope, w2, s, g_c2)
        g_c1, gr[f"{p}bn2.weight"], gr[f"{p}bn2.bias"], gr[f"{p}prelu.weight"] = _bn_bwd(c1, g_a2, ctx["stat2"], ctx["affine2"],
                                                                                         t[f"{p}bn2.weight"], slope)
        gr[f"{p}conv1.weight"] = _conv_wgrad(x, ctx["affine1"], None, w1, 1, g_c1)
        g_a1 = _conv_dgrad(x, ctx["affine1"], None, w1, 1, g_c1)
        add = g
        if self.has_ds:
            wd, cd = t[f"{p}downsample.0.weight"], ctx["cd"]
            g_cd, gr[f"{p}downsample.1.weight"], gr[f"{p}downsample.1.bias"], _ = _bn_bwd(cd, g, ctx["statd"], ctx["affined"],
                                                                                        t[f"{p}downsample.1.weight"])
            gr[f"{p}downsample.0.weight"] = _conv_wgrad(x, None, None, wd, s, g_cd)
            add = _conv_dgrad(x, None, None, wd, s, g_cd)
        g_x, gr[f"{p}bn1.weight"], gr[f"{p}bn1.bias"], _ = _bn_bwd(x, g_a1, ctx["stat1"], ctx["affine1"], t[f"{p}bn1.weight"], None, add)
        return BlockGrad({k: gr[k] for k in self.trainable()}, g_x)


def _check_grad(grad, like: torch.Tensor) -> torch.Tensor:
    if not torch.is_tensor(grad) or grad.dtype != torch.float32 or tuple(grad.shape) != tuple(like.shape) or grad.device != like.device:
        raise ValueError(f"grad: expected fp32 {tuple(like.shape)} on {like.device}, got {getattr(grad, 'dtype', type(grad))} "
                         f"{tuple(getattr(grad, 'shape', ()))}")
    return grad.contiguous()


class TrainStem(_Module):
    """conv1 (3 -> 64, 3x3, stride 1) -> bn1 -> prelu of IResNet.forward; the input is the float NCHW batch."""

    def __init__(self, sd: Dict[str, torch.Tensor], prefix: str = ""):
        p = prefix if (not prefix or prefix.endswith(".")) else prefix + "."
        self.prefix = p
        shapes: "OrderedDict[str, Tuple[int, ...]]" = OrderedDict()
        shapes[f"{p}conv1.weight"] = (64, 3, 3, 3)
        for f in _BN:
            shapes[f"{p}bn1.{f}"] = () if f == "num_batches_tracked" else (64,)
        shapes[f"{p}prelu.weight"] = (64,)
        self.bns = (f"{p}bn1",)
        self._shapes = shapes
        self._load(sd, shapes, "TrainStem")

    def _padded_weight(self) -> torch.Tensor:
        w = self.t[f"{self.prefix}conv1.weight"]
        wp = torch.zeros((64, 3, 3, 4), dtype=torch.float32, device=w.device)
        wp[..., :3] = w
        return wp

    def __call__(self, images: torch.Tensor, _pending: Optional[list] = None) -> BlockOut:
        self._check_input(images, 1, 3, "TrainStem")
        img = images.contiguous()
        b, _, h, w = (int(v) for v in img.shape)
        p, t, tr = self.prefix, self.t, self.training
        x4 = torch.empty((b, h, w, 4), dtype=torch.float32, device=self.device)
        _lib.check(_lib.load().idb_blk_pack_images(img.data_ptr(), b, h, w, x4.data_ptr(), _stream(self.device)), "idb_blk_pack_images")
        wp = self._padded_weight()
        flags, saved = self._begin()
        c = _conv_fwd(x4, None, None, wp, 1)
        st, af = _bn_fwd(t, f"{p}bn1", c, tr, flags[0])
        out = _affine(c, af, t[f"{p}prelu.weight"])
        self._finish(flags, saved, _pending)
        return BlockOut(out, dict(x=x4, c1=c, stat1=st, affine1=af, weight=wp, training=tr, module=self))

    def backward(self, out: BlockOut, grad: torch.Tensor) -> BlockGrad:
        ctx = out.ctx
        if ctx.get("module") is not self:
            raise ValueError("backward: `out` was not produced by this stem")
        if not ctx["training"]:
            raise ValueError("backward: `out` comes from an eval-mode forward (the backward built is that of the batch statistics)")
        g = _check_grad(grad, out.output)
        p, t = self.prefix, self.t
        gr: Dict[str, torch.Tensor] = {}
        g_c, gr[f"{p}bn1.weight"], gr[f"{p}bn1.bias"], gr[f"{p}prelu.weight"] = _bn_bwd(ctx["c1"], g, ctx["stat1"], ctx["affine1"],
                                                                                       t[f"{p}bn1.weight"], t[f"{p}prelu.weight"])
        gr[f"{p}conv1.weight"] = _conv_wgrad(ctx["x"], None, None, ctx["weight"], 1, g_c)[..., :3].contiguous()      # the pad channel dropped
        return BlockGrad({k: gr[k] for k in self.trainable()}, None)


class TrunkOut:
    """map: layer4's output, fp32 NHWC, what EmbeddingStage takes; outs: the stem's and every block's BlockOut in order."""
    __slots__ = ("map", "outs", "trunk")

    def __init__(self, fmap: torch.Tensor, outs: List[BlockOut], trunk: "Trunk"):
        self.map, self.outs, self.trunk = fmap, outs, trunk


class Trunk:
    """The stem plus the blocks of an IResNet: `arch` one of r18 / r34 / r50 / r100 (arcface.ARCHS), or `layers`, the four block
    counts.  Any input size whose map stays >= 1 x 1 (and <= 128 x 128) is accepted."""

    def __init__(self, sd: Dict[str, torch.Tensor], arch: Optional[str] = None, layers: Optional[Sequence[int]] = None, dilation: int = 1,
                 world_size: int = 1):
        if dilation != 1:
            raise NotImplementedError("Trunk: dilation (replace_stride_with_dilation) is not built")
        if world_size != 1:
            raise NotImplementedError("Trunk: sharding over devices is not built (one device holds the whole backbone)")
        _refuse_unbuilt(sd, "Trunk")
        if (arch is None) == (layers is None):
            raise ValueError("Trunk: give either arch or layers")
        if arch is not None:
            if arch not in ARCHS:
                raise ValueError(f"Trunk: unknown arch {arch!r}; one of {sorted(ARCHS)}")
            layers = ARCHS[arch]
        layers = [int(v) for v in layers]
        if len(layers) != 4 or any(v < 1 for v in layers):
            raise ValueError("Trunk: layers is four block counts >= 1")
        self.arch, self.layers = arch, layers
        self.shapes = trunk_param_shapes(layers)
        self.stem = TrainStem(sd)
        self.blocks: List[TrainBlock] = []
        cin = 64
        for i, (nb, planes) in enumerate(zip(layers, PLANES)):
            for j in range(nb):
                self.blocks.append(TrainBlock(sd, f"layer{i + 1}.{j}.", cin if j == 0 else planes, planes, 2 if j == 0 else 1))
            cin = planes
        self.training = True
        self.device: Optional[torch.device] = None

    @property
    def modules(self) -> List[_Module]:
        return [self.stem] + list(self.blocks)

    def to(self, device) -> "Trunk":
        for m in self.modules:
            m.to(device)
        self.device = self.stem.device
        return self

    def train(self, mode: bool = True) -> "Trunk":
        self.training = bool(mode)
        for m in self.modules:
            m.train(mode)
        return self

    def eval(self) -> "Trunk":
        return self.train(False)

    def trainable(self) -> List[str]:
        return [k for m in self.modules for k in m.trainable()]

    def tensor(self, key: str) -> torch.Tensor:
        for m in self.modules:
            if key in m.t:
                return m.t[key]
        raise KeyError(key)

    def state_dict(self) -> Dict[str, torch.Tensor]:
        sd: Dict[str, torch.Tensor] = {}
        for m in self.modules:
            sd.update(m.state_dict())
        return {k: sd[k] for k in self.shapes}

    def merged_state_dict(self, stage: EmbeddingStage) -> Dict[str, torch.Tensor]:
        """A whole <step>_backbone.pth in upstream's layout: the trunk's tensors, then the stage's."""
        sd = self.state_dict()
        sd.update(stage.state_dict())
        return sd

    def map_size(self, h: int, w: int) -> Tuple[int, int]:
        for _ in range(4):
            h, w = conv_out(h, 3, 2), conv_out(w, 3, 2)
        return h, w

    def __call__(self, images: torch.Tensor) -> TrunkOut:
        if self.device is None:
            raise _lib.IdbError("Trunk is not on a device: call .to('cuda:0') first (there is no CPU fallback)")
        pending: list = []
        outs = [self.stem(images, _pending=pending)]
        try:
            for blk in self.blocks:
                outs.append(blk(outs[-1].output, _pending=pending))
        finally:
            _settle(pending)      # also after a refusal part-way: what ran is checked, and put back if a flag was raised
        return TrunkOut(outs[-1].output, outs, self)

    def backward(self, out: TrunkOut, grad_map: torch.Tensor) -> Dict[str, torch.Tensor]:
        """Gradients of every trainable tensor by upstream key, in upstream's parameter order; conv weights in the device layout
        [cout][ky][kx][cin] (grads_upstream converts)."""
        if not isinstance(out, TrunkOut) or out.trunk is not self:
            raise ValueError("backward: `out` was not produced by this trunk")
        g = grad_map
        got: Dict[str, torch.Tensor] = {}
        for blk, bo in zip(reversed(self.blocks), reversed(out.outs[1:])):
            bg = blk.backward(bo, g)
            got.update(bg.params)
            g = bg.input
        got.update(self.stem.backward(out.outs[0], g).params)
        return {k: got[k] for k in self.trainable()}


class BackboneSGD(ClippedSGD):
    """The loop's `clip_grad_norm_(model.parameters(), max_norm)` and `opt_backbone.step()` over every trainable tensor of trunk and
    stage in upstream's model.parameters() order, with one joint norm (idb_sgd_clip_step_table).  `lr` may be reassigned between
    steps (frtail.learning_rate).  State dict: {"lr", "momentum", "weight_decay", "max_norm", "steps", "momentum_buffers" ({key: fp32
    on the host} in upstream's layouts; None before a step)}."""

    def __init__(self, trunk: Trunk, stage: EmbeddingStage, lr: float, momentum: float = 0.9, weight_decay: float = 5e-4, max_norm: float = 5.0):
        if not isinstance(trunk, Trunk) or not isinstance(stage, EmbeddingStage):
            raise TypeError("BackboneSGD: expected a Trunk and an EmbeddingStage")
        super().__init__(lr, momentum, weight_decay, max_norm)
        self.trunk, self.stage = trunk, stage
        self.keys: List[str] = trunk.trainable() + list(STAGE_TRAINABLE)
        if len(self.keys) > 1024:
            raise ValueError(f"BackboneSGD: {len(self.keys)} tensors, idb_sgd_clip_step_table takes at most 1024")
        self._tables = None

    def _weight(self, key: str) -> torch.Tensor:
        return self.stage.t[key] if key in STAGE_TRAINABLE else self.trunk.tensor(key)

    def _new_buffers(self) -> Dict[str, torch.Tensor]:
        return {k: torch.empty_like(self._weight(k)) for k in self.keys}

    def _buffers_out(self, bufs):
        st = self.stage
        return {k: to_upstream_order(v, st.ch, st.hw) if k == "fc.weight" else conv_to_upstream(v) if v.ndim == 4 else v.clone()
                for k, v in bufs.items()}

    def _buffers_in(self, bufs) -> Dict[str, torch.Tensor]:
        if sorted(bufs) != sorted(self.keys):
            raise ValueError("BackboneSGD state dict: momentum_buffers do not match the backbone's trainable tensors")
        st, new = self.stage, {}
        for k in self.keys:
            v = bufs[k].detach().to("cpu", torch.float32)
            v = to_device_order(v, st.ch, st.hw) if k == "fc.weight" else conv_to_device(v) if v.ndim == 4 else v.contiguous().clone()
            if tuple(v.shape) != tuple(self._weight(k).shape):
                raise ValueError(f"BackboneSGD state dict: momentum buffer {k} has the wrong shape")
            new[k] = v.to(self.trunk.device) if self.trunk.device is not None else v
        self._tables = None
        return new

    def step(self, trunk_grads: Dict[str, torch.Tensor], stage_grad: StageGrad) -> float:
        """One clipped SGD step on every tensor.  Returns the joint gradient norm before clipping, as clip_grad_norm_ does."""
        dev = self.trunk.device
        if dev is None or self.stage.device != dev:
            raise _lib.IdbError("BackboneSGD.step: trunk and stage must be on the same HIP device (there is no CPU fallback)")
        if not isinstance(stage_grad, StageGrad):
            raise TypeError("BackboneSGD.step: expected the StageGrad of EmbeddingStage.backward")
        gs = dict(trunk_grads)
        gs.update({"bn2.weight": stage_grad.bn2_weight, "bn2.bias": stage_grad.bn2_bias, "fc.weight": stage_grad.fc_weight,
                   "fc.bias": stage_grad.fc_bias, "features.bias": stage_grad.features_bias})
        ws_ = [self._weight(k) for k in self.keys]
        grads = []
        for k, w in zip(self.keys, ws_):
            g = gs.get(k)
            if g is None or g.dtype != torch.float32 or tuple(g.shape) != tuple(w.shape) or g.device != dev:
                raise ValueError(f"BackboneSGD.step: gradient of {k} expected fp32 {tuple(w.shape)} on {dev}")
            grads.append(g.contiguous())
        first = self._begin(dev)
        if first:
            self._tables = None
        n = len(self.keys)
        i64 = lambda vals: torch.tensor(vals, dtype=torch.int64).to(dev)      # noqa: E731
        if self._tables is None or self._tables[3] != [w.data_ptr() for w in ws_]:
            bufs = [self._buf[k] for k in self.keys]
            self._tables = (i64([w.data_ptr() for w in ws_]), i64([b.data_ptr() for b in bufs]), i64([w.numel() for w in ws_]),
                            [w.data_ptr() for w in ws_])
        tw, tb, tn, _ = self._tables
        tg = i64([g.data_ptr() for g in grads])
        lib = _lib.load()
        need = lib.idb_sgd_clip_table_workspace_bytes(n)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        total = torch.zeros(1, dtype=torch.float64, device=dev)
        _lib.check(lib.idb_sgd_clip_step_table(n, tw.data_ptr(), tg.data_ptr(), tb.data_ptr(), tn.data_ptr(), self.lr, self.momentum,
                                               self.weight_decay, self.max_norm, 1 if first else 0, total.data_ptr(), ws.data_ptr(), need,
                                               _stream(dev)), "idb_sgd_clip_step_table")
        return self._finish(float(total.item()))


def train_step_full(trunk: Trunk, stage: EmbeddingStage, header: MarginHeader, opt_backbone: BackboneSGD, opt_header: HeaderSGD, images, labels,
                    keep=None, generator: Optional[torch.Generator] = None) -> Dict[str, object]:
    """The loop body of train_FR.py from `features = F.normalize(model(images))` to the two `opt.step()` calls with nothing frozen.
    images: float32 NCHW on the device.  Returns what frtail.train_step returns ({"loss", "acc", "correct", "grad_norm_stage",
    "grad_norm_header", "grad_input"}) plus "grad_norm_backbone": the joint norm over trunk and stage before clipping
    ("grad_norm_stage" is that same joint norm: the stage's tensors are clipped together with the trunk's; "grad_input" is None: no
    gradient with respect to the images is formed)."""
    if not isinstance(trunk, Trunk) or not isinstance(stage, EmbeddingStage):
        raise TypeError("train_step_full: expected a Trunk and an EmbeddingStage")
    if not isinstance(opt_backbone, BackboneSGD) or opt_backbone.trunk is not trunk or opt_backbone.stage is not stage:
        raise TypeError("train_step_full: expected the BackboneSGD built on this trunk and stage")
    if not isinstance(header, MarginHeader) or not isinstance(opt_header, HeaderSGD) or opt_header.header is not header:
        raise TypeError("train_step_full: expected a MarginHeader and the HeaderSGD built on it")
    if not trunk.training or not stage.training:
        raise ValueError("train_step_full: the trunk or the stage is in eval mode")
    tout = trunk(images)
    hl, hg, grad = loss_backward(stage, header, stage(tout.map, keep=keep, generator=generator), labels)
    tgrads = trunk.backward(tout, grad.input)
    norm_backbone = opt_backbone.step(tgrads, grad)
    norm_header = opt_header.step(hg.kernel)
    return {"loss": hl.loss, "acc": hl.acc, "correct": hl.correct, "grad_norm_stage": norm_backbone, "grad_norm_backbone": norm_backbone,
            "grad_norm_header": norm_header, "grad_input": None}
