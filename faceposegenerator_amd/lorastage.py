"""One (resnet, attention) stage of the UNet, trainable on the device: the layers that lie between two transformer blocks, so that the
gradient of a later block's loss reaches an earlier block's adapters (train_ID-Booth.py:672-678 trains the rank-4 adapters of every
attention module of the UNet together).

``TrainResnetBlock`` is diffusers' ``ResnetBlock2D`` (GroupNorm + SiLU -> conv1 3x3 -> + time_emb_proj(SiLU(temb)) -> GroupNorm + SiLU
-> conv2 3x3 -> + shortcut, Dropout(0), output_scale_factor 1), in the up path over the channel concatenation x | skip.
``LoRATransformer2D`` is ``Transformer2DModel`` with ``use_linear_projection``: GroupNorm -> proj_in -> ``LoRATransformerBlock``s ->
proj_out -> + input.  ``LoRAStage`` is the pair, as CrossAttnDownBlock2D, UNetMidBlock2DCrossAttn and CrossAttnUpBlock2D chain them, and
``train_stage_step`` runs a chain of stages forward, backward and through one ``LoRAAdamW`` step.

Every weight of the resnet and of the wrapper is frozen upstream (peft marks only the adapters trainable), so their backward is the
INPUT gradient alone.  A stride-1, padding-1 3x3 convolution's input gradient is the same convolution of the output gradient with the
weight flipped in both spatial axes and its channel axes swapped (``w.flip(2, 3).transpose(0, 1)``); a Linear's or 1x1 convolution's is
``idb_gemm`` with the transposed matrix; GroupNorm's (with the SiLU) is ``idb_groupnorm_bwd``, which also adds the shortcut's or
residual's gradient.  The forward keeps the raw inputs of each GroupNorm and their statistics partials (``idb_groupnorm_stats``; one
extra read of the tensor per norm) and recomputes the normalised tensors in the backward.  ``temb`` gets no gradient: nothing trainable
lies behind it.  Downsample2D / Upsample2D, conv_in / conv_out and the loss gradient are not built.  There is no CPU fallback."""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Callable, Dict, List, Optional, Sequence, Tuple, Union

import torch

from . import _lib as L
from ._frtrain import hip_device
from .lorablock import BlockOut, LoRAAdamW, LoRATransformerBlock

SD = Dict[str, torch.Tensor]


class _Device:
    """What the two layers share: the library handle, the stream, a growing workspace, idb_gemm and the three GroupNorm entry points."""
    device: Optional[torch.device] = None
    dtype = torch.float16

    def _bind(self, device, dtype, who: str) -> None:
        if dtype not in (torch.float16, torch.bfloat16):
            raise ValueError(f"{who}: operand dtype must be float16 or bfloat16")
        self.device, self.dtype = hip_device(device, who), dtype
        self.lib = L.load()
        self.dt = L.IDB_F16 if dtype == torch.float16 else L.IDB_BF16
        self._ws = torch.empty(0, dtype=torch.uint8, device=self.device)
        self._gn_ws = torch.empty(0, dtype=torch.uint8, device=self.device)

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def _workspace(self, nbytes: int) -> torch.Tensor:
        if self._ws.numel() < nbytes:
            self._ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        return self._ws

    def _norm_workspace(self, nbytes: int) -> torch.Tensor:
        if self._gn_ws.numel() < nbytes:
            self._gn_ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        return self._gn_ws

    def _gemm(self, srcs, w: torch.Tensor, n: int, batch: int, h: int, w_: int, **kw) -> torch.Tensor:
        """idb_gemm on the batch x h x w_ grid: srcs [(tensor, channels, taps)], w [n][K] with one K segment per source."""
        out = torch.empty((batch * h * w_, n), dtype=self.dtype, device=self.device)
        ptr = {k: (None if v is None else v.data_ptr()) if k in ("bias", "sample_bias", "residual") else v for k, v in kw.items()}
        d = L.gemm_desc(self.dt, [(t.data_ptr(), ch, taps, h, w_) for t, ch, taps in srcs], w.data_ptr(), n, batch, h, w_, out=out.data_ptr(), **ptr)
        L.check(L.run_gemm(self.lib, d, self._workspace, self._stream()), "idb_gemm")
        return out

    def _pack_conv(self, w: torch.Tensor) -> torch.Tensor:
        """[cout][cin][kh][kw] fp32 -> [cout][kh kw][cin] operand dtype (idb_pack_conv_weight)."""
        cout, cin, kh, kw = w.shape
        src = w.detach().to(device=self.device, dtype=torch.float32).contiguous()
        dst = torch.empty((cout, kh * kw * cin), dtype=self.dtype, device=self.device)
        L.check(self.lib.idb_pack_conv_weight(src.data_ptr(), dst.data_ptr(), cout, cin, kh * kw, self.dt, self._stream()), "idb_pack_conv_weight")
        return dst

    def _gn_stats(self, x0, c0, x1, c1, batch, hw, groups) -> Tuple[torch.Tensor, int]:
        part = torch.empty((batch * 64 * groups * 2,), dtype=torch.float32, device=self.device)
        chunks = C.c_int32()
        L.check(self.lib.idb_groupnorm_stats(x0.data_ptr(), c0, None if x1 is None else x1.data_ptr(), c1, batch, hw, groups, part.data_ptr(),
                                             part.numel() * 4, C.byref(chunks), self.dt, self._stream()), "idb_groupnorm_stats")
        return part, chunks.value

    def _gn(self, x0, c0, x1, c1, batch, hw, groups, eps, gamma, beta, silu) -> torch.Tensor:
        out = torch.empty((batch * hw, c0 + c1), dtype=self.dtype, device=self.device)
        need = self.lib.idb_groupnorm_workspace_bytes(batch, hw, groups)
        ws = self._norm_workspace(need)
        L.check(self.lib.idb_groupnorm(x0.data_ptr(), c0, None if x1 is None else x1.data_ptr(), c1, batch, hw, groups, eps, gamma.data_ptr(),
                                       beta.data_ptr(), int(silu), out.data_ptr(), self.dt, ws.data_ptr(), ws.numel(), None, 0, None, 0, self._stream()),
                "idb_groupnorm")
        return out

    def _gn_bwd(self, x0, c0, x1, c1, stats, dy, add, batch, hw, groups, eps, gamma, beta, silu) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        part, chunks = stats
        dx0 = torch.empty((batch * hw, c0), dtype=self.dtype, device=self.device)
        dx1 = torch.empty((batch * hw, c1), dtype=self.dtype, device=self.device) if c1 else None
        need = self.lib.idb_groupnorm_bwd_workspace_bytes(batch, hw, groups)
        ws = self._norm_workspace(need)
        L.check(self.lib.idb_groupnorm_bwd(x0.data_ptr(), c0, None if x1 is None else x1.data_ptr(), c1, part.data_ptr(), chunks, dy.data_ptr(),
                                           None if add is None else add.data_ptr(), gamma.data_ptr(), beta.data_ptr(), eps, int(silu), dx0.data_ptr(),
                                           None if dx1 is None else dx1.data_ptr(), batch, hw, groups, self.dt, ws.data_ptr(), ws.numel(), self._stream()),
                "idb_groupnorm_bwd")
        return dx0, dx1


def _vec(sd: SD, key: str, n: int, who: str) -> torch.Tensor:
    t = sd[key]
    if tuple(t.shape) != (n,):
        raise ValueError(f"{who}: {key} is {tuple(t.shape)}, expected ({n},)")
    return t.detach().float().contiguous()


def _check_groups(who: str, channels: int, groups: int) -> None:
    if groups <= 0 or channels % groups or channels // groups < 2:
        raise ValueError(f"{who}: {groups} groups do not divide {channels} channels into groups of at least 2")


# ---- ResnetBlock2D ----------------------------------------------------------------------------------------------------------------------
@dataclass
class ResnetOut:
    """The output and what the backward needs: the raw inputs, conv1's raw output and the statistics partials of the two GroupNorms."""
    out: torch.Tensor                          # [b][h][w][cout]
    x: torch.Tensor                            # [b][h][w][cin]
    skip: Optional[torch.Tensor]               # [b][h][w][skip]
    stats1: Tuple[torch.Tensor, int]           # (partials of x | skip, their pixel chunks)
    conv1: torch.Tensor                        # [b h w][cout]: conv1 + bias + time_emb_proj, before norm2
    stats2: Tuple[torch.Tensor, int]


@dataclass
class ResnetGrad:
    input: torch.Tensor                        # [b][h][w][cin]
    skip: Optional[torch.Tensor]               # [b][h][w][skip], None without a skip input


class TrainResnetBlock(_Device):
    KEYS = ("norm1.weight", "norm1.bias", "conv1.weight", "conv1.bias", "time_emb_proj.weight", "time_emb_proj.bias", "norm2.weight", "norm2.bias",
            "conv2.weight", "conv2.bias")

    def __init__(self, sd: SD, prefix: str, cin: int, cout: int, skip: int = 0, groups: int = 32, eps: float = 1e-5):
        who = "TrainResnetBlock"
        for name, v in (("cin", cin), ("cout", cout)):
            if v <= 0 or v % 64:
                raise ValueError(f"{who}: {name} must be a positive multiple of 64 (idb_gemm), got {v}")
        if skip < 0 or skip % 64:
            raise ValueError(f"{who}: skip must be 0 or a positive multiple of 64 (idb_gemm), got {skip}")
        ctot = cin + skip
        _check_groups(who, ctot, groups)
        _check_groups(who, cout, groups)
        missing = [k for k in self.KEYS if f"{prefix}.{k}" not in sd]
        if missing:
            raise KeyError(f"{who}: the state dict has no {prefix}.{missing[0]}")
        self.prefix, self.cin, self.cout, self.skip, self.groups, self.eps = prefix, cin, cout, skip, groups, float(eps)
        self.has_shortcut = f"{prefix}.conv_shortcut.weight" in sd
        if not self.has_shortcut and (skip or cin != cout):
            raise ValueError(f"{who}: {ctot} -> {cout} channels need a conv_shortcut, and {prefix} has none")
        f = lambda k: sd[f"{prefix}.{k}"].detach().float().contiguous()       # noqa: E731
        self.host: SD = {"norm1.weight": _vec(sd, f"{prefix}.norm1.weight", ctot, who), "norm1.bias": _vec(sd, f"{prefix}.norm1.bias", ctot, who),
                         "norm2.weight": _vec(sd, f"{prefix}.norm2.weight", cout, who), "norm2.bias": _vec(sd, f"{prefix}.norm2.bias", cout, who),
                         "conv1.bias": _vec(sd, f"{prefix}.conv1.bias", cout, who), "conv2.bias": _vec(sd, f"{prefix}.conv2.bias", cout, who),
                         "time_emb_proj.bias": _vec(sd, f"{prefix}.time_emb_proj.bias", cout, who),
                         "conv1.weight": f("conv1.weight"), "conv2.weight": f("conv2.weight"), "time_emb_proj.weight": f("time_emb_proj.weight")}
        if tuple(self.host["conv1.weight"].shape) != (cout, ctot, 3, 3) or tuple(self.host["conv2.weight"].shape) != (cout, cout, 3, 3):
            raise ValueError(f"{who}: conv1 / conv2 are {tuple(self.host['conv1.weight'].shape)} / {tuple(self.host['conv2.weight'].shape)}, expected "
                             f"({cout}, {ctot}, 3, 3) / ({cout}, {cout}, 3, 3)")
        tw = self.host["time_emb_proj.weight"]
        if tw.dim() != 2 or tw.shape[0] != cout:
            raise ValueError(f"{who}: time_emb_proj.weight is {tuple(tw.shape)}, expected ({cout}, time_embed_dim)")
        self.time_embed_dim = tw.shape[1]
        if self.has_shortcut:
            ws = f("conv_shortcut.weight")
            if tuple(ws.shape) not in ((cout, ctot, 1, 1), (cout, ctot)):
                raise ValueError(f"{who}: conv_shortcut.weight is {tuple(ws.shape)}, expected ({cout}, {ctot}, 1, 1)")
            self.host["conv_shortcut.weight"] = ws.reshape(cout, ctot, 1, 1)
            self.host["conv_shortcut.bias"] = _vec(sd, f"{prefix}.conv_shortcut.bias", cout, who)

    # ---- construction -------------------------------------------------------------------------------------------------------------
    @classmethod
    def from_state_dict(cls, sd: SD, prefix: str, skip: int = 0, groups: int = 32, eps: float = 1e-5) -> "TrainResnetBlock":
        """Sizes from the weights' shapes; `skip`: how many of conv1's input channels arrive as the second tensor."""
        w1 = sd[f"{prefix}.conv1.weight"]
        return cls(sd, prefix, w1.shape[1] - skip, w1.shape[0], skip, groups, eps)

    @classmethod
    def from_synthetic(cls, seed: int, cin: int = 64, cout: int = 64, skip: int = 0, time_embed_dim: int = 256, groups: int = 32, eps: float = 1e-5,
                       shortcut: Optional[bool] = None, prefix: str = "mid_block.resnets.0") -> "TrainResnetBlock":
        g = torch.Generator().manual_seed(seed)
        ctot = cin + skip
        shortcut = (skip > 0 or cin != cout) if shortcut is None else shortcut
        sd: SD = {}
        for i, c in ((1, ctot), (2, cout)):
            sd[f"{prefix}.norm{i}.weight"] = 1.0 + torch.randn(c, generator=g) * 0.1
            sd[f"{prefix}.norm{i}.bias"] = torch.randn(c, generator=g) * 0.1
        sd[f"{prefix}.conv1.weight"] = torch.randn(cout, ctot, 3, 3, generator=g) / math.sqrt(9 * ctot)
        sd[f"{prefix}.conv1.bias"] = torch.randn(cout, generator=g) * 0.1
        sd[f"{prefix}.time_emb_proj.weight"] = torch.randn(cout, time_embed_dim, generator=g) / math.sqrt(time_embed_dim)
        sd[f"{prefix}.time_emb_proj.bias"] = torch.randn(cout, generator=g) * 0.1
        sd[f"{prefix}.conv2.weight"] = torch.randn(cout, cout, 3, 3, generator=g) / math.sqrt(9 * cout)
        sd[f"{prefix}.conv2.bias"] = torch.randn(cout, generator=g) * 0.1
        if shortcut:
            sd[f"{prefix}.conv_shortcut.weight"] = torch.randn(cout, ctot, 1, 1, generator=g) / math.sqrt(ctot)
            sd[f"{prefix}.conv_shortcut.bias"] = torch.randn(cout, generator=g) * 0.1
        return cls(sd, prefix, cin, cout, skip, groups, eps)

    def frozen_state_dict(self) -> SD:
        """The frozen fp32 weights under their upstream keys (host copies): what from_state_dict takes."""
        return {f"{self.prefix}.{k}": v.detach().cpu() for k, v in self.host.items()}

    def to(self, device, dtype: torch.dtype = torch.float16) -> "TrainResnetBlock":
        self._bind(device, dtype, "TrainResnetBlock")
        dev, h = self.device, self.host
        self.vec = {k: h[k].to(dev) for k in ("norm1.weight", "norm1.bias", "norm2.weight", "norm2.bias", "conv1.bias", "time_emb_proj.weight",
                                                "time_emb_proj.bias")}
        # forward: conv1 over the normalised dense x | skip; conv2 with the 1x1 shortcut over the raw inputs as further K segments
        self.w1 = self._pack_conv(h["conv1.weight"])
        w2, b2 = self._pack_conv(h["conv2.weight"]), h["conv2.bias"]
        # backward: the flipped-and-swapped 3x3 weights through the same packer, and the transposed shortcut
        self.w1_bwd = self._pack_conv(h["conv1.weight"].flip(2, 3).transpose(0, 1).contiguous())
        self.w2_bwd = self._pack_conv(h["conv2.weight"].flip(2, 3).transpose(0, 1).contiguous())
        if self.has_shortcut:
            ws = h["conv_shortcut.weight"]
            segs = [ws[:, :self.cin]] + ([ws[:, self.cin:]] if self.skip else [])
            w2 = torch.cat([w2] + [self._pack_conv(s.contiguous()) for s in segs], dim=1).contiguous()
            b2 = b2 + h["conv_shortcut.bias"]
            self.ws_bwd = self._pack_conv(ws.transpose(0, 1).contiguous())              # [cin + skip][cout]
        self.w2, self.b2 = w2, b2.to(dev)
        return self

    # ---- forward and backward -------------------------------------------------------------------------------------------------------
    def _check_inputs(self, x, temb, skip):
        who = "TrainResnetBlock"
        if self.device is None:
            raise L.IdbError(f"{who}: call .to('cuda:0') first (there is no CPU fallback)")
        if x.dim() != 4 or x.shape[-1] != self.cin or x.dtype != self.dtype or x.device != self.device:
            raise ValueError(f"{who}: x must be NHWC [batch][h][w][{self.cin}] {self.dtype} on {self.device}")
        if (skip is None) != (self.skip == 0):
            raise ValueError(f"{who}: the block takes {'no' if self.skip == 0 else 'a'} skip input")
        if skip is not None and (skip.shape != x.shape[:3] + (self.skip,) or skip.dtype != self.dtype or skip.device != self.device):
            raise ValueError(f"{who}: skip must be NHWC [batch][h][w][{self.skip}] {self.dtype} on {self.device}")
        if tuple(temb.shape) != (x.shape[0], self.time_embed_dim) or temb.dtype != torch.float32 or temb.device != self.device:
            raise ValueError(f"{who}: temb must be fp32 [batch][{self.time_embed_dim}] on {self.device}")

    def __call__(self, x: torch.Tensor, temb: torch.Tensor, skip: Optional[torch.Tensor] = None) -> ResnetOut:
        self._check_inputs(x, temb, skip)
        x, temb = x.contiguous(), temb.contiguous()
        skip = None if skip is None else skip.contiguous()
        b, h, w_, _ = x.shape
        hw, v, G = h * w_, self.vec, self.groups
        ctot = self.cin + self.skip
        stats1 = self._gn_stats(x, self.cin, skip, self.skip, b, hw, G)
        h0 = self._gn(x, self.cin, skip, self.skip, b, hw, G, self.eps, v["norm1.weight"], v["norm1.bias"], True)
        tb = torch.empty((b, self.cout), dtype=torch.float32, device=self.device)
        L.check(self.lib.idb_linear_f32(temb.data_ptr(), v["time_emb_proj.weight"].data_ptr(), v["time_emb_proj.bias"].data_ptr(), tb.data_ptr(), b,
                                        self.cout, self.time_embed_dim, 1, self._stream()), "idb_linear_f32")
        c1 = self._gemm([(h0, ctot, 9)], self.w1, self.cout, b, h, w_, bias=v["conv1.bias"], sample_bias=tb, sample_bias_ld=self.cout)
        stats2 = self._gn_stats(c1, self.cout, None, 0, b, hw, G)
        h1 = self._gn(c1, self.cout, None, 0, b, hw, G, self.eps, v["norm2.weight"], v["norm2.bias"], True)
        if self.has_shortcut:
            sc = [(x, self.cin, 1)] + ([(skip, self.skip, 1)] if skip is not None else [])
            out = self._gemm([(h1, self.cout, 9)] + sc, self.w2, self.cout, b, h, w_, bias=self.b2)
        else:
            out = self._gemm([(h1, self.cout, 9)], self.w2, self.cout, b, h, w_, bias=self.b2, residual=x)
        return ResnetOut(out.view(b, h, w_, self.cout), x, skip, stats1, c1, stats2)

    def backward(self, out: ResnetOut, grad_out: torch.Tensor) -> ResnetGrad:
        if grad_out.shape != out.out.shape or grad_out.dtype != self.dtype or grad_out.device != self.device:
            raise ValueError("TrainResnetBlock.backward: grad_out must match the output's shape, dtype and device")
        g = grad_out.contiguous()
        b, h, w_, _ = out.x.shape
        hw, v, G = h * w_, self.vec, self.groups
        ctot = self.cin + self.skip
        dsc = self._gemm([(g, self.cout, 1)], self.ws_bwd, ctot, b, h, w_) if self.has_shortcut else g
        dh1 = self._gemm([(g, self.cout, 9)], self.w2_bwd, self.cout, b, h, w_)
        dc1, _ = self._gn_bwd(out.conv1, self.cout, None, 0, out.stats2, dh1, None, b, hw, G, self.eps, v["norm2.weight"], v["norm2.bias"], True)
        dh0 = self._gemm([(dc1, self.cout, 9)], self.w1_bwd, ctot, b, h, w_)
        dx, dskip = self._gn_bwd(out.x, self.cin, out.skip, self.skip, out.stats1, dh0, dsc, b, hw, G, self.eps, v["norm1.weight"], v["norm1.bias"], True)
        return ResnetGrad(dx.view(b, h, w_, self.cin), None if dskip is None else dskip.view(b, h, w_, self.skip))


# ---- Transformer2DModel -----------------------------------------------------------------------------------------------------------------
@dataclass
class Transformer2DOut:
    out: torch.Tensor                          # [b][h][w][c]
    x: torch.Tensor                            # [b][h][w][c]
    stats: Tuple[torch.Tensor, int]            # the norm's statistics partials of x
    blocks: List[BlockOut]


@dataclass
class Transformer2DGrad:
    adapters: SD                               # 16 adapter gradients per block, fp32, by upstream key
    input: torch.Tensor                        # [b][h][w][c]
    context: Optional[torch.Tensor]            # [b][n_kv][context_dim] when asked for (summed over the blocks)


class LoRATransformer2D(_Device):
    def __init__(self, sd: SD, prefix: str, channels: int, context_dim: int, depth: int = 1, rank: int = 4, alpha: Optional[float] = None,
                 groups: int = 32, eps: float = 1e-6):
        who = "LoRATransformer2D"
        if channels <= 0 or channels % 64:
            raise ValueError(f"{who}: channels must be a positive multiple of 64, got {channels}")
        if depth < 1:
            raise ValueError(f"{who}: depth must be at least 1, got {depth}")
        _check_groups(who, channels, groups)
        for k in ("norm.weight", "norm.bias", "proj_in.weight", "proj_in.bias", "proj_out.weight", "proj_out.bias"):
            if f"{prefix}.{k}" not in sd:
                raise KeyError(f"{who}: the state dict has no {prefix}.{k}")
        self.prefix, self.channels, self.context_dim, self.depth, self.rank, self.groups, self.eps = prefix, channels, context_dim, depth, rank, groups, float(eps)
        self.host: SD = {"norm.weight": _vec(sd, f"{prefix}.norm.weight", channels, who), "norm.bias": _vec(sd, f"{prefix}.norm.bias", channels, who)}
        for p in ("proj_in", "proj_out"):
            w = sd[f"{prefix}.{p}.weight"].detach().float()
            if tuple(w.shape) not in ((channels, channels), (channels, channels, 1, 1)):
                raise ValueError(f"{who}: {prefix}.{p}.weight is {tuple(w.shape)}, expected ({channels}, {channels}) (or its 1x1 conv form)")
            self.host[f"{p}.weight"] = w.reshape(channels, channels).contiguous()         # a 1x1 convolution is the same matrix
            self.host[f"{p}.bias"] = _vec(sd, f"{prefix}.{p}.bias", channels, who)
        self.blocks = [LoRATransformerBlock(sd, f"{prefix}.transformer_blocks.{i}", channels, context_dim, rank, alpha) for i in range(depth)]

    # ---- construction -------------------------------------------------------------------------------------------------------------
    @property
    def layers(self):
        return tuple(a for blk in self.blocks for a in blk.layers)

    @classmethod
    def from_state_dict(cls, sd: SD, prefix: str, lora: Optional[SD] = None, alpha: Optional[float] = None, groups: int = 32,
                        eps: float = 1e-6) -> "LoRATransformer2D":
        c = sd[f"{prefix}.proj_in.weight"].shape[0]
        depth = 0
        while f"{prefix}.transformer_blocks.{depth}.attn1.to_q.weight" in sd:
            depth += 1
        kdim = sd[f"{prefix}.transformer_blocks.0.attn2.to_k.weight"].shape[1]
        rank = 4 if lora is None else lora[f"{prefix}.transformer_blocks.0.attn1.to_q.lora_A.weight"].shape[0]
        model = cls(sd, prefix, c, kdim, depth, rank, alpha, groups, eps)
        if lora is not None:
            model.load_adapters(lora)
        return model

    @classmethod
    def from_synthetic(cls, seed: int, channels: int = 128, context_dim: int = 128, depth: int = 1, rank: int = 4, alpha: Optional[float] = None,
                       groups: int = 32, eps: float = 1e-6, prefix: str = "mid_block.attentions.0") -> "LoRATransformer2D":
        g = torch.Generator().manual_seed(seed)
        sd: SD = {f"{prefix}.norm.weight": 1.0 + torch.randn(channels, generator=g) * 0.1, f"{prefix}.norm.bias": torch.randn(channels, generator=g) * 0.1}
        for p in ("proj_in", "proj_out"):
            sd[f"{prefix}.{p}.weight"] = torch.randn(channels, channels, generator=g) / math.sqrt(channels)
            sd[f"{prefix}.{p}.bias"] = torch.randn(channels, generator=g) * 0.1
        for i in range(depth):
            bp = f"{prefix}.transformer_blocks.{i}"
            sd.update(LoRATransformerBlock.from_synthetic(seed + 101 * (i + 1), channels, context_dim, rank, alpha, prefix=bp).frozen_state_dict())
        return cls(sd, prefix, channels, context_dim, depth, rank, alpha, groups, eps)

    def frozen_state_dict(self) -> SD:
        sd = {f"{self.prefix}.{k}": v.detach().cpu() for k, v in self.host.items()}
        for blk in self.blocks:
            sd.update(blk.frozen_state_dict())
        return sd

    def init_adapters(self, generator: Optional[torch.Generator] = None) -> "LoRATransformer2D":
        for blk in self.blocks:
            blk.init_adapters(generator)
        return self

    def load_adapters(self, lora: SD) -> "LoRATransformer2D":
        for blk in self.blocks:
            blk.load_adapters(lora)
        return self

    def state_dict(self) -> SD:
        """The adapters under exactly the keys weights.normalize_lora_keys produces (what load_lora_weights takes)."""
        sd: SD = {}
        for blk in self.blocks:
            sd.update(blk.state_dict())
        return sd

    def refresh(self) -> None:
        for blk in self.blocks:
            blk.refresh()

    def to(self, device, dtype: torch.dtype = torch.float16) -> "LoRATransformer2D":
        self._bind(device, dtype, "LoRATransformer2D")
        dev, h = self.device, self.host
        for blk in self.blocks:
            blk.to(self.device, dtype)
        self.vec = {k: h[k].to(dev) for k in ("norm.weight", "norm.bias", "proj_in.bias", "proj_out.bias")}
        self.w_in, self.w_out = h["proj_in.weight"].to(dev).to(dtype), h["proj_out.weight"].to(dev).to(dtype)
        self.w_in_t, self.w_out_t = self.w_in.t().contiguous(), self.w_out.t().contiguous()
        return self

    # ---- forward and backward -------------------------------------------------------------------------------------------------------
    def __call__(self, x: torch.Tensor, context: torch.Tensor) -> Transformer2DOut:
        who = "LoRATransformer2D"
        if self.device is None:
            raise L.IdbError(f"{who}: call .to('cuda:0') first (there is no CPU fallback)")
        if x.dim() != 4 or x.shape[-1] != self.channels or x.dtype != self.dtype or x.device != self.device:
            raise ValueError(f"{who}: x must be NHWC [batch][h][w][{self.channels}] {self.dtype} on {self.device}")
        x = x.contiguous()
        b, h, w_, c = x.shape
        hw, v = h * w_, self.vec
        stats = self._gn_stats(x, c, None, 0, b, hw, self.groups)
        hn = self._gn(x, c, None, 0, b, hw, self.groups, self.eps, v["norm.weight"], v["norm.bias"], False)
        t = self._gemm([(hn, c, 1)], self.w_in, c, b, h, w_, bias=v["proj_in.bias"]).view(b, hw, c)
        saved: List[BlockOut] = []
        for blk in self.blocks:
            saved.append(blk(t, context))
            t = saved[-1].out
        out = self._gemm([(t, c, 1)], self.w_out, c, b, h, w_, bias=v["proj_out.bias"], residual=x)      # the residual in the epilogue: one rounding
        return Transformer2DOut(out.view(b, h, w_, c), x, stats, saved)

    def backward(self, out: Transformer2DOut, grad_out: torch.Tensor, need_context_grad: bool = False) -> Transformer2DGrad:
        if grad_out.shape != out.out.shape or grad_out.dtype != self.dtype or grad_out.device != self.device:
            raise ValueError("LoRATransformer2D.backward: grad_out must match the output's shape, dtype and device")
        g = grad_out.contiguous()
        b, h, w_, c = out.x.shape
        hw, v = h * w_, self.vec
        d = self._gemm([(g, c, 1)], self.w_out_t, c, b, h, w_).view(b, hw, c)
        adapters: SD = {}
        dctx = None
        for blk, saved in zip(reversed(self.blocks), reversed(out.blocks)):
            bg = blk.backward(saved, d, need_context_grad)
            adapters.update(bg.adapters)
            d = bg.input
            if need_context_grad:
                dctx = bg.context if dctx is None else dctx + bg.context
        dhn = self._gemm([(d, c, 1)], self.w_in_t, c, b, h, w_)
        dx, _ = self._gn_bwd(out.x, c, None, 0, out.stats, dhn, g, b, hw, self.groups, self.eps, v["norm.weight"], v["norm.bias"], False)
        return Transformer2DGrad(adapters, dx.view(b, h, w_, c), dctx)


# ---- one (resnet, attention) stage and a chain of them ----------------------------------------------------------------------------------
@dataclass
class StageOut:
    out: torch.Tensor
    resnet: ResnetOut
    transformer: Transformer2DOut


@dataclass
class StageGrad:
    adapters: SD
    input: torch.Tensor
    skip: Optional[torch.Tensor]


class LoRAStage:
    def __init__(self, resnet: TrainResnetBlock, transformer: LoRATransformer2D):
        if resnet.cout != transformer.channels:
            raise ValueError(f"LoRAStage: the resnet writes {resnet.cout} channels, the transformer takes {transformer.channels}")
        self.resnet, self.transformer = resnet, transformer

    @property
    def layers(self):
        return self.transformer.layers

    def to(self, device, dtype: torch.dtype = torch.float16) -> "LoRAStage":
        self.resnet.to(device, dtype)
        self.transformer.to(device, dtype)
        return self

    def state_dict(self) -> SD:
        return self.transformer.state_dict()

    def load_adapters(self, lora: SD) -> "LoRAStage":
        self.transformer.load_adapters(lora)
        return self

    def init_adapters(self, generator: Optional[torch.Generator] = None) -> "LoRAStage":
        self.transformer.init_adapters(generator)
        return self

    def refresh(self) -> None:
        self.transformer.refresh()

    def frozen_state_dict(self) -> SD:
        return {**self.resnet.frozen_state_dict(), **self.transformer.frozen_state_dict()}

    def __call__(self, x: torch.Tensor, temb: torch.Tensor, context: torch.Tensor, skip: Optional[torch.Tensor] = None) -> StageOut:
        r = self.resnet(x, temb, skip)
        t = self.transformer(r.out, context)
        return StageOut(t.out, r, t)

    def backward(self, out: StageOut, grad_out: torch.Tensor) -> StageGrad:
        tg = self.transformer.backward(out.transformer, grad_out)
        rg = self.resnet.backward(out.resnet, tg.input)
        return StageGrad(tg.adapters, rg.input, rg.skip)


def train_stage_step(stages: Sequence[LoRAStage], opt: LoRAAdamW, x: torch.Tensor, temb: torch.Tensor, context: torch.Tensor,
                     grad_out: Union[torch.Tensor, Callable[[torch.Tensor], torch.Tensor]], inv_scale: float = 1.0,
                     skips: Optional[Sequence[Optional[torch.Tensor]]] = None) -> Dict[str, object]:
    """Forward through the chain of stages (each feeding the next; `skips[i]` is stage i's skip input), backward through all of them, and
    one optimiser step over the union of their adapter gradients.  `grad_out` is the gradient of the (scaled) loss with respect to the
    last stage's output, or a function that forms it from that output."""
    skips = list(skips) if skips is not None else [None] * len(stages)
    if len(skips) != len(stages) or not stages:
        raise ValueError("train_stage_step: one skip entry (or None) per stage, and at least one stage")
    saved: List[StageOut] = []
    t = x
    for stage, skip in zip(stages, skips):
        saved.append(stage(t, temb, context, skip))
        t = saved[-1].out
    g = grad_out(t) if callable(grad_out) else grad_out
    adapters: SD = {}
    skip_grads: List[Optional[torch.Tensor]] = [None] * len(stages)
    for i in range(len(stages) - 1, -1, -1):
        sg = stages[i].backward(saved[i], g)
        adapters.update(sg.adapters)
        g, skip_grads[i] = sg.input, sg.skip
    norm, skipped = opt.step(adapters, inv_scale)
    return {"out": t, "grad_input": g, "grad_skips": skip_grads, "adapters": adapters, "grad_norm": norm, "skipped": skipped}
