"""One UNet transformer block with LoRA adapters on its two attention modules, trainable on the device, and the optimiser the
reference steps them with (train_ID-Booth.py:672-678 attaches the adapters, :796-810 builds torch.optim.AdamW, :1140-1146 clips the
gradient norm to 1.0 and steps under fp16 mixed precision).

``LoRATransformerBlock`` is diffusers' ``BasicTransformerBlock`` in SD-2.1's form: LayerNorm -> self-attention -> residual, LayerNorm ->
cross-attention -> residual, LayerNorm -> GEGLU feed-forward -> residual, Dropout(0).  Only the 16 adapter tensors of ``attn1`` and
``attn2`` (``loraattn.LoRAAttention``) train: LayerNorm's affine and the feed-forward weights are frozen upstream, so the backward forms
no gradient for them.  The forward is ``idb_layernorm``, the attention layers, ``idb_gemm`` (residuals in its epilogue) and
``idb_geglu_fwd`` on the projection's stored output; the backward is ``idb_gemm`` with the transposed feed-forward weights,
``idb_geglu_bwd``, ``idb_layernorm_bwd`` (which adds the residual stream's gradient) and the attention layers' backward.  The residual
stream and its gradient stay in the operand dtype, rounded once per stage; a GradScaler's factor on ``grad_out`` passes through
linearly to every gradient.

``LoRAAdamW`` is ``GradScaler.unscale_`` + ``clip_grad_norm_`` + ``torch.optim.AdamW.step`` on the fp32 adapter masters as one library
call (``idb_adamw_clip_step_table``), ``cosine_lr`` the reference's schedule.  The convolutions and GroupNorms between the UNet's blocks
have their backward in lorastage.py.  There is no CPU fallback."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Callable, Dict, Iterable, List, Optional, Tuple, Union

import torch

from . import _lib as L
from ._frtrain import hip_device
from .loraattn import NAMES, AttnOut, LoRAAttention

SD = Dict[str, torch.Tensor]
LN_EPS = 1e-5
_HYPER = ("lr", "beta1", "beta2", "eps", "weight_decay", "max_norm")


@dataclass
class BlockOut:
    """The output and what the backward needs: the three residual-stream tensors, the feed-forward's projection and its GEGLU output,
    and what the two attention layers saved (their `x` are LN1 x and LN2 h1)."""
    out: torch.Tensor                  # [b][n][c]
    x: torch.Tensor                    # [b][n][c]
    context: torch.Tensor              # [b][n_kv][context_dim]
    h1: torch.Tensor                   # x + attn1(LN1 x)
    h2: torch.Tensor                   # h1 + attn2(LN2 h1, context)
    hg: torch.Tensor                   # [b*n][2 inner]: ff.net.0.proj(LN3 h2), value then gate
    act: torch.Tensor                  # [b*n][inner]: value gelu(gate)
    attn1: AttnOut
    attn2: AttnOut


@dataclass
class BlockGrad:
    adapters: SD                       # the 16 adapter gradients, fp32, by upstream key
    input: torch.Tensor                # [b][n][c]
    context: Optional[torch.Tensor]    # [b][n_kv][context_dim] when asked for


class LoRATransformerBlock:
    def __init__(self, sd: SD, prefix: str, channels: int, context_dim: int, rank: int = 4, alpha: Optional[float] = None):
        if channels > 1536:
            raise ValueError(f"LoRATransformerBlock: channels must be at most 1536 (idb_layernorm), got {channels}")
        if context_dim is None:
            raise ValueError("LoRATransformerBlock: context_dim is required (attn2 attends the context)")
        self.prefix, self.channels, self.context_dim, self.rank = prefix, channels, context_dim, rank
        self.attn1 = LoRAAttention(sd, f"{prefix}.attn1", channels, None, rank, alpha)
        self.attn2 = LoRAAttention(sd, f"{prefix}.attn2", channels, context_dim, rank, alpha)
        self.norm: List[Tuple[torch.Tensor, torch.Tensor]] = []
        for i in (1, 2, 3):
            w, b = sd[f"{prefix}.norm{i}.weight"], sd[f"{prefix}.norm{i}.bias"]
            if tuple(w.shape) != (channels,) or tuple(b.shape) != (channels,):
                raise ValueError(f"LoRATransformerBlock: {prefix}.norm{i} is {tuple(w.shape)} / {tuple(b.shape)}, expected ({channels},)")
            self.norm.append((w.detach().float().contiguous(), b.detach().float().contiguous()))
        w1, b1 = sd[f"{prefix}.ff.net.0.proj.weight"], sd[f"{prefix}.ff.net.0.proj.bias"]
        w2, b2 = sd[f"{prefix}.ff.net.2.weight"], sd[f"{prefix}.ff.net.2.bias"]
        inner = w2.shape[1]
        if inner <= 0 or inner % 64 or tuple(w1.shape) != (2 * inner, channels) or tuple(w2.shape) != (channels, inner) \
                or tuple(b1.shape) != (2 * inner,) or tuple(b2.shape) != (channels,):
            raise ValueError(f"LoRATransformerBlock: {prefix}.ff is {tuple(w1.shape)} -> {tuple(w2.shape)}, expected (2 inner, {channels}) -> "
                             f"({channels}, inner) with inner a multiple of 64")
        self.inner = inner
        # plain row order (value rows, then gate rows), not the inference engine's GEGLU-interleaved packing: idb_geglu_bwd needs the
        # projection's output as diffusers chunks it
        self.ff = {"w1": w1.detach().float().contiguous(), "b1": b1.detach().float().contiguous(),
                   "w2": w2.detach().float().contiguous(), "b2": b2.detach().float().contiguous()}
        self.device: Optional[torch.device] = None
        self.dtype = torch.float16

    # ---- construction -------------------------------------------------------------------------------------------------------------
    @property
    def layers(self) -> Tuple[LoRAAttention, LoRAAttention]:
        return self.attn1, self.attn2

    @classmethod
    def from_state_dict(cls, sd: SD, prefix: str, lora: Optional[SD] = None, alpha: Optional[float] = None) -> "LoRATransformerBlock":
        """Sizes from the weights' shapes; `lora` (normalized keys, weights.normalize_lora_keys) sets the rank and the adapters."""
        c = sd[f"{prefix}.attn1.to_q.weight"].shape[0]
        kdim = sd[f"{prefix}.attn2.to_k.weight"].shape[1]
        rank = 4 if lora is None else lora[f"{prefix}.attn1.to_q.lora_A.weight"].shape[0]
        block = cls(sd, prefix, c, kdim, rank, alpha)
        if lora is not None:
            block.load_adapters(lora)
        return block

    @classmethod
    def from_synthetic(cls, seed: int, channels: int = 128, context_dim: int = 128, rank: int = 4, alpha: Optional[float] = None,
                       prefix: str = "mid_block.attentions.0.transformer_blocks.0") -> "LoRATransformerBlock":
        g = torch.Generator().manual_seed(seed)
        inner = 4 * channels
        sd: SD = {}
        for a, kdim in (("attn1", channels), ("attn2", context_dim)):
            for n in NAMES:
                k = kdim if n in ("to_k", "to_v") else channels
                sd[f"{prefix}.{a}.{n}.weight"] = torch.randn(channels, k, generator=g) / math.sqrt(k)
            sd[f"{prefix}.{a}.to_out.0.bias"] = torch.randn(channels, generator=g) * 0.1
        for i in (1, 2, 3):
            sd[f"{prefix}.norm{i}.weight"] = 1.0 + torch.randn(channels, generator=g) * 0.1
            sd[f"{prefix}.norm{i}.bias"] = torch.randn(channels, generator=g) * 0.1
        sd[f"{prefix}.ff.net.0.proj.weight"] = torch.randn(2 * inner, channels, generator=g) / math.sqrt(channels)
        sd[f"{prefix}.ff.net.0.proj.bias"] = torch.randn(2 * inner, generator=g) * 0.1
        sd[f"{prefix}.ff.net.2.weight"] = torch.randn(channels, inner, generator=g) / math.sqrt(inner)
        sd[f"{prefix}.ff.net.2.bias"] = torch.randn(channels, generator=g) * 0.1
        return cls(sd, prefix, channels, context_dim, rank, alpha)

    def frozen_state_dict(self) -> SD:
        """The frozen fp32 weights under their upstream keys (host copies): what from_state_dict takes."""
        sd: SD = {}
        for a in self.layers:
            for n in NAMES:
                sd[f"{a.prefix}.{n}.weight"] = a.base[n].detach().cpu()
            sd[f"{a.prefix}.to_out.0.bias"] = a.bias.detach().cpu()
        for i, (w, b) in enumerate(self.norm, 1):
            sd[f"{self.prefix}.norm{i}.weight"], sd[f"{self.prefix}.norm{i}.bias"] = w.detach().cpu(), b.detach().cpu()
        for key, name in (("w1", "ff.net.0.proj.weight"), ("b1", "ff.net.0.proj.bias"), ("w2", "ff.net.2.weight"), ("b2", "ff.net.2.bias")):
            sd[f"{self.prefix}.{name}"] = self.ff[key].detach().cpu()
        return sd

    def init_adapters(self, generator: Optional[torch.Generator] = None) -> "LoRATransformerBlock":
        for a in self.layers:
            a.init_adapters(generator)
        return self

    def load_adapters(self, lora: SD) -> "LoRATransformerBlock":
        for a in self.layers:
            a.load_adapters(lora)
        return self

    def state_dict(self) -> SD:
        """The 16 adapter tensors under exactly the keys weights.normalize_lora_keys produces (what load_lora_weights takes)."""
        return {**self.attn1.state_dict(), **self.attn2.state_dict()}

    def to(self, device, dtype: torch.dtype = torch.float16) -> "LoRATransformerBlock":
        if dtype not in (torch.float16, torch.bfloat16):
            raise ValueError("LoRATransformerBlock: operand dtype must be float16 or bfloat16")
        self.device, self.dtype = hip_device(device, "LoRATransformerBlock"), dtype
        for a in self.layers:
            a.to(self.device, dtype)
        self.lib, self.dt = self.attn1.lib, self.attn1.dt
        dev = self.device
        self.norm = [(w.to(dev), b.to(dev)) for w, b in self.norm]
        self.ff = {k: v.to(dev) for k, v in self.ff.items()}
        # operand-dtype copies idb_gemm reads, and their transposes for the two input-gradient GEMMs
        self.w1, self.w2 = self.ff["w1"].to(dtype), self.ff["w2"].to(dtype)
        self.w1_t, self.w2_t = self.w1.t().contiguous(), self.w2.t().contiguous()
        return self

    def refresh(self) -> None:
        for a in self.layers:
            a.refresh()

    # ---- device plumbing ------------------------------------------------------------------------------------------------------------
    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def _layernorm(self, x: torch.Tensor, i: int) -> torch.Tensor:
        out = torch.empty_like(x)
        w, b = self.norm[i]
        L.check(self.lib.idb_layernorm(x.data_ptr(), out.data_ptr(), x.numel() // self.channels, self.channels, LN_EPS, w.data_ptr(), b.data_ptr(),
                                       self.dt, self._stream()), "idb_layernorm")
        return out

    def _layernorm_bwd(self, x: torch.Tensor, dy: torch.Tensor, add: Optional[torch.Tensor], i: int) -> torch.Tensor:
        dx = torch.empty_like(x)
        L.check(self.lib.idb_layernorm_bwd(x.data_ptr(), dy.data_ptr(), None if add is None else add.data_ptr(), self.norm[i][0].data_ptr(),
                                           dx.data_ptr(), x.numel() // self.channels, self.channels, LN_EPS, self.dt, self._stream()),
                "idb_layernorm_bwd")
        return dx

    def _check_inputs(self, x, context):
        if self.device is None:
            raise L.IdbError("LoRATransformerBlock: call .to('cuda:0') first (there is no CPU fallback)")
        if context is None:
            raise ValueError("LoRATransformerBlock: the block needs a context (attn2 is a cross-attention layer)")
        self.attn2._check_inputs(x, context)

    # ---- forward and backward -------------------------------------------------------------------------------------------------------
    def __call__(self, x: torch.Tensor, context: torch.Tensor) -> BlockOut:
        self._check_inputs(x, context)
        x, context = x.contiguous(), context.contiguous()
        b, n, c = x.shape
        a1 = self.attn1(self._layernorm(x, 0), None, residual=x)
        h1 = a1.out
        a2 = self.attn2(self._layernorm(h1, 1), context, residual=h1)
        h2 = a2.out
        gemm = self.attn1._gemm
        hg = gemm(self._layernorm(h2, 2), self.w1, self.ff["b1"])
        act = torch.empty((b * n, self.inner), dtype=self.dtype, device=self.device)
        L.check(self.lib.idb_geglu_fwd(hg.data_ptr(), 2 * self.inner, act.data_ptr(), b * n, self.inner, self.dt, self._stream()), "idb_geglu_fwd")
        out = gemm(act, self.w2, self.ff["b2"], h2).view(b, n, c)
        return BlockOut(out, x, context, h1, h2, hg, act, a1, a2)

    def backward(self, out: BlockOut, grad_out: torch.Tensor, need_context_grad: bool = False) -> BlockGrad:
        b, n, c = out.x.shape
        if grad_out.shape != out.out.shape or grad_out.dtype != self.dtype or grad_out.device != self.device:
            raise ValueError("LoRATransformerBlock.backward: grad_out must match the output's shape, dtype and device")
        g = grad_out.contiguous()
        gemm = self.attn1._gemm
        dact = gemm(g, self.w2_t)
        dhg = torch.empty_like(out.hg)
        L.check(self.lib.idb_geglu_bwd(out.hg.data_ptr(), 2 * self.inner, dact.data_ptr(), dhg.data_ptr(), b * n, self.inner, self.dt, self._stream()),
                "idb_geglu_bwd")
        dh2 = self._layernorm_bwd(out.h2, gemm(dhg, self.w1_t), g, 2)                       # the residual carries grad_out past the feed-forward
        g2 = self.attn2.backward(out.attn2, dh2, need_context_grad)
        dh1 = self._layernorm_bwd(out.h1, g2.input, dh2, 1)
        g1 = self.attn1.backward(out.attn1, dh1)
        dx = self._layernorm_bwd(out.x, g1.input, dh1, 0)
        return BlockGrad({**g1.adapters, **g2.adapters}, dx, g2.context)


# ---- the optimiser ----------------------------------------------------------------------------------------------------------------------
def cosine_lr(step: int, total_steps: int, warmup: int = 0) -> float:
    """diffusers' get_cosine_schedule_with_warmup multiplier (half a cosine period after a linear warm-up): the reference's
    lr_scheduler = "cosine"."""
    if step < warmup:
        return float(step) / float(max(1, warmup))
    progress = float(step - warmup) / float(max(1, total_steps - warmup))
    return max(0.0, 0.5 * (1.0 + math.cos(math.pi * progress)))


def _owners(block_or_layers) -> List[LoRAAttention]:
    items = block_or_layers if isinstance(block_or_layers, (list, tuple)) else [block_or_layers]
    out: List[LoRAAttention] = []
    for it in items:
        if not isinstance(it, (LoRATransformerBlock, LoRAAttention)) and hasattr(it, "layers"):      # lorastage's LoRATransformer2D / LoRAStage
            out.extend(it.layers)
            continue
        out.extend(it.layers if isinstance(it, LoRATransformerBlock) else [it])
    if not out or not all(isinstance(a, LoRAAttention) for a in out):
        raise ValueError("LoRAAdamW: takes a LoRATransformerBlock, a LoRAAttention, or a list of them")
    if len({a.prefix for a in out}) != len(out):
        raise ValueError("LoRAAdamW: two layers share a prefix")
    return out


class LoRAAdamW:
    """clip_grad_norm_(max_norm) + torch.optim.AdamW (the reference's configuration as defaults) on the fp32 adapter masters of the given
    layers, in place, as one idb_adamw_clip_step_table call.  `lr` may be reassigned between steps (the scheduler).  The two moment
    buffers exist exactly after the first applied step; `steps` counts applied steps only: a step whose gradient norm is not finite
    changes nothing (GradScaler.step's skip) and the scale's backoff is the caller's."""

    def __init__(self, block_or_layers, lr: float = 1e-4, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2,
                 max_norm: float = 1.0):
        self.owners = _owners(block_or_layers)
        self.lr, self.beta1, self.beta2, self.eps = float(lr), float(betas[0]), float(betas[1]), float(eps)
        self.weight_decay, self.max_norm = float(weight_decay), float(max_norm)
        self._check_hyper()
        self.steps = 0
        self._m: Optional[SD] = None
        self._v: Optional[SD] = None
        self._tables = None

    def _check_hyper(self):
        if not (0.0 <= self.lr <= 1e4 and 0.0 <= self.beta1 < 1.0 and 0.0 <= self.beta2 < 1.0 and 0.0 <= self.eps <= 1.0
                and 0.0 <= self.weight_decay <= 1e4 and 0.0 < self.max_norm <= 1e30):
            raise ValueError("LoRAAdamW: lr in [0, 1e4], betas in [0, 1), eps in [0, 1], weight_decay in [0, 1e4], max_norm in (0, 1e30]")

    def params(self) -> SD:
        """The fp32 masters by upstream key, as the layers hold them now."""
        return {f"{a.prefix}.{n}.lora_{ab}.weight": a.lora[f"{n}.lora_{ab}"] for a in self.owners for n in NAMES for ab in "AB"}

    def state_dict(self) -> Dict[str, object]:
        host = lambda d: None if d is None else {k: v.detach().cpu() for k, v in d.items()}       # noqa: E731
        return {**{k: getattr(self, k) for k in _HYPER}, "steps": self.steps, "exp_avg": host(self._m), "exp_avg_sq": host(self._v)}

    def load_state_dict(self, sd) -> None:
        missing = [k for k in _HYPER + ("steps", "exp_avg", "exp_avg_sq") if k not in sd]
        if missing:
            raise ValueError(f"LoRAAdamW state dict without {missing}")
        steps, m, v = int(sd["steps"]), sd["exp_avg"], sd["exp_avg_sq"]
        if (m is None) != (steps == 0) or (v is None) != (steps == 0):
            raise ValueError("LoRAAdamW state dict: moment buffers exist exactly after the first step")
        new = []
        for buf in (m, v):
            if buf is None:
                new.append(None)
                continue
            par = self.params()
            if set(buf) != set(par) or any(tuple(buf[k].shape) != tuple(par[k].shape) for k in par):
                raise ValueError("LoRAAdamW state dict: moment buffers do not match the adapters' keys and shapes")
            new.append({k: buf[k].detach().float().contiguous().clone() for k in par})
        for k in _HYPER:
            setattr(self, k, float(sd[k]))
        self._check_hyper()
        self.steps, (self._m, self._v), self._tables = steps, new, None

    def _device_tables(self, par: SD, grads: SD, dev):
        """Pointer and numel tables in device memory, rebuilt only when a pointer changed."""
        keys = sorted(par)
        ptrs = tuple(tuple(d[k].data_ptr() for k in keys) for d in (par, grads, self._m, self._v))
        if self._tables is None or self._tables[0] != ptrs:
            host = torch.tensor([list(p) for p in ptrs] + [[par[k].numel() for k in keys]], dtype=torch.int64)
            need = self.lib.idb_adamw_clip_table_workspace_bytes(len(keys))
            self._tables = (ptrs, host.to(dev), torch.empty(need, dtype=torch.uint8, device=dev), torch.zeros(1, dtype=torch.float64, device=dev),
                            torch.zeros(1, dtype=torch.int32, device=dev))
        return self._tables[1:]

    def step(self, grads: SD, inv_scale: float = 1.0) -> Tuple[float, bool]:
        """One step from the fp32 gradients by upstream key (BlockGrad.adapters / AttnGrad.adapters); `inv_scale` is 1 / the GradScaler's
        factor the gradients carry.  Returns (the unscaled gradient norm before clipping, whether the step was skipped)."""
        par = self.params()
        dev = next(iter(par.values())).device
        if dev.type != "cuda":
            raise L.IdbError("LoRAAdamW: the layers are not on a HIP device (call .to('cuda:0') first; there is no CPU fallback)")
        if set(grads) != set(par):
            raise ValueError("LoRAAdamW.step: the gradients' keys are not the adapters'")
        grads = {k: g if g.is_contiguous() else g.contiguous() for k, g in grads.items()}
        for k, p in par.items():
            g = grads[k]
            if g.shape != p.shape or g.dtype != torch.float32 or g.device != dev:
                raise ValueError(f"LoRAAdamW.step: gradient {k} must be fp32 {tuple(p.shape)} on {dev}")
        if not (0.0 < inv_scale <= 1e30):
            raise ValueError("LoRAAdamW.step: inv_scale in (0, 1e30]")
        self._check_hyper()
        self.lib = L.load()
        if self._m is None:
            self._m, self._v = ({k: torch.zeros_like(p) for k, p in par.items()} for _ in range(2))
        else:
            self._m, self._v = ({k: t if t.device == dev else t.to(dev) for k, t in d.items()} for d in (self._m, self._v))
        tab, ws, norm, skipped = self._device_tables(par, grads, dev)
        L.check(self.lib.idb_adamw_clip_step_table(len(par), tab[0].data_ptr(), tab[1].data_ptr(), tab[2].data_ptr(), tab[3].data_ptr(),
                                                   tab[4].data_ptr(), self.lr, self.beta1, self.beta2, self.eps, self.weight_decay, self.max_norm,
                                                   float(inv_scale), self.steps + 1, norm.data_ptr(), skipped.data_ptr(), ws.data_ptr(), ws.numel(),
                                                   torch.cuda.current_stream(dev).cuda_stream), "idb_adamw_clip_step_table")
        skip = bool(skipped.item())
        if skip:
            if self.steps == 0:                # the buffers exist exactly after the first applied step
                self._m = self._v = self._tables = None
        else:
            self.steps += 1
            for a in self.owners:
                a.refresh()
        return float(norm.item()), skip


def train_block_step(block: LoRATransformerBlock, opt: LoRAAdamW, x: torch.Tensor, context: torch.Tensor,
                     grad_out: Union[torch.Tensor, Callable[[torch.Tensor], torch.Tensor]], inv_scale: float = 1.0) -> Dict[str, object]:
    """Forward, backward and one optimiser step of one block.  `grad_out` is the gradient of the (scaled) loss with respect to the block's
    output, or a function that forms it from that output."""
    fwd = block(x, context)
    go = grad_out(fwd.out) if callable(grad_out) else grad_out
    g = block.backward(fwd, go)
    norm, skipped = opt.step(g.adapters, inv_scale)
    return {"out": fwd.out, "grad_input": g.input, "grad_norm": norm, "skipped": skipped}
