"""One UNet attention module with its LoRA adapters, trainable on the device: the layer every trainable parameter of the reference's
fine-tuning lives in (train_ID-Booth.py:672-678 attaches rank-4 adapters to to_q / to_k / to_v / to_out.0 of every attention module).

``LoRAAttention`` is diffusers' ``Attention`` as SD-2.1's ``BasicTransformerBlock`` uses it (heads = channels / 64, scale 1/8, to_out.0
with a bias, Dropout(0)) with peft ``lora.Linear`` adapters (scaling = alpha / rank).  The forward runs on MERGED weights
(``idb_lora_merge``, rebuilt by ``refresh()`` whenever the adapters change) through ``idb_gemm`` and ``idb_attention_fwd_train``; that is
mathematically peft's unmerged training forward, rounded differently.  The backward is ``idb_attention_bwd``, ``idb_gemm`` with the
transposed merged weights for the input gradients, and ``idb_lora_grad`` for the eight adapter gradients; the out x in weight gradients
are never formed.  The surrounding transformer block (LayerNorm, GEGLU, the residuals) and the optimiser are lorablock.py's; the
backward of GroupNorm, the convolutions and the loss is not built.  There is no CPU fallback."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, Optional

import torch

from . import _lib as L
from ._frtrain import hip_device

NAMES = ("to_q", "to_k", "to_v", "to_out.0")
SD = Dict[str, torch.Tensor]


@dataclass
class AttnOut:
    """The output and what the backward needs: the inputs, the packed projections, the attention output and lse."""
    out: torch.Tensor                  # [b][n][c]
    x: torch.Tensor                    # [b][n][c]
    context: Optional[torch.Tensor]    # [b][n_kv][context_dim], None for self-attention
    q: torch.Tensor                    # self-attention: the packed [b*n][3c] q|k|v buffer; cross-attention: [b*n][c]
    kv: Optional[torch.Tensor]         # cross-attention: [b*n_kv][2c] k|v
    attn: torch.Tensor                 # [b*n][c]
    lse: torch.Tensor                  # [b][heads][n] fp32


@dataclass
class AttnGrad:
    adapters: SD                       # the eight adapter gradients, fp32, by upstream key
    input: torch.Tensor                # [b][n][c]
    context: Optional[torch.Tensor]    # [b][n_kv][context_dim] when asked for


class LoRAAttention:
    def __init__(self, sd: SD, prefix: str, channels: int, context_dim: Optional[int] = None, rank: int = 4, alpha: Optional[float] = None):
        if channels <= 0 or channels % 64:
            raise ValueError(f"LoRAAttention: channels must be a positive multiple of 64 (head dim 64), got {channels}")
        if not 1 <= rank <= L.IDB_LORA_MAX_RANK:
            raise ValueError(f"LoRAAttention: rank must be 1..{L.IDB_LORA_MAX_RANK}, got {rank}")
        if context_dim is not None and (context_dim <= 0 or context_dim % 64):
            raise ValueError(f"LoRAAttention: context_dim must be a positive multiple of 64, got {context_dim}")
        self.prefix, self.channels, self.context_dim, self.rank = prefix, channels, context_dim, rank
        self.alpha = float(rank if alpha is None else alpha)
        self.scaling = self.alpha / rank
        self.heads = channels // 64
        kdim = context_dim or channels
        shapes = {"to_q": (channels, channels), "to_k": (channels, kdim), "to_v": (channels, kdim), "to_out.0": (channels, channels)}
        self.base: SD = {}
        for n, shp in shapes.items():
            w = sd[f"{prefix}.{n}.weight"]
            if tuple(w.shape) != shp:
                raise ValueError(f"LoRAAttention: {prefix}.{n}.weight is {tuple(w.shape)}, expected {shp}")
            self.base[n] = w.detach().float().contiguous()
        self.bias = sd[f"{prefix}.to_out.0.bias"].detach().float().contiguous()
        self.shapes = shapes
        self.lora: SD = {}
        for n, (o, i) in shapes.items():
            self.lora[f"{n}.lora_A"] = torch.zeros(rank, i)
            self.lora[f"{n}.lora_B"] = torch.zeros(o, rank)
        self.device: Optional[torch.device] = None
        self.dtype = torch.float16

    # ---- construction -------------------------------------------------------------------------------------------------------------
    @classmethod
    def from_state_dict(cls, sd: SD, prefix: str, lora: Optional[SD] = None, alpha: Optional[float] = None,
                        cross: Optional[bool] = None) -> "LoRAAttention":
        """Sizes from the weights' shapes; `lora` (normalized keys, weights.normalize_lora_keys) sets the rank and the adapters.  `cross`
        says whether the layer attends a context; None reads it off the module name (attn2) or a to_k wider or narrower than to_q."""
        c = sd[f"{prefix}.to_q.weight"].shape[0]
        kdim = sd[f"{prefix}.to_k.weight"].shape[1]
        if cross is None:
            cross = prefix.endswith("attn2") or kdim != c
        rank = 4 if lora is None else lora[f"{prefix}.to_q.lora_A.weight"].shape[0]
        layer = cls(sd, prefix, c, kdim if cross else None, rank, alpha)
        if lora is not None:
            layer.load_adapters(lora)
        return layer

    @classmethod
    def from_synthetic(cls, seed: int, channels: int = 128, context_dim: Optional[int] = None, rank: int = 4, alpha: Optional[float] = None,
                       prefix: str = "mid_block.attentions.0.transformer_blocks.0.attn1") -> "LoRAAttention":
        g = torch.Generator().manual_seed(seed)
        kdim = context_dim or channels
        sd = {f"{prefix}.{n}.weight": torch.randn(channels, kdim if n in ("to_k", "to_v") else channels, generator=g) / math.sqrt(channels)
              for n in NAMES}
        sd[f"{prefix}.to_out.0.bias"] = torch.randn(channels, generator=g) * 0.1
        return cls(sd, prefix, channels, context_dim, rank, alpha)

    def init_adapters(self, generator: Optional[torch.Generator] = None) -> "LoRAAttention":
        """Upstream's init_lora_weights="gaussian": A ~ N(0, 1 / rank) (std 1 / rank), B = 0."""
        for n, (o, i) in self.shapes.items():
            self.lora[f"{n}.lora_A"] = torch.randn(self.rank, i, generator=generator) / self.rank
            self.lora[f"{n}.lora_B"] = torch.zeros(o, self.rank)
        return self._adapters_changed()

    def load_adapters(self, lora: SD) -> "LoRAAttention":
        for n, (o, i) in self.shapes.items():
            a, b = lora[f"{self.prefix}.{n}.lora_A.weight"], lora[f"{self.prefix}.{n}.lora_B.weight"]
            if tuple(a.shape) != (self.rank, i) or tuple(b.shape) != (o, self.rank):
                raise ValueError(f"LoRAAttention: adapter of {self.prefix}.{n} is {tuple(a.shape)} / {tuple(b.shape)}, expected rank {self.rank}")
            self.lora[f"{n}.lora_A"], self.lora[f"{n}.lora_B"] = a.detach().float().contiguous(), b.detach().float().contiguous()
        return self._adapters_changed()

    def state_dict(self) -> SD:
        """The adapters under exactly the keys weights.normalize_lora_keys produces (what load_lora_weights takes)."""
        return {f"{self.prefix}.{n}.lora_{ab}.weight": self.lora[f"{n}.lora_{ab}"].detach().cpu().clone() for n in NAMES for ab in "AB"}

    def to(self, device, dtype: torch.dtype = torch.float16) -> "LoRAAttention":
        if dtype not in (torch.float16, torch.bfloat16):
            raise ValueError("LoRAAttention: operand dtype must be float16 or bfloat16")
        self.device, self.dtype = hip_device(device, "LoRAAttention"), dtype
        self.lib = L.load()
        self.dt = L.IDB_F16 if dtype == torch.float16 else L.IDB_BF16
        dev = self.device
        self.base = {n: w.to(dev) for n, w in self.base.items()}
        self.base_t = {n: w.t().contiguous() for n, w in self.base.items()}
        self.bias = self.bias.to(dev)
        c, kdim = self.channels, self.context_dim or self.channels
        # the merged operand-dtype matrices idb_gemm reads: forward rows stacked [q;k;v] (self) or q and [k;v] (cross), to_out, and
        # their transposes with the output channels of q|k|v side by side along K
        self.w_fwd = {"qkv" if self.context_dim is None else "q": torch.empty((3 * c if self.context_dim is None else c, c), dtype=dtype, device=dev),
                      "out": torch.empty((c, c), dtype=dtype, device=dev)}
        self.w_bwd = {"out": torch.empty((c, c), dtype=dtype, device=dev)}
        if self.context_dim is None:
            self.w_bwd["qkv"] = torch.empty((c, 3 * c), dtype=dtype, device=dev)
        else:
            self.w_fwd["kv"] = torch.empty((2 * c, kdim), dtype=dtype, device=dev)
            self.w_bwd["q"] = torch.empty((c, c), dtype=dtype, device=dev)
            self.w_bwd["kv"] = torch.empty((kdim, 2 * c), dtype=dtype, device=dev)
        self._ws = torch.empty(0, dtype=torch.uint8, device=dev)
        return self._adapters_changed()

    def _adapters_changed(self) -> "LoRAAttention":
        if self.device is not None:
            self.lora = {k: v.to(self.device) for k, v in self.lora.items()}
            self.refresh()
        return self

    # ---- device plumbing ------------------------------------------------------------------------------------------------------------
    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def _workspace(self, nbytes: int) -> torch.Tensor:
        if self._ws.numel() < nbytes:
            self._ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        return self._ws

    def _merge(self, w, a, b, dst: torch.Tensor) -> None:
        rows, cols = w.shape
        L.check(self.lib.idb_lora_merge(w.data_ptr(), a.data_ptr(), b.data_ptr(), dst.data_ptr(), rows, cols, self.rank, self.scaling, self.dt,
                                        self._stream()), "idb_lora_merge")

    def refresh(self) -> None:
        """Rebuild the merged weights from the fp32 masters and the current adapters: W + s B A for the forward, and for the input
        gradients W^T + s A^T B^T, which is idb_lora_merge on W^T with lora_b := A^T and lora_a := B^T."""
        c, dev, dtype = self.channels, self.device, self.dtype
        self_attn = self.context_dim is None
        for j, n in enumerate(NAMES):
            a, b = self.lora[f"{n}.lora_A"], self.lora[f"{n}.lora_B"]
            if n == "to_out.0":
                fwd = self.w_fwd["out"]
            elif self_attn:
                fwd = self.w_fwd["qkv"][j * c:(j + 1) * c]
            else:
                fwd = self.w_fwd["q"] if n == "to_q" else self.w_fwd["kv"][(j - 1) * c:j * c]
            self._merge(self.base[n], a, b, fwd)                      # row slices of a row-major matrix are contiguous
            tmp = torch.empty(self.base_t[n].shape, dtype=dtype, device=dev)
            self._merge(self.base_t[n], b.t().contiguous(), a.t().contiguous(), tmp)
            if n == "to_out.0":
                self.w_bwd["out"].copy_(tmp)
            elif self_attn:
                self.w_bwd["qkv"][:, j * c:(j + 1) * c].copy_(tmp)
            elif n == "to_q":
                self.w_bwd["q"].copy_(tmp)
            else:
                self.w_bwd["kv"][:, (j - 1) * c:j * c].copy_(tmp)

    def _gemm(self, x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None) -> torch.Tensor:
        """out[m][n] = x[m][k] w[n][k]^T (+ bias) (+ residual [m][n], in the epilogue: one rounding) through idb_gemm; x dense."""
        n, k = w.shape
        m = x.numel() // k
        out = torch.empty((m, n), dtype=self.dtype, device=self.device)
        d = L.gemm_desc(self.dt, [(x.data_ptr(), k, 1, 1, 1)], w.data_ptr(), n, m, 1, 1, out=out.data_ptr(),
                        bias=None if bias is None else bias.data_ptr(), residual=None if residual is None else residual.data_ptr())
        L.check(L.run_gemm(self.lib, d, self._workspace, self._stream()), "idb_gemm")
        return out

    def _check_inputs(self, x, context):
        if self.device is None:
            raise L.IdbError("LoRAAttention: call .to('cuda:0') first (there is no CPU fallback)")
        if (context is None) != (self.context_dim is None):
            raise ValueError("LoRAAttention: a self-attention layer takes no context" if self.context_dim is None
                             else "LoRAAttention: a cross-attention layer needs a context")
        if x.dim() != 3 or x.shape[-1] != self.channels or x.dtype != self.dtype or x.device != self.device:
            raise ValueError(f"LoRAAttention: x must be [batch][tokens][{self.channels}] {self.dtype} on {self.device}")
        if context is not None and (context.dim() != 3 or context.shape[0] != x.shape[0] or context.shape[-1] != self.context_dim
                                    or context.dtype != self.dtype or context.device != self.device):
            raise ValueError(f"LoRAAttention: context must be [batch][tokens][{self.context_dim}] {self.dtype} on {self.device}")

    # ---- forward and backward -------------------------------------------------------------------------------------------------------
    def __call__(self, x: torch.Tensor, context: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None) -> AttnOut:
        """`residual` ([batch][tokens][channels], the block's residual stream) is added in the to_out GEMM's epilogue: `out` is then the
        sum, rounded once.  The backward is unchanged: the gradient of the sum is the gradient of the module's own output."""
        self._check_inputs(x, context)
        if residual is not None:
            if residual.shape != x.shape or residual.dtype != self.dtype or residual.device != self.device:
                raise ValueError("LoRAAttention: residual must match x's shape, dtype and device")
            residual = residual.contiguous()
        x = x.contiguous()
        b, n, c = x.shape
        h, es = self.heads, 2
        if context is None:
            q, kv, n_kv = self._gemm(x, self.w_fwd["qkv"]), None, n
            qp, kp, vp, q_ld, kv_ld = q.data_ptr(), q.data_ptr() + c * es, q.data_ptr() + 2 * c * es, 3 * c, 3 * c
        else:
            context = context.contiguous()
            n_kv = context.shape[1]
            q, kv = self._gemm(x, self.w_fwd["q"]), self._gemm(context, self.w_fwd["kv"])
            qp, kp, vp, q_ld, kv_ld = q.data_ptr(), kv.data_ptr(), kv.data_ptr() + c * es, c, 2 * c
        attn = torch.empty((b * n, c), dtype=self.dtype, device=self.device)
        lse = torch.empty((b, h, n), dtype=torch.float32, device=self.device)
        L.check(self.lib.idb_attention_fwd_train(qp, q_ld, kp, vp, kv_ld, attn.data_ptr(), c, lse.data_ptr(), b, h, n, n_kv, n_kv, 0.125, self.dt,
                                                 self._stream()), "idb_attention_fwd_train")
        out = self._gemm(attn, self.w_fwd["out"], self.bias, residual).view(b, n, c)
        return AttnOut(out, x, context, q, kv, attn, lse)

    def _lora_grad(self, grads: SD, name: str, x: torch.Tensor, dy_ptr: int, dy_ld: int, m: int) -> None:
        o, i = self.shapes[name]
        da = torch.empty((self.rank, i), dtype=torch.float32, device=self.device)
        db = torch.empty((o, self.rank), dtype=torch.float32, device=self.device)
        need = self.lib.idb_lora_grad_workspace_bytes(m, i, o, self.rank)
        L.check(self.lib.idb_lora_grad(x.data_ptr(), i, dy_ptr, dy_ld, self.lora[f"{name}.lora_A"].data_ptr(), self.lora[f"{name}.lora_B"].data_ptr(),
                                       da.data_ptr(), db.data_ptr(), m, i, o, self.rank, self.scaling, self._workspace(need).data_ptr(), need, self.dt,
                                       self._stream()), "idb_lora_grad")
        grads[f"{self.prefix}.{name}.lora_A.weight"], grads[f"{self.prefix}.{name}.lora_B.weight"] = da, db

    def backward(self, out: AttnOut, grad_out: torch.Tensor, need_context_grad: bool = False) -> AttnGrad:
        b, n, c = out.x.shape
        if grad_out.shape != out.out.shape or grad_out.dtype != self.dtype or grad_out.device != self.device:
            raise ValueError("LoRAAttention.backward: grad_out must match the output's shape, dtype and device")
        if need_context_grad and out.context is None:
            raise ValueError("LoRAAttention.backward: a self-attention layer has no context gradient")
        g = grad_out.contiguous().view(b * n, c)
        h, es = self.heads, 2
        grads: SD = {}
        dattn = self._gemm(g, self.w_bwd["out"])
        self._lora_grad(grads, "to_out.0", out.attn, g.data_ptr(), c, b * n)
        if out.context is None:
            n_kv = n
            dqkv = torch.empty((b * n, 3 * c), dtype=self.dtype, device=self.device)
            qp, kp, vp, q_ld, kv_ld = out.q.data_ptr(), out.q.data_ptr() + c * es, out.q.data_ptr() + 2 * c * es, 3 * c, 3 * c
            dqp, dkp, dvp, dq_ld, dkv_ld = dqkv.data_ptr(), dqkv.data_ptr() + c * es, dqkv.data_ptr() + 2 * c * es, 3 * c, 3 * c
        else:
            n_kv = out.context.shape[1]
            dq = torch.empty((b * n, c), dtype=self.dtype, device=self.device)
            dkv = torch.empty((b * n_kv, 2 * c), dtype=self.dtype, device=self.device)
            qp, kp, vp, q_ld, kv_ld = out.q.data_ptr(), out.kv.data_ptr(), out.kv.data_ptr() + c * es, c, 2 * c
            dqp, dkp, dvp, dq_ld, dkv_ld = dq.data_ptr(), dkv.data_ptr(), dkv.data_ptr() + c * es, c, 2 * c
        need = self.lib.idb_attention_bwd_workspace_bytes(b, h, n, n_kv)
        L.check(self.lib.idb_attention_bwd(qp, q_ld, kp, vp, kv_ld, out.attn.data_ptr(), c, dattn.data_ptr(), c, out.lse.data_ptr(), dqp, dq_ld, dkp, dvp,
                                           dkv_ld, self._workspace(need).data_ptr(), need, b, h, n, n_kv, n_kv, 0.125, self.dt, self._stream()),
                "idb_attention_bwd")
        src = out.x if out.context is None else out.context
        self._lora_grad(grads, "to_q", out.x, dqp, dq_ld, b * n)
        self._lora_grad(grads, "to_k", src, dkp, dkv_ld, b * n_kv)
        self._lora_grad(grads, "to_v", src, dvp, dkv_ld, b * n_kv)
        if out.context is None:
            return AttnGrad(grads, self._gemm(dqkv, self.w_bwd["qkv"]).view(b, n, c), None)
        dctx = self._gemm(dkv, self.w_bwd["kv"]).view(b, n_kv, self.context_dim) if need_context_grad else None
        return AttnGrad(grads, self._gemm(dq, self.w_bwd["q"]).view(b, n, c), dctx)
