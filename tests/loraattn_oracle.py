"""A float64 restatement of faceposegenerator_amd.loraattn.LoRAAttention: diffusers' Attention as SD-2.1's BasicTransformerBlock uses it
(heads = channels / 64, scale 1/8, to_out.0 with a bias, Dropout(0)) with peft lora.Linear adapters on to_q / to_k / to_v / to_out.0,
forward and backward in CLOSED FORM: lse, dQ, dK, dV, the eight adapter gradients, the input and context gradients.

Pinned on the CPU (tests/test_loraattn_cpu.py) against torch autograd in float64 through `autograd_layer`, a plain restatement with
F.scaled_dot_product_attention and UNMERGED adapters (W x + s B (A x)), to 1e-12 relative.  diffusers and peft are not installed where
this project is built, so parity with their binaries is UNPINNED: the restatement follows their published source (Attention.forward with
AttnProcessor2_0; peft.tuners.lora.Linear.forward: result + lora_B(lora_A(dropout(x))) * scaling, scaling = alpha / r).

`rt` is the rounding hook: identity gives the exact oracle; round-to-operand-dtype gives the yardstick of the layer-level tolerance, the
oracle with a rounding at every point where the engine stores a 16-bit tensor and nothing else: the merged weights, q / k / v, P (for
P V and P^T dO), the attention output, the gradient of the attention output (the to_out GEMM stores it), dS, dq / dk / dv, the layer
output and the returned input / context gradients."""
from typing import Callable, Dict, Optional

import torch
import torch.nn.functional as F

NAMES = ("to_q", "to_k", "to_v", "to_out.0")
F64 = torch.float64


def _heads(x, h):
    b, n, _ = x.shape
    return x.reshape(b, n, h, 64).permute(0, 2, 1, 3)


def _rows(x):
    b, h, n, _ = x.shape
    return x.permute(0, 2, 1, 3).reshape(b, n, h * 64)


def run(sd: Dict[str, torch.Tensor], prefix: str, lora: Dict[str, torch.Tensor], scaling: float, x, context, grad_out,
        rt: Optional[Callable] = None) -> Dict[str, torch.Tensor]:
    """Forward and backward.  sd: `<prefix>.to_q.weight` ... `<prefix>.to_out.0.bias`; lora: `<prefix>.<name>.lora_A/lora_B.weight`;
    x [b][n][c]; context [b][n_kv][context_dim] or None (self-attention); grad_out like the output.  Returns `out`, `lse`, `input`,
    `context` (None for self-attention) and the eight adapter gradients by key."""
    rt = rt or (lambda t: t)
    d = lambda t: t.to(F64)
    x, g = d(x), d(grad_out)
    ctx = x if context is None else d(context)
    c = x.shape[-1]
    h = c // 64
    A = {n: d(lora[f"{prefix}.{n}.lora_A.weight"]) for n in NAMES}
    B = {n: d(lora[f"{prefix}.{n}.lora_B.weight"]) for n in NAMES}
    Wm = {n: rt(d(sd[f"{prefix}.{n}.weight"]) + scaling * B[n] @ A[n]) for n in NAMES}
    q, k, v = rt(x @ Wm["to_q"].T), rt(ctx @ Wm["to_k"].T), rt(ctx @ Wm["to_v"].T)
    qh, kh, vh = _heads(q, h), _heads(k, h), _heads(v, h)
    s = 0.125 * qh @ kh.transpose(-1, -2)
    lse = torch.logsumexp(s, -1)
    p = torch.exp(s - lse[..., None])
    pr = rt(p)
    oh = rt(pr @ vh)
    o = _rows(oh)
    out = rt(o @ Wm["to_out.0"].T + d(sd[f"{prefix}.to_out.0.bias"]))
    # backward
    do = rt(g @ Wm["to_out.0"])
    doh = _heads(do, h)
    delta = (doh * oh).sum(-1, keepdim=True)
    ds = rt(p * (doh @ vh.transpose(-1, -2) - delta))
    dq, dk, dv = _rows(rt(0.125 * ds @ kh)), _rows(rt(0.125 * ds.transpose(-1, -2) @ qh)), _rows(rt(pr.transpose(-1, -2) @ doh))
    res = {"out": out, "lse": lse}

    def adapter(name, xin, dy):
        x2, dy2 = xin.reshape(-1, xin.shape[-1]), dy.reshape(-1, dy.shape[-1])
        res[f"{prefix}.{name}.lora_B.weight"] = scaling * dy2.T @ (x2 @ A[name].T)
        res[f"{prefix}.{name}.lora_A.weight"] = scaling * (dy2 @ B[name]).T @ x2

    adapter("to_out.0", o, g)
    adapter("to_q", x, dq)
    adapter("to_k", ctx, dk)
    adapter("to_v", ctx, dv)
    dctx = dk @ Wm["to_k"] + dv @ Wm["to_v"]
    if context is None:
        res["input"], res["context"] = rt(dq @ Wm["to_q"] + dctx), None
    else:
        res["input"], res["context"] = rt(dq @ Wm["to_q"]), rt(dctx)
    return res


def autograd_layer(sd, prefix, lora, scaling, x, context, grad_out) -> Dict[str, torch.Tensor]:
    """The same quantities from torch autograd in float64: unmerged adapters and F.scaled_dot_product_attention."""
    d = lambda t: t.to(F64)
    x = d(x).clone().requires_grad_(True)
    ctx = None if context is None else d(context).clone().requires_grad_(True)
    par = {f"{prefix}.{n}.lora_{ab}.weight": d(lora[f"{prefix}.{n}.lora_{ab}.weight"]).clone().requires_grad_(True) for n in NAMES for ab in "AB"}

    def lin(name, t, bias=None):
        a, b = par[f"{prefix}.{name}.lora_A.weight"], par[f"{prefix}.{name}.lora_B.weight"]
        return F.linear(t, d(sd[f"{prefix}.{name}.weight"]), bias) + F.linear(F.linear(t, a), b) * scaling

    src = x if ctx is None else ctx
    h = x.shape[-1] // 64
    q, k, v = _heads(lin("to_q", x), h), _heads(lin("to_k", src), h), _heads(lin("to_v", src), h)
    o = _rows(F.scaled_dot_product_attention(q, k, v, scale=0.125))
    out = lin("to_out.0", o, d(sd[f"{prefix}.to_out.0.bias"]))
    (out * d(grad_out)).sum().backward()
    res = {"out": out.detach(), "input": x.grad, "context": None if ctx is None else ctx.grad}
    res["lse"] = torch.logsumexp(0.125 * q.detach() @ k.detach().transpose(-1, -2), -1)
    res.update({k_: v_.grad for k_, v_ in par.items()})
    return res


def deviation(got: torch.Tensor, exact: torch.Tensor) -> float:
    """The layer-level figure: the largest absolute deviation from the exact oracle over the tensor's largest magnitude."""
    return float((got.to(F64) - exact).abs().max() / exact.abs().max().clamp(min=1e-300))
