"""A float64 restatement of faceposegenerator_amd.lorablock.LoRATransformerBlock: diffusers' BasicTransformerBlock in SD-2.1's form
(LayerNorm -> self-attention -> residual, LayerNorm -> cross-attention -> residual, LayerNorm -> GEGLU feed-forward -> residual; Dropout(0))
with peft lora.Linear adapters on to_q / to_k / to_v / to_out.0 of both attention modules, forward and backward in CLOSED FORM: the
output, the input and context gradients and the 16 adapter gradients.  LayerNorm's affine and the feed-forward weights are frozen
upstream and get no gradient here.  The attention modules are loraattn_oracle.run's formulas, restated in two halves (the backward of a
block needs the later stages' gradient first) and with the residual inside the to_out rounding, as the engine's GEMM epilogue adds it.

Pinned on the CPU (tests/test_lorablock_cpu.py) against torch autograd in float64 through `autograd_block` (F.layer_norm, F.linear,
F.gelu, UNMERGED adapters, F.scaled_dot_product_attention) to 1e-12 relative.  diffusers and peft are not installed where this project
is built, so parity with their binaries is UNPINNED: the restatement follows their published source (BasicTransformerBlock.forward,
GEGLU.forward: hidden, gate = proj(x).chunk(2, -1); hidden * gelu(gate)).

`rt` is the rounding hook: identity gives the exact oracle; round-to-operand-dtype gives the yardstick of the layer-level tolerance, the
oracle with a rounding at every point where the engine stores a 16-bit tensor and nothing else:
    forward    LN1 x; attn1: the merged weights, q / k / v, P (for P V and P^T dO), the attention output; h1 (to_out + bias + x, one
               rounding); LN2 h1; attn2 likewise; h2; LN3 h2; the operand-dtype feed-forward weights; hg = proj(LN3 h2); value gelu(gate);
               out (ff.net.2 + bias + h2, one rounding)
    backward   grad_out W2; dvalue and dgate; their product with W1; dh2 (LayerNorm backward + grad_out, one rounding); attn2: the
               gradient of the attention output, dS, dq / dk / dv, the input gradient (and the context gradient); dh1 (LayerNorm
               backward + dh2); attn1 likewise; the returned input gradient (LayerNorm backward + dh1).
The fp32 adapter gradients are not rounded."""
import math
from typing import Callable, Dict, Optional

import torch
import torch.nn.functional as F

from loraattn_oracle import NAMES, _heads, _rows, deviation  # noqa: F401  (deviation: the layer-level figure, re-exported)

F64 = torch.float64
EPS = 1e-5


def _d(t):
    return t.to(F64)


def _ln(x, w, b):
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    return (x - mean) / torch.sqrt(var + EPS) * w + b


def _ln_bwd(x, dy, w):
    mean = x.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((x - mean) ** 2).mean(-1, keepdim=True) + EPS)
    xhat, g = (x - mean) * rstd, dy * w
    return rstd * (g - g.mean(-1, keepdim=True) - xhat * (g * xhat).mean(-1, keepdim=True))


def _attn_fwd(sd, prefix, lora, scaling, x, context, residual, rt):
    ctx = x if context is None else context
    h = x.shape[-1] // 64
    A = {n: _d(lora[f"{prefix}.{n}.lora_A.weight"]) for n in NAMES}
    B = {n: _d(lora[f"{prefix}.{n}.lora_B.weight"]) for n in NAMES}
    Wm = {n: rt(_d(sd[f"{prefix}.{n}.weight"]) + scaling * B[n] @ A[n]) for n in NAMES}
    q, k, v = rt(x @ Wm["to_q"].T), rt(ctx @ Wm["to_k"].T), rt(ctx @ Wm["to_v"].T)
    qh, kh, vh = _heads(q, h), _heads(k, h), _heads(v, h)
    s = 0.125 * qh @ kh.transpose(-1, -2)
    p = torch.exp(s - torch.logsumexp(s, -1)[..., None])
    pr = rt(p)
    oh = rt(pr @ vh)
    o = _rows(oh)
    out = rt(o @ Wm["to_out.0"].T + _d(sd[f"{prefix}.to_out.0.bias"]) + residual)
    return out, dict(x=x, ctx=ctx, cross=context is not None, A=A, B=B, Wm=Wm, qh=qh, kh=kh, vh=vh, p=p, pr=pr, oh=oh, o=o, h=h)


def _attn_bwd(prefix, scaling, c, g, rt, res):
    """The gradients of one attention module from the gradient `g` of its output; the adapter gradients go into `res` by key.  Returns
    (input gradient, context gradient or None), both rounded."""
    Wm, A, B, h = c["Wm"], c["A"], c["B"], c["h"]
    doh = _heads(rt(g @ Wm["to_out.0"]), h)
    delta = (doh * c["oh"]).sum(-1, keepdim=True)
    ds = rt(c["p"] * (doh @ c["vh"].transpose(-1, -2) - delta))
    dq, dk, dv = _rows(rt(0.125 * ds @ c["kh"])), _rows(rt(0.125 * ds.transpose(-1, -2) @ c["qh"])), _rows(rt(c["pr"].transpose(-1, -2) @ doh))

    def adapter(name, xin, dy):
        x2, dy2 = xin.reshape(-1, xin.shape[-1]), dy.reshape(-1, dy.shape[-1])
        res[f"{prefix}.{name}.lora_B.weight"] = scaling * dy2.T @ (x2 @ A[name].T)
        res[f"{prefix}.{name}.lora_A.weight"] = scaling * (dy2 @ B[name]).T @ x2

    adapter("to_out.0", c["o"], g)
    adapter("to_q", c["x"], dq)
    adapter("to_k", c["ctx"], dk)
    adapter("to_v", c["ctx"], dv)
    dctx = dk @ Wm["to_k"] + dv @ Wm["to_v"]
    if c["cross"]:
        return rt(dq @ Wm["to_q"]), rt(dctx)
    return rt(dq @ Wm["to_q"] + dctx), None


def _phi(t):
    return 0.5 * torch.erfc(-t / math.sqrt(2.0)), torch.exp(-0.5 * t * t) / math.sqrt(2.0 * math.pi)


def run(sd: Dict[str, torch.Tensor], prefix: str, lora: Dict[str, torch.Tensor], scaling: float, x, context, grad_out,
        rt: Optional[Callable] = None) -> Dict[str, torch.Tensor]:
    """Forward and backward.  sd: the block's frozen weights by upstream key (`<prefix>.attn1.to_q.weight` ... `<prefix>.norm1.weight`,
    `<prefix>.ff.net.0.proj.weight`, `<prefix>.ff.net.2.bias`); lora: the 16 adapter tensors; x [b][n][c]; context [b][n_kv][context_dim];
    grad_out like the output.  Returns `out`, `input`, `context` and the 16 adapter gradients by key."""
    rt = rt or (lambda t: t)
    x, ctx, g = _d(x), _d(context), _d(grad_out)
    nw = [(_d(sd[f"{prefix}.norm{i}.weight"]), _d(sd[f"{prefix}.norm{i}.bias"])) for i in (1, 2, 3)]
    w1, b1 = rt(_d(sd[f"{prefix}.ff.net.0.proj.weight"])), _d(sd[f"{prefix}.ff.net.0.proj.bias"])
    w2, b2 = rt(_d(sd[f"{prefix}.ff.net.2.weight"])), _d(sd[f"{prefix}.ff.net.2.bias"])
    inner = w2.shape[1]
    h1, c1 = _attn_fwd(sd, f"{prefix}.attn1", lora, scaling, rt(_ln(x, *nw[0])), None, x, rt)
    h2, c2 = _attn_fwd(sd, f"{prefix}.attn2", lora, scaling, rt(_ln(h1, *nw[1])), ctx, h1, rt)
    hg = rt(rt(_ln(h2, *nw[2])) @ w1.T + b1)
    value, gate = hg[..., :inner], hg[..., inner:]
    cdf, pdf = _phi(gate)
    act = rt(value * gate * cdf)
    res = {"out": rt(act @ w2.T + b2 + h2)}
    # backward
    dact = rt(g @ w2)
    dhg = torch.cat([rt(dact * gate * cdf), rt(dact * value * (cdf + gate * pdf))], -1)
    dh2 = rt(_ln_bwd(h2, rt(dhg @ w1), nw[2][0]) + g)
    din2, res["context"] = _attn_bwd(f"{prefix}.attn2", scaling, c2, dh2, rt, res)
    dh1 = rt(_ln_bwd(h1, din2, nw[1][0]) + dh2)
    din1, _ = _attn_bwd(f"{prefix}.attn1", scaling, c1, dh1, rt, res)
    res["input"] = rt(_ln_bwd(x, din1, nw[0][0]) + dh1)
    return res


def autograd_block(sd, prefix, lora, scaling, x, context, grad_out) -> Dict[str, torch.Tensor]:
    """The same quantities from torch autograd in float64: F.layer_norm, F.linear, F.gelu, unmerged adapters, SDPA."""
    x = _d(x).clone().requires_grad_(True)
    ctx = _d(context).clone().requires_grad_(True)
    par = {k: _d(v).clone().requires_grad_(True) for k, v in lora.items()}
    c = x.shape[-1]

    def lin(mod, name, t, bias=None):
        a, b = par[f"{prefix}.{mod}.{name}.lora_A.weight"], par[f"{prefix}.{mod}.{name}.lora_B.weight"]
        return F.linear(t, _d(sd[f"{prefix}.{mod}.{name}.weight"]), bias) + F.linear(F.linear(t, a), b) * scaling

    def attn(mod, t, src):
        h = c // 64
        q, k, v = _heads(lin(mod, "to_q", t), h), _heads(lin(mod, "to_k", src), h), _heads(lin(mod, "to_v", src), h)
        return lin(mod, "to_out.0", _rows(F.scaled_dot_product_attention(q, k, v, scale=0.125)), _d(sd[f"{prefix}.{mod}.to_out.0.bias"]))

    def norm(i, t):
        return F.layer_norm(t, (c,), _d(sd[f"{prefix}.norm{i}.weight"]), _d(sd[f"{prefix}.norm{i}.bias"]), EPS)

    n1 = norm(1, x)
    h1 = x + attn("attn1", n1, n1)
    h2 = h1 + attn("attn2", norm(2, h1), ctx)
    value, gate = F.linear(norm(3, h2), _d(sd[f"{prefix}.ff.net.0.proj.weight"]), _d(sd[f"{prefix}.ff.net.0.proj.bias"])).chunk(2, -1)
    out = h2 + F.linear(value * F.gelu(gate), _d(sd[f"{prefix}.ff.net.2.weight"]), _d(sd[f"{prefix}.ff.net.2.bias"]))
    (out * _d(grad_out)).sum().backward()
    res = {"out": out.detach(), "input": x.grad, "context": ctx.grad}
    res.update({k: v.grad for k, v in par.items()})
    return res
