"""A float64 restatement of faceposegenerator_amd.lorastage: diffusers' ResnetBlock2D (GroupNorm + SiLU -> conv1 -> + time_emb_proj(SiLU(temb))
-> GroupNorm + SiLU -> conv2 -> + shortcut; over x | skip in the up path), Transformer2DModel with use_linear_projection (GroupNorm ->
proj_in -> BasicTransformerBlocks -> proj_out -> + input), one (resnet, attention) stage and a chain of stages, forward and backward in
CLOSED FORM: the output, the input and skip gradients and the adapter gradients of every block of the chain.  Everything but the
adapters is frozen upstream and gets no gradient.  The closed forms: GroupNorm's input gradient rstd (g - mean g - xhat mean(g xhat)) with
g = dy SiLU'(y) gamma; a 3x3 stride-1 padding-1 convolution's input gradient as the same convolution of the output gradient with
w.flip(2, 3).transpose(0, 1); a Linear's with the transposed matrix; the blocks are lorablock_oracle.run's.

Pinned on the CPU (tests/test_lorastage_cpu.py) against torch autograd in float64 through F.group_norm, F.silu, F.conv2d, F.linear and the
block of lorablock_oracle.autograd_block (unmerged adapters, SDPA) to 1e-12 relative.  diffusers and peft are not installed where this
project is built, so parity with their binaries is UNPINNED: the restatement follows their published source (ResnetBlock2D.forward,
Transformer2DModel.forward).

`rt` is the rounding hook: identity gives the exact oracle; round-to-operand-dtype gives the yardstick of the layer-level tolerance, the
oracle with a rounding at every point where the engine stores a 16-bit tensor and nothing else:
    resnet forward     the packed conv1 / conv2 / conv_shortcut weights; SiLU(norm1(x | skip)); conv1 + bias + time_emb_proj (one
                       rounding; the time embedding's projection stays fp32); SiLU(norm2(.)); conv2 + bias + shortcut (one rounding)
    resnet backward    the shortcut's gradient (a 1x1 GEMM; grad_out itself without a conv_shortcut); conv2's input gradient; norm2's;
                       conv1's; norm1's + the shortcut's gradient (one rounding), split into `input` and `skip`
    transformer        the operand-dtype proj_in / proj_out; norm(x); proj_in + bias; the blocks (lorablock_oracle lists their
                       points); proj_out + bias + x (one rounding); backward: grad_out proj_out; the blocks; their gradient times
                       proj_in; norm's input gradient + grad_out (one rounding)
The fp32 adapter gradients are not rounded."""
from dataclasses import dataclass
from typing import Callable, Dict, List, Optional, Sequence

import torch
import torch.nn.functional as F

import lorablock_oracle as LB
from loraattn_oracle import _heads, _rows, deviation  # noqa: F401  (deviation: the layer-level figure, re-exported)

F64 = torch.float64
SD = Dict[str, torch.Tensor]


def _d(t):
    return t.to(F64)


@dataclass
class ResSpec:
    sd: SD
    prefix: str
    skip: int = 0
    groups: int = 32
    eps: float = 1e-5


@dataclass
class TrSpec:
    sd: SD
    prefix: str
    lora: SD
    scaling: float
    depth: int = 1
    groups: int = 32
    eps: float = 1e-6


def _stats(x, groups):
    """x [b][hw][c] -> (xhat, rstd) per (sample, group), broadcast to x (the variance without eps: the caller adds it)."""
    b, hw, c = x.shape
    xg = x.reshape(b, hw, groups, c // groups)
    mean = xg.mean(dim=(1, 3), keepdim=True)
    var = ((xg - mean) ** 2).mean(dim=(1, 3), keepdim=True)
    return xg, mean, var


def _gn(x, w, b, groups, eps, silu):
    xg, mean, var = _stats(x, groups)
    y = ((xg - mean) / torch.sqrt(var + eps)).reshape(x.shape) * w + b
    return y * torch.sigmoid(y) if silu else y


def _gn_bwd(x, dy, w, b, groups, eps, silu):
    xg, mean, var = _stats(x, groups)
    rstd = 1.0 / torch.sqrt(var + eps)
    xhat = (xg - mean) * rstd
    d = dy
    if silu:
        y = xhat.reshape(x.shape) * w + b
        s = torch.sigmoid(y)
        d = dy * s * (1.0 + y * (1.0 - s))
    g = (d * w).reshape(xg.shape)
    core = rstd * (g - g.mean(dim=(1, 3), keepdim=True) - xhat * (g * xhat).mean(dim=(1, 3), keepdim=True))
    return core.reshape(x.shape)


def _conv3(x, w):
    """x NHWC [b][h][w][ci], w [co][ci][3][3] -> NHWC [b][h][w][co]; stride 1, padding 1."""
    return F.conv2d(x.permute(0, 3, 1, 2), w, padding=1).permute(0, 2, 3, 1)


def flipped(w):
    """The weight whose 3x3 stride-1 padding-1 convolution is the input gradient of w's: flipped in both spatial axes, channel axes swapped."""
    return w.flip(2, 3).transpose(0, 1)


def packed_index(tap: int, ci: int, cin: int) -> int:
    """Column of element (tap, ci) in a row of the [cout][tap][cin] layout idb_pack_conv_weight documents, restated here (the CPU test checks
    the identity on this restatement, not on the device's packer)."""
    return tap * cin + ci


# ---- the resnet -------------------------------------------------------------------------------------------------------------------------
def resnet_forward(s: ResSpec, x, temb, skip, rt):
    p, sd = s.prefix, s.sd
    cat = x if skip is None else torch.cat([x, skip], -1)
    b, h, w_, c = cat.shape
    w1, w2 = rt(_d(sd[f"{p}.conv1.weight"])), rt(_d(sd[f"{p}.conv2.weight"]))
    cout = w1.shape[0]
    n1 = (_d(sd[f"{p}.norm1.weight"]), _d(sd[f"{p}.norm1.bias"]))
    n2 = (_d(sd[f"{p}.norm2.weight"]), _d(sd[f"{p}.norm2.bias"]))
    h0 = rt(_gn(cat.reshape(b, h * w_, c), *n1, s.groups, s.eps, True)).reshape(b, h, w_, c)
    tb = F.linear(F.silu(_d(temb)), _d(sd[f"{p}.time_emb_proj.weight"]), _d(sd[f"{p}.time_emb_proj.bias"]))
    c1 = rt(_conv3(h0, w1) + _d(sd[f"{p}.conv1.bias"]) + tb[:, None, None, :])
    h1 = rt(_gn(c1.reshape(b, h * w_, cout), *n2, s.groups, s.eps, True)).reshape(b, h, w_, cout)
    ws = None
    if f"{p}.conv_shortcut.weight" in sd:
        ws = rt(_d(sd[f"{p}.conv_shortcut.weight"]).reshape(cout, c))
        short = cat @ ws.T + _d(sd[f"{p}.conv_shortcut.bias"])
    else:
        short = cat
    out = rt(_conv3(h1, w2) + _d(sd[f"{p}.conv2.bias"]) + short)
    return out, dict(cat=cat, c1=c1, w1=w1, w2=w2, ws=ws, n1=n1, n2=n2, cin=x.shape[-1])


def resnet_backward(s: ResSpec, c, g, rt):
    cat, c1 = c["cat"], c["c1"]
    b, h, w_, ctot = cat.shape
    cout = c1.shape[-1]
    dsc = g if c["ws"] is None else rt(g @ c["ws"])
    dh1 = rt(_conv3(g, flipped(c["w2"])))
    dc1 = rt(_gn_bwd(c1.reshape(b, h * w_, cout), dh1.reshape(b, h * w_, cout), *c["n2"], s.groups, s.eps, True)).reshape(b, h, w_, cout)
    dh0 = rt(_conv3(dc1, flipped(c["w1"])))
    dcat = rt(_gn_bwd(cat.reshape(b, h * w_, ctot), dh0.reshape(b, h * w_, ctot), *c["n1"], s.groups, s.eps, True).reshape(b, h, w_, ctot) + dsc)
    return dcat[..., :c["cin"]], (dcat[..., c["cin"]:] if s.skip else None)


def resnet_run(s: ResSpec, x, temb, skip, grad_out, rt: Optional[Callable] = None) -> Dict[str, Optional[torch.Tensor]]:
    rt = rt or (lambda t: t)
    out, c = resnet_forward(s, _d(x), temb, None if skip is None else _d(skip), rt)
    dx, dskip = resnet_backward(s, c, _d(grad_out), rt)
    return {"out": out, "input": dx, "skip": dskip}


# ---- the transformer wrapper ------------------------------------------------------------------------------------------------------------
def _block_prefix(s: TrSpec, i: int) -> str:
    return f"{s.prefix}.transformer_blocks.{i}"


def transformer_forward(s: TrSpec, x, context, rt):
    p, sd = s.prefix, s.sd
    b, h, w_, c = x.shape
    nw = (_d(sd[f"{p}.norm.weight"]), _d(sd[f"{p}.norm.bias"]))
    w_in, w_out = rt(_d(sd[f"{p}.proj_in.weight"]).reshape(c, c)), rt(_d(sd[f"{p}.proj_out.weight"]).reshape(c, c))
    xs = x.reshape(b, h * w_, c)
    t = rt(rt(_gn(xs, *nw, s.groups, s.eps, False)) @ w_in.T + _d(sd[f"{p}.proj_in.bias"]))
    ins = []
    for i in range(s.depth):
        ins.append(t)
        t = LB.run(sd, _block_prefix(s, i), s.lora, s.scaling, t, context, torch.zeros_like(t), rt)["out"]
    out = rt(t @ w_out.T + _d(sd[f"{p}.proj_out.bias"]) + xs).reshape(b, h, w_, c)
    return out, dict(x=xs, nw=nw, w_in=w_in, w_out=w_out, ins=ins, context=context, shape=(b, h, w_, c))


def transformer_backward(s: TrSpec, c, g, rt, adapters: SD):
    b, h, w_, ch = c["shape"]
    gs = g.reshape(b, h * w_, ch)
    d = rt(gs @ c["w_out"])
    dctx = None
    for i in reversed(range(s.depth)):
        res = LB.run(s.sd, _block_prefix(s, i), s.lora, s.scaling, c["ins"][i], c["context"], d, rt)
        adapters.update({k: v for k, v in res.items() if "lora_" in k})
        d = res["input"]
        dctx = res["context"] if dctx is None else rt(dctx + res["context"])
    dhn = rt(d @ c["w_in"])
    dx = rt(_gn_bwd(c["x"], dhn, *c["nw"], s.groups, s.eps, False) + gs)
    return dx.reshape(b, h, w_, ch), dctx


def transformer_run(s: TrSpec, x, context, grad_out, rt: Optional[Callable] = None) -> Dict[str, torch.Tensor]:
    rt = rt or (lambda t: t)
    out, c = transformer_forward(s, _d(x), _d(context), rt)
    res: Dict[str, torch.Tensor] = {}
    res["input"], res["context"] = transformer_backward(s, c, _d(grad_out), rt, res)
    res["out"] = out
    return res


# ---- a chain of (resnet, transformer) stages --------------------------------------------------------------------------------------------
def chain_forward(stages: Sequence, x, temb, context, skips, rt):
    saved, t = [], _d(x)
    for (rs, ts), skip in zip(stages, skips):
        r_out, rc = resnet_forward(rs, t, temb, None if skip is None else _d(skip), rt)
        t, tc = transformer_forward(ts, r_out, _d(context), rt)
        saved.append((rc, tc))
    return t, saved


def chain_run(stages: Sequence, x, temb, context, skips, grad_out, rt: Optional[Callable] = None) -> Dict[str, object]:
    """stages: [(ResSpec, TrSpec)]; skips: one tensor or None per stage.  Returns `out`, `input`, `skips` (a list) and every adapter gradient
    by key.  grad_out: a tensor, or a function of the chain's output."""
    rt = rt or (lambda t: t)
    out, saved = chain_forward(stages, x, temb, context, skips, rt)
    g = _d(grad_out(out) if callable(grad_out) else grad_out)
    res: Dict[str, object] = {"out": out}
    dskips: List[Optional[torch.Tensor]] = [None] * len(stages)
    for i in reversed(range(len(stages))):
        g, _ = transformer_backward(stages[i][1], saved[i][1], g, rt, res)
        g, dskips[i] = resnet_backward(stages[i][0], saved[i][0], g, rt)
    res["input"], res["skips"] = g, dskips
    return res


# ---- torch autograd through the upstream functionals ------------------------------------------------------------------------------------
def _auto_gn(x, w, b, groups, eps):
    """F.group_norm over NHWC x [b][h][w][c]."""
    return F.group_norm(x.permute(0, 3, 1, 2), groups, w, b, eps).permute(0, 2, 3, 1)


def _auto_resnet(s: ResSpec, x, temb, skip):
    p, sd = s.prefix, s.sd
    cat = x if skip is None else torch.cat([x, skip], -1)
    h0 = F.silu(_auto_gn(cat, _d(sd[f"{p}.norm1.weight"]), _d(sd[f"{p}.norm1.bias"]), s.groups, s.eps))
    tb = F.linear(F.silu(_d(temb)), _d(sd[f"{p}.time_emb_proj.weight"]), _d(sd[f"{p}.time_emb_proj.bias"]))
    c1 = F.conv2d(h0.permute(0, 3, 1, 2), _d(sd[f"{p}.conv1.weight"]), _d(sd[f"{p}.conv1.bias"]), padding=1) + tb[:, :, None, None]
    h1 = F.silu(F.group_norm(c1, s.groups, _d(sd[f"{p}.norm2.weight"]), _d(sd[f"{p}.norm2.bias"]), s.eps))
    out = F.conv2d(h1, _d(sd[f"{p}.conv2.weight"]), _d(sd[f"{p}.conv2.bias"]), padding=1)
    if f"{p}.conv_shortcut.weight" in sd:
        w = _d(sd[f"{p}.conv_shortcut.weight"])
        short = F.conv2d(cat.permute(0, 3, 1, 2), w.reshape(w.shape[0], w.shape[1], 1, 1), _d(sd[f"{p}.conv_shortcut.bias"]))
    else:
        short = cat.permute(0, 3, 1, 2)
    return (out + short).permute(0, 2, 3, 1)


def _auto_block(sd, prefix, par, scaling, x, ctx):
    """lorablock_oracle.autograd_block's forward (F.layer_norm, F.linear, F.gelu, unmerged adapters, SDPA), composable."""
    c = x.shape[-1]

    def lin(mod, name, t, bias=None):
        a, b = par[f"{prefix}.{mod}.{name}.lora_A.weight"], par[f"{prefix}.{mod}.{name}.lora_B.weight"]
        return F.linear(t, _d(sd[f"{prefix}.{mod}.{name}.weight"]), bias) + F.linear(F.linear(t, a), b) * scaling

    def attn(mod, t, src):
        h = c // 64
        q, k, v = _heads(lin(mod, "to_q", t), h), _heads(lin(mod, "to_k", src), h), _heads(lin(mod, "to_v", src), h)
        return lin(mod, "to_out.0", _rows(F.scaled_dot_product_attention(q, k, v, scale=0.125)), _d(sd[f"{prefix}.{mod}.to_out.0.bias"]))

    def norm(i, t):
        return F.layer_norm(t, (c,), _d(sd[f"{prefix}.norm{i}.weight"]), _d(sd[f"{prefix}.norm{i}.bias"]), LB.EPS)

    n1 = norm(1, x)
    h1 = x + attn("attn1", n1, n1)
    h2 = h1 + attn("attn2", norm(2, h1), ctx)
    value, gate = F.linear(norm(3, h2), _d(sd[f"{prefix}.ff.net.0.proj.weight"]), _d(sd[f"{prefix}.ff.net.0.proj.bias"])).chunk(2, -1)
    return h2 + F.linear(value * F.gelu(gate), _d(sd[f"{prefix}.ff.net.2.weight"]), _d(sd[f"{prefix}.ff.net.2.bias"]))


def _auto_transformer(s: TrSpec, par, x, ctx):
    p, sd = s.prefix, s.sd
    b, h, w_, c = x.shape
    t = _auto_gn(x, _d(sd[f"{p}.norm.weight"]), _d(sd[f"{p}.norm.bias"]), s.groups, s.eps).reshape(b, h * w_, c)
    t = F.linear(t, _d(sd[f"{p}.proj_in.weight"]).reshape(c, c), _d(sd[f"{p}.proj_in.bias"]))
    for i in range(s.depth):
        t = _auto_block(sd, _block_prefix(s, i), par, s.scaling, t, ctx)
    t = F.linear(t, _d(sd[f"{p}.proj_out.weight"]).reshape(c, c), _d(sd[f"{p}.proj_out.bias"]))
    return t.reshape(b, h, w_, c) + x


def autograd_chain(stages: Sequence, x, temb, context, skips, grad_out) -> Dict[str, object]:
    """chain_run's quantities from torch autograd in float64 (context gradient included as `context`)."""
    x = _d(x).clone().requires_grad_(True)
    ctx = _d(context).clone().requires_grad_(True)
    sk = [None if s is None else _d(s).clone().requires_grad_(True) for s in skips]
    par: SD = {}
    for _, ts in stages:
        par.update({k: _d(v).clone().requires_grad_(True) for k, v in ts.lora.items()})
    t = x
    for (rs, ts), skip in zip(stages, sk):
        t = _auto_transformer(ts, par, _auto_resnet(rs, t, temb, skip), ctx)
    g = _d(grad_out(t.detach()) if callable(grad_out) else grad_out)
    (t * g).sum().backward()
    res: Dict[str, object] = {"out": t.detach(), "input": x.grad, "context": ctx.grad, "skips": [None if s is None else s.grad for s in sk]}
    res.update({k: v.grad for k, v in par.items()})
    return res


# ---- what the two test files share: the stages under test and their inputs ---------------------------------------------------------------
def trained(model, seed):
    g = torch.Generator().manual_seed(seed)
    model.init_adapters(torch.Generator().manual_seed(seed + 1))
    model.load_adapters({k: (v if "lora_A" in k else torch.randn(v.shape, generator=g) * 0.05) for k, v in model.state_dict().items()})
    return model


def specs(stage):
    r, t = stage.resnet, stage.transformer
    return (ResSpec(r.frozen_state_dict(), r.prefix, r.skip, r.groups, r.eps),
            TrSpec(t.frozen_state_dict(), t.prefix, t.state_dict(), t.blocks[0].attn1.scaling, t.depth, t.groups, t.eps))


def two_stage_chain(seed=40, is_trained=True):
    """64 -> 128 channels with a shortcut, then 128 + 64 (a skip input) -> 64 channels: the chain the GPU file runs."""
    from faceposegenerator_amd.lorastage import LoRAStage, LoRATransformer2D, TrainResnetBlock
    stages = []
    for i, (cin, cout, skip) in enumerate(((64, 128, 0), (128, 64, 64))):
        r = TrainResnetBlock.from_synthetic(seed + i, cin, cout, skip, 256, prefix=f"up_blocks.1.resnets.{i}")
        t = LoRATransformer2D.from_synthetic(seed + 10 + i, cout, 128, prefix=f"up_blocks.1.attentions.{i}")
        t = trained(t, seed + 20 + i) if is_trained else t.init_adapters(torch.Generator().manual_seed(seed + 20 + i))
        stages.append(LoRAStage(r, t))
    return stages


def chain_inputs(seed=41, side=4, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g)       # noqa: E731
    x, temb, ctx = rnd(2, side, side, 64).to(dtype), rnd(2, 256).float(), rnd(2, 77, 128).to(dtype)
    skips = [None, rnd(2, side, side, 64).to(dtype)]
    go = rnd(2, side, side, 64).to(dtype)
    return x, temb, ctx, skips, go
