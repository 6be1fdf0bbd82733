"""The (resnet, attention) stage on the device against its float64 oracle (tests/lorastage_oracle.py), and eight real optimiser steps of a
chain of two stages.  Shapes, the smallest that still take every path: batch 2, 8 x 8 and 4 x 4 pixels, time_embed_dim 256, context
77 x 128; resnets 64 -> 64 (no shortcut), 64 -> 128 (shortcut), 128 + 64 -> 64 (two sources, shortcut); Transformer2D with 128 channels
(two heads) and with 64, the latter also with two blocks (the context gradient summed over them); one chain of two stages (64 -> 128,
then 128 + 64 -> 64 with a skip input), both dtypes, the adapters in upstream's initial state (B = 0) and in a trained-looking state.

Tolerance: the project's layer rule (test_loraattn_gpu.py, test_lorablock_gpu.py).  Per tensor, the figure is max |deviation from the exact
oracle| / max |exact|.  The yardstick is the oracle itself with a rounding to the operand dtype at every point where the engine stores a
16-bit tensor and nothing else (lorastage_oracle lists the points).  The device's figure may be at most TWICE the yardstick's.  A tensor
that is exactly 0 in the oracle (every lora_A gradient while B = 0) must be exactly 0 on the device.  Every ratio is printed; DESIGN 4.19
records them.

Also asserted: bit-identical repeats; asking for the context gradient changes no other bit; ResnetGrad.skip is None without a skip; the
chain's first-stage adapter gradients are nonzero and match the oracle of the WHOLE chain (the gradient of the second stage's loss reaches
the first stage's adapters); 8 train_stage_step calls on loss = mean((out - target)^2), lr = cosine_lr(step, 8) * 1e-2, from B = 0, towards
a target the same chain reaches with other adapters: the loss falls monotonically over the first steps; a non-finite grad_out leaves every
adapter and merged matrix bit-unchanged with skipped = 1; the trained adapters saved with save_lora and loaded into a fresh chain merge to
the same bits."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lorastage_oracle as O  # noqa: E402
import matrix_common as MC  # noqa: E402
from faceposegenerator_amd import weights as W  # noqa: E402
from faceposegenerator_amd.loraattn import NAMES  # noqa: E402
from faceposegenerator_amd.lorablock import LoRAAdamW, cosine_lr  # noqa: E402
from faceposegenerator_amd.lorastage import LoRAStage, LoRATransformer2D, TrainResnetBlock, train_stage_step  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TDT = {"f16": torch.float16, "bf16": torch.bfloat16}
_WORST = MC.Worst("LoRA stage", ratio="device figure / yardstick")


def _rt(dtype):
    t = TDT[dtype]
    return lambda v: v.float().to(t).double()


def _compare(tag, dtype, got, exact, yard, strip=""):
    failures = []
    for k in sorted(exact):
        if exact[k] is None:
            assert got[k] is None, k
            continue
        g = got[k].detach().cpu().double().reshape(exact[k].shape)
        assert torch.isfinite(g).all(), k
        if not exact[k].any():
            assert not g.any(), f"{k}: exactly 0 in the oracle (B = 0), not on the device"
            continue
        dev_fig, yard_fig = O.deviation(g, exact[k]), O.deviation(yard[k], exact[k])
        short = k.replace(strip, "")
        ratio = dev_fig / yard_fig if yard_fig > 0 else (0.0 if dev_fig == 0 else math.inf)
        print(f"{tag} {dtype} {short:58s} device {dev_fig:.3e}  yardstick {yard_fig:.3e}  ratio {ratio:.2f}")
        _WORST.note(f"{dtype} {tag.split()[0]} {short.split('transformer_blocks.')[-1]}", ratio, tag)
        if not dev_fig <= 2 * yard_fig:
            failures.append(f"{short}: device {dev_fig:.3e} > 2 x yardstick {yard_fig:.3e}")
    assert not failures, f"{tag} {dtype}\n" + "\n".join(failures)


@pytest.mark.parametrize("dtype", ("f16", "bf16"))
@pytest.mark.parametrize("side", (8, 4))
@pytest.mark.parametrize("cin,cout,skip", ((64, 64, 0), (64, 128, 0), (128, 64, 64)))
def test_resnet_against_oracle(lib, cin, cout, skip, side, dtype):
    t = TDT[dtype]
    r = TrainResnetBlock.from_synthetic(7, cin, cout, skip)
    s = O.ResSpec(r.frozen_state_dict(), r.prefix, skip, r.groups, r.eps)
    g = torch.Generator().manual_seed(8 + side)
    x, temb, go = torch.randn(2, side, side, cin, generator=g).to(t), torch.randn(2, 256, generator=g), torch.randn(2, side, side, cout, generator=g).to(t)
    sk = torch.randn(2, side, side, skip, generator=g).to(t) if skip else None
    exact, yard = O.resnet_run(s, x, temb, sk, go), O.resnet_run(s, x, temb, sk, go, rt=_rt(dtype))
    r.to(DEV, t)
    dsk = None if sk is None else sk.to(DEV)
    fwd = r(x.to(DEV), temb.to(DEV), dsk)
    grad = r.backward(fwd, go.to(DEV))
    again = r(x.to(DEV), temb.to(DEV), dsk)
    grad2 = r.backward(again, go.to(DEV))
    torch.cuda.synchronize()
    assert torch.equal(again.out, fwd.out) and torch.equal(grad2.input, grad.input)               # bit-identical repeats
    assert (grad.skip is None) == (skip == 0)
    if skip:
        assert torch.equal(grad2.skip, grad.skip) and grad.skip.shape == sk.shape
    assert fwd.out.shape == (2, side, side, cout) and grad.input.shape == x.shape and grad.input.dtype == t
    _compare(f"resnet {cin}+{skip}->{cout} {side}x{side}", dtype, {"out": fwd.out, "input": grad.input, "skip": grad.skip}, exact, yard)


@pytest.mark.parametrize("dtype", ("f16", "bf16"))
@pytest.mark.parametrize("is_trained", (False, True))
@pytest.mark.parametrize("channels,side,depth", ((128, 8, 1), (64, 4, 1), (64, 4, 2)))
def test_transformer_against_oracle(lib, channels, side, depth, is_trained, dtype):
    t = TDT[dtype]
    m = LoRATransformer2D.from_synthetic(14, channels, 128, depth=depth)
    m = O.trained(m, 15) if is_trained else m.init_adapters(torch.Generator().manual_seed(15))
    s = O.TrSpec(m.frozen_state_dict(), m.prefix, m.state_dict(), m.blocks[0].attn1.scaling, m.depth, m.groups, m.eps)
    g = torch.Generator().manual_seed(16)
    x, ctx, go = torch.randn(2, side, side, channels, generator=g).to(t), torch.randn(2, 77, 128, generator=g).to(t), torch.randn(2, side, side, channels, generator=g).to(t)
    exact, yard = O.transformer_run(s, x, ctx, go), O.transformer_run(s, x, ctx, go, rt=_rt(dtype))
    m.to(DEV, t)
    fwd = m(x.to(DEV), ctx.to(DEV))
    grads = [m.backward(fwd, go.to(DEV), need_context_grad=need) for need in (False, True)]
    again = m(x.to(DEV), ctx.to(DEV))
    torch.cuda.synchronize()
    assert grads[0].context is None and torch.equal(grads[0].input, grads[1].input)          # asking for the context gradient changes nothing else
    assert set(grads[0].adapters) == set(grads[1].adapters) == set(m.state_dict()) and len(grads[0].adapters) == 16 * depth
    for k in grads[0].adapters:
        assert torch.equal(grads[0].adapters[k], grads[1].adapters[k]) and grads[0].adapters[k].dtype == torch.float32, k
    assert torch.equal(again.out, fwd.out) and torch.equal(m.backward(again, go.to(DEV)).input, grads[0].input)
    got = {"out": fwd.out, "input": grads[1].input, "context": grads[1].context, **grads[1].adapters}
    assert set(got) == set(exact)
    _compare(f"transformer2d {channels} {side}x{side} depth {depth} {'trained' if is_trained else 'initial'}", dtype, got, exact, yard, strip=m.prefix + ".")


def _chain_on_device(is_trained, t, seed=40):
    stages = O.two_stage_chain(seed, is_trained)
    for st in stages:
        st.to(DEV, t)
    return stages


def _forward_backward(stages, x, temb, ctx, skips, go):
    saved, cur = [], x
    for st, sk in zip(stages, skips):
        saved.append(st(cur, temb, ctx, sk))
        cur = saved[-1].out
    res = {"out": cur}
    dskips = [None] * len(stages)
    g = go
    for i in reversed(range(len(stages))):
        sg = stages[i].backward(saved[i], g)
        res.update(sg.adapters)
        g, dskips[i] = sg.input, sg.skip
    res["input"], res["skips"] = g, dskips
    return res


@pytest.mark.parametrize("dtype", ("f16", "bf16"))
@pytest.mark.parametrize("is_trained", (False, True))
def test_chain_against_oracle(lib, is_trained, dtype):
    """The test that fails without the feature: the first stage's adapter gradients under a loss behind the second stage."""
    t = TDT[dtype]
    stages = O.two_stage_chain(40, is_trained)
    sp = [O.specs(s) for s in stages]
    x, temb, ctx, skips, go = O.chain_inputs(dtype=t)
    exact, yard = O.chain_run(sp, x, temb, ctx, skips, go), O.chain_run(sp, x, temb, ctx, skips, go, rt=_rt(dtype))
    for st in stages:
        st.to(DEV, t)
    dev = lambda v: None if v is None else v.to(DEV)       # noqa: E731
    args = (dev(x), dev(temb), dev(ctx), [dev(s) for s in skips], dev(go))
    got, rep = _forward_backward(stages, *args), _forward_backward(stages, *args)
    torch.cuda.synchronize()
    assert set(got) == set(exact) and len([k for k in got if "lora_" in k]) == 32
    for k in got:
        if k != "skips":
            assert torch.equal(got[k], rep[k]), k                             # bit-identical repeats
    assert got["skips"][0] is None and torch.equal(got["skips"][1], rep["skips"][1])
    first = stages[0].transformer.prefix
    for m in ("attn1", "attn2"):
        for n in NAMES:
            assert got[f"{first}.transformer_blocks.0.{m}.{n}.lora_B.weight"].any(), (m, n)
            assert bool(got[f"{first}.transformer_blocks.0.{m}.{n}.lora_A.weight"].any()) == is_trained, (m, n)
    flat = lambda d: {**{k: v for k, v in d.items() if k != "skips"}, "skip[1]": d["skips"][1]}       # noqa: E731
    _compare(f"chain {'trained' if is_trained else 'initial'}", dtype, flat(got), flat(exact), flat(yard), strip="up_blocks.1.")


def _merged_bits(stages):
    return {f"{a.prefix}.{group}[{k}]": v.cpu().view(torch.int16).numpy().copy() for st in stages for a in st.layers for group in ("w_fwd", "w_bwd")
            for k, v in getattr(a, group).items()}


@pytest.mark.parametrize("dtype", ("f16", "bf16"))
def test_training_steps(lib, dtype, tmp_path):
    t = TDT[dtype]
    stages, teacher = _chain_on_device(False, t, seed=50), _chain_on_device(True, t, seed=50)      # the same frozen weights with other adapters
    x, temb, ctx, skips, _ = (None if v is None else ([None if s is None else s.to(DEV) for s in v] if isinstance(v, list) else v.to(DEV))
                              for v in O.chain_inputs(seed=51, dtype=t))
    cur = x
    for st, sk in zip(teacher, skips):
        cur = st(cur, temb, ctx, sk).out
    target = cur.float()
    opt = LoRAAdamW(stages, lr=1e-2)
    assert len(opt.owners) == 4
    n = target.numel()
    losses = []
    for step in range(8):
        opt.lr = cosine_lr(step, 8) * 1e-2
        seen = {}

        def grad(out):
            diff = out.float() - target
            seen["loss"] = float((diff * diff).mean())
            return (2.0 / n * diff * 1024.0).to(t)                         # a GradScaler's factor of 1024 on the loss

        res = train_stage_step(stages, opt, x, temb, ctx, grad, inv_scale=1.0 / 1024.0, skips=skips)
        assert res["skipped"] is False and math.isfinite(res["grad_norm"]) and res["grad_input"].shape == x.shape
        assert res["grad_skips"][0] is None and res["grad_skips"][1].shape == skips[1].shape and len(res["adapters"]) == 32
        losses.append(seen["loss"])
    print(f"{dtype}: losses {' '.join(f'{v:.6e}' for v in losses)}")
    assert opt.steps == 8
    assert all(b < a for a, b in zip(losses[:4], losses[1:5])), losses        # monotone over the first steps
    assert losses[-1] < losses[0]
    for st in stages:                                                          # B has left 0 in BOTH stages: the first one saw the loss
        assert any(v.any() for k, v in st.state_dict().items() if "lora_B" in k)
    # the trained adapters, saved and loaded into a fresh chain, merge to the same bits
    lora = {k: v for st in stages for k, v in st.state_dict().items()}
    back, _ = W.load_lora(W.save_lora(str(tmp_path), lora))
    fresh = [LoRAStage(TrainResnetBlock.from_state_dict(st.resnet.frozen_state_dict(), st.resnet.prefix, st.resnet.skip),
                       LoRATransformer2D.from_state_dict(st.transformer.frozen_state_dict(), st.transformer.prefix)).load_adapters(back).to(DEV, t)
             for st in stages]
    torch.cuda.synchronize()
    a, b = _merged_bits(stages), _merged_bits(fresh)
    assert set(a) == set(b) and len(a) == 20
    for k in a:
        MC.same_bits(k, b[k], a[k])
    # a non-finite grad_out: nothing changes, the step is skipped and not counted
    adapters = {k: v.detach().cpu().numpy().copy() for k, v in opt.params().items()}
    bad = torch.zeros_like(target).to(t)
    bad[0, 0, 0, 0] = math.inf
    res = train_stage_step(stages, opt, x, temb, ctx, bad, skips=skips)
    assert res["skipped"] is True and not math.isfinite(res["grad_norm"]) and opt.steps == 8
    for k, v in opt.params().items():
        MC.same_bits(f"{k} after a skipped step", v.detach().cpu().numpy(), adapters[k])
    c = _merged_bits(stages)
    for k in a:
        MC.same_bits(f"{k} after a skipped step", c[k], a[k])


def test_summary(lib):
    print()
    _WORST.show()
