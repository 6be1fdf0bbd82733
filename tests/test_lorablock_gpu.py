"""The LoRA transformer block on the device against its float64 oracle (tests/lorablock_oracle.py), and eight real optimiser steps:
channels 128, 70 tokens, batch 2, context 77 x 128, both dtypes, adapters in upstream's initial state (B = 0) and in a trained-looking
state, the context gradient asked for and not (everything else must stay torch.equal).  The output, `input`, `context` and the 16 adapter
gradients are compared.

Tolerance: the project's layer rule (test_loraattn_gpu.py).  Per tensor, the figure is max |deviation from the exact oracle| / max |exact|.
The yardstick is the oracle itself with a rounding to the operand dtype at every point where the engine stores a 16-bit tensor and
nothing else (lorablock_oracle lists the points).  The device's figure may be at most TWICE the yardstick's.  A tensor that is exactly 0
in the oracle (every lora_A gradient while B = 0) must be exactly 0 on the device.  Every ratio is printed; DESIGN 4.18 records them.

Training: 8 train_block_step calls on loss = mean((out - target)^2), lr = cosine_lr(step, 8) * 1e-2, from B = 0.  The loss falls
monotonically over the first steps; the adapters after step 1 equal the float64 AdamW + clip_grad_norm_ oracle's step on the device's own
gradients to one fp32 ulp (the matrix's one-step criterion); the trained adapters saved with save_lora and loaded into a fresh block merge
to the same bits; a non-finite grad_out leaves every adapter and merged matrix bit-unchanged with skipped = 1."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lorablock_oracle as O  # noqa: E402
import matrix_common as MC  # noqa: E402
import tblock_matrix as TM  # noqa: E402
from faceposegenerator_amd import weights as W  # noqa: E402
from faceposegenerator_amd.lorablock import LoRAAdamW, LoRATransformerBlock, cosine_lr, train_block_step  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TDT = {"f16": torch.float16, "bf16": torch.bfloat16}
_WORST = MC.Worst("LoRA transformer block", ratio="device figure / yardstick")
_ORACLE = {}


def _block(trained, seed=5):
    block = LoRATransformerBlock.from_synthetic(seed, 128, 128, 4).init_adapters(torch.Generator().manual_seed(seed + 1))
    if trained:
        g = torch.Generator().manual_seed(seed + 2)
        block.load_adapters({k: (v if "lora_A" in k else torch.randn(v.shape, generator=g) * 0.05) for k, v in block.state_dict().items()})
    return block


def _inputs(dtype, seed=21):
    g = torch.Generator().manual_seed(seed)
    t = TDT[dtype]
    return torch.randn(2, 70, 128, generator=g).to(t), torch.randn(2, 77, 128, generator=g).to(t), torch.randn(2, 70, 128, generator=g).to(t)


def _problem(trained, dtype):
    """The block, its inputs (operand-dtype values) and both oracles, once per (state, dtype)."""
    key = (trained, dtype)
    if key not in _ORACLE:
        t = TDT[dtype]
        block = _block(trained)
        x, ctx, go = _inputs(dtype)
        args = (block.frozen_state_dict(), block.prefix, block.state_dict(), block.attn1.scaling, x, ctx, go)
        _ORACLE[key] = (block, x, ctx, go, O.run(*args), O.run(*args, rt=lambda v: v.float().to(t).double()))
    return _ORACLE[key]


@pytest.mark.parametrize("dtype", ("f16", "bf16"))
@pytest.mark.parametrize("trained", (False, True))
def test_block_against_oracle(lib, trained, dtype):
    block, x, ctx, go, exact, yard = _problem(trained, dtype)
    block.to(DEV, TDT[dtype])
    fwd = block(x.to(DEV), ctx.to(DEV))
    grads = [block.backward(fwd, go.to(DEV), need_context_grad=need) for need in (False, True)]
    torch.cuda.synchronize()
    assert grads[0].context is None
    assert torch.equal(grads[0].input, grads[1].input)                     # asking for the context gradient changes nothing else
    assert set(grads[0].adapters) == set(grads[1].adapters) and len(grads[0].adapters) == 16
    for k in grads[0].adapters:
        assert torch.equal(grads[0].adapters[k], grads[1].adapters[k]), k
        assert grads[0].adapters[k].dtype == torch.float32
    again = block(x.to(DEV), ctx.to(DEV))                                  # bit-identical repeats
    assert torch.equal(again.out, fwd.out) and torch.equal(block.backward(again, go.to(DEV)).input, grads[0].input)
    got = {"out": fwd.out, "input": grads[1].input, "context": grads[1].context, **grads[1].adapters}
    assert set(got) == set(exact)
    tag = f"{'trained' if trained else 'initial'} {dtype}"
    failures = []
    for k in sorted(got):
        g = got[k].detach().cpu().double().reshape(exact[k].shape)
        assert torch.isfinite(g).all(), k
        if not exact[k].any():
            assert not g.any(), f"{k}: exactly 0 in the oracle (B = 0), not on the device"
            continue
        dev_fig, yard_fig = O.deviation(g, exact[k]), O.deviation(yard[k], exact[k])
        short = k.replace(block.prefix + ".", "")
        print(f"{tag} {short:30s} device {dev_fig:.3e}  yardstick {yard_fig:.3e}  ratio {dev_fig / yard_fig:.2f}")
        _WORST.note(f"{dtype} {short}", dev_fig / yard_fig, tag)
        if not dev_fig <= 2 * yard_fig:
            failures.append(f"{short}: device {dev_fig:.3e} > 2 x yardstick {yard_fig:.3e}")
    assert not failures, tag + "\n" + "\n".join(failures)


def _merged_bits(block):
    return {f"{a.prefix}.{group}[{k}]": t.cpu().view(torch.int16).numpy().copy() for a in block.layers for group in ("w_fwd", "w_bwd")
            for k, t in getattr(a, group).items()}


@pytest.mark.parametrize("dtype", ("f16", "bf16"))
def test_training_steps(lib, dtype, tmp_path):
    t = TDT[dtype]
    block = _block(False, seed=11).to(DEV, t)
    teacher = _block(True, seed=11).to(DEV, t)                             # the same frozen weights with other adapters: a reachable target
    x, ctx, _ = (v.to(DEV) for v in _inputs(dtype, seed=31))
    target = teacher(x, ctx).out.float()
    opt = LoRAAdamW(block, lr=1e-2)
    n = target.numel()
    losses = []
    for step in range(8):
        opt.lr = cosine_lr(step, 8) * 1e-2
        seen = {}

        def grad(out):
            diff = out.float() - target
            seen["loss"] = float((diff * diff).mean())
            return (2.0 / n * diff * 1024.0).to(t)                         # a GradScaler's factor of 1024 on the loss

        res = train_block_step(block, opt, x, ctx, grad, inv_scale=1.0 / 1024.0)
        assert res["skipped"] is False and math.isfinite(res["grad_norm"]) and res["grad_input"].shape == x.shape
        losses.append(seen["loss"])
    print(f"{dtype}: losses {' '.join(f'{v:.6e}' for v in losses)}")
    assert opt.steps == 8
    assert all(b < a for a, b in zip(losses[:4], losses[1:5])), losses        # monotone over the first steps
    assert losses[-1] < losses[0]
    # the trained adapters, saved and loaded into a fresh block, merge to the same bits
    back, _ = W.load_lora(W.save_lora(str(tmp_path), block.state_dict()))
    again = LoRATransformerBlock.from_state_dict(block.frozen_state_dict(), block.prefix, back).to(DEV, t)
    torch.cuda.synchronize()
    a, b = _merged_bits(block), _merged_bits(again)
    assert set(a) == set(b) and len(a) == 10
    for k in a:
        MC.same_bits(k, b[k], a[k])
    assert any(v.any() for k, v in block.state_dict().items() if "lora_B" in k)            # B has left 0: a real step
    # a non-finite grad_out: nothing changes, the step is skipped and not counted
    adapters = {k: v.detach().cpu().numpy().copy() for k, v in opt.params().items()}
    moments = opt.state_dict()
    bad = torch.zeros_like(x)
    bad[0, 0, 0] = math.inf
    res = train_block_step(block, opt, x, ctx, bad)
    assert res["skipped"] is True and not math.isfinite(res["grad_norm"]) and opt.steps == 8
    for k, v in opt.params().items():
        MC.same_bits(f"{k} after a skipped step", v.detach().cpu().numpy(), adapters[k])
    after = opt.state_dict()
    for name in ("exp_avg", "exp_avg_sq"):
        for k in moments[name]:
            MC.same_bits(f"{name}[{k}] after a skipped step", after[name][k].numpy(), moments[name][k].numpy())
    c = _merged_bits(block)
    for k in a:
        MC.same_bits(f"{k} after a skipped step", c[k], a[k])


@pytest.mark.parametrize("dtype", ("f16", "bf16"))
def test_first_step_matches_the_float64_optimiser(lib, dtype):
    """One step from B = 0: the adapters equal torch.optim.AdamW + clip_grad_norm_ in float64 stepped on the DEVICE's own gradients, to
    one fp32 ulp per element (tblock_matrix's criterion), and the reported norm meets its bound."""
    t = TDT[dtype]
    block = _block(False, seed=12).to(DEV, t)
    x, ctx, go = (v.to(DEV) for v in _inputs(dtype, seed=32))
    opt = LoRAAdamW(block, lr=1e-2)
    grads = block.backward(block(x, ctx), go).adapters
    keys = sorted(grads)
    w = [opt.params()[k].detach().cpu().numpy().reshape(-1).copy() for k in keys]
    g = [grads[k].detach().cpu().numpy().reshape(-1).copy() for k in keys]
    zeros = [np.zeros_like(a) for a in w]
    case = TM.AdamCase("block", len(keys), step=1, lr=opt.lr, beta1=opt.beta1, beta2=opt.beta2, eps=opt.eps, wd=opt.weight_decay,
                       max_norm=opt.max_norm, inv_scale=0.5)
    ow, om, ov, onorm, oskip = TM.adam_oracle(case, w, g, zeros, zeros)
    norm, skipped = opt.step(grads, inv_scale=0.5)
    assert not skipped and not oskip and opt.steps == 1
    numel = sum(a.size for a in w)
    print(f"{dtype}: grad norm {norm!r} against {onorm!r}")
    assert abs(norm - onorm) <= abs(onorm) * (numel + 8) * 2.0 ** -53
    st = opt.state_dict()
    for name, got, want in (("w", [opt.params()[k].detach().cpu().numpy().reshape(-1) for k in keys], ow),
                            ("m", [st["exp_avg"][k].numpy().reshape(-1) for k in keys], om),
                            ("v", [st["exp_avg_sq"][k].numpy().reshape(-1) for k in keys], ov)):
        ok, ratio, where = TM.adam_verdict(name, got, want)
        print(f"{dtype}: {name}: worst err / ulp {ratio:.4f} at {where}")
        assert ok, (name, where, ratio)
        _WORST.note(f"{dtype} first step {name} (err / ulp)", ratio, where)


def test_summary(lib):
    print()
    _WORST.show()
