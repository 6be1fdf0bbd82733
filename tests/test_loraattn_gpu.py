"""The LoRA attention layer on the device against its float64 oracle (tests/loraattn_oracle.py): a self-attention layer (channels 128,
70 tokens, batch 2) and a cross-attention layer (context 77 x 128, the context gradient asked for and not), both dtypes, adapters in
upstream's initial state (B = 0) and in a trained-looking state.  The output, lse, the eight adapter gradients, `input` and `context`
are compared.

Tolerance (measured, not derived: four chained 16-bit stages).  Per tensor, the figure is max |deviation from the exact oracle| /
max |exact|.  The yardstick is the oracle itself with a rounding to the operand dtype at every point where the engine stores a 16-bit
tensor and nothing else (loraattn_oracle's `rt` hook).  The device's figure may be at most TWICE the yardstick's: the factor covers the
fp32 accumulation and the exp that the emulation leaves exact.  A tensor that is exactly 0 in the oracle (every lora_A gradient while
B = 0) must be exactly 0 on the device.  Both figures are printed per tensor and dtype; DESIGN §4.17 records them.

Also, with no tolerance: the layer's adapters saved with save_lora, loaded back and merged by a second layer give bit-identical packed
weights, after a change of the adapters on the device (refresh)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loraattn_oracle as O  # noqa: E402
import matrix_common as MC  # noqa: E402
from faceposegenerator_amd import weights as W  # noqa: E402
from faceposegenerator_amd.loraattn import NAMES, LoRAAttention  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TDT = {"f16": torch.float16, "bf16": torch.bfloat16}
_WORST = MC.Worst("LoRA attention layer", ratio="device figure / yardstick")
_ORACLE = {}


def _layer(context_dim, trained, seed=5):
    layer = LoRAAttention.from_synthetic(seed, 128, context_dim, 4).init_adapters(torch.Generator().manual_seed(seed + 1))
    if trained:
        g = torch.Generator().manual_seed(seed + 2)
        layer.load_adapters({k: (v if "lora_A" in k else torch.randn(v.shape, generator=g) * 0.05) for k, v in layer.state_dict().items()})
    return layer


def _sd(layer):
    sd = {f"{layer.prefix}.{n}.weight": layer.base[n].cpu() for n in NAMES}
    sd[f"{layer.prefix}.to_out.0.bias"] = layer.bias.cpu()
    return sd


def _problem(cross, trained, dtype):
    """The layer, its inputs (operand-dtype values) and both oracles, once per (kind, state, dtype)."""
    key = (cross, trained, dtype)
    if key not in _ORACLE:
        t = TDT[dtype]
        layer = _layer(128 if cross else None, trained)
        g = torch.Generator().manual_seed(21)
        x = torch.randn(2, 70, 128, generator=g).to(t)
        ctx = torch.randn(2, 77, 128, generator=g).to(t) if cross else None
        go = torch.randn(2, 70, 128, generator=g).to(t)
        args = (_sd(layer), layer.prefix, layer.state_dict(), layer.scaling, x, ctx, go)
        exact = O.run(*args)
        yard = O.run(*args, rt=lambda v: v.float().to(t).double())
        _ORACLE[key] = (layer, x, ctx, go, exact, yard)
    return _ORACLE[key]


@pytest.mark.parametrize("dtype", ("f16", "bf16"))
@pytest.mark.parametrize("trained", (False, True))
@pytest.mark.parametrize("cross", (False, True))
def test_layer_against_oracle(lib, cross, trained, dtype):
    layer, x, ctx, go, exact, yard = _problem(cross, trained, dtype)
    layer.to(DEV, TDT[dtype])
    fwd = layer(x.to(DEV), None if ctx is None else ctx.to(DEV))
    grads = [layer.backward(fwd, go.to(DEV), need_context_grad=need) for need in ((False, True) if cross else (False,))]
    torch.cuda.synchronize()
    assert grads[0].context is None
    got = {"out": fwd.out, "lse": fwd.lse, "input": grads[-1].input, **grads[-1].adapters}
    if cross:
        got["context"] = grads[1].context
        assert torch.equal(grads[0].input, grads[1].input)                 # asking for the context gradient changes nothing else
        for k in grads[0].adapters:
            assert torch.equal(grads[0].adapters[k], grads[1].adapters[k]), k
    assert set(got) == {k for k, v in exact.items() if v is not None}
    tag = f"{'cross' if cross else 'self'} {'trained' if trained else 'initial'} {dtype}"
    failures = []
    for k in sorted(got):
        g = got[k].detach().cpu().double().reshape(exact[k].shape)
        assert torch.isfinite(g).all(), k
        if not exact[k].any():
            assert not g.any(), f"{k}: exactly 0 in the oracle (B = 0), not on the device"
            continue
        dev_fig, yard_fig = O.deviation(g, exact[k]), O.deviation(yard[k], exact[k])
        short = k.replace(layer.prefix + ".", "")
        print(f"{tag} {short:24s} device {dev_fig:.3e}  yardstick {yard_fig:.3e}  ratio {dev_fig / yard_fig:.2f}")
        _WORST.note(f"{dtype} {short}", dev_fig / yard_fig, tag)
        if not dev_fig <= 2 * yard_fig:
            failures.append(f"{short}: device {dev_fig:.3e} > 2 x yardstick {yard_fig:.3e}")
    assert not failures, tag + "\n" + "\n".join(failures)


@pytest.mark.parametrize("dtype", ("f16", "bf16"))
def test_saved_adapters_merge_to_the_same_bits(lib, dtype, tmp_path):
    layer = _layer(128, True, seed=8).to(DEV, TDT[dtype])
    g = torch.Generator().manual_seed(4)
    layer.load_adapters({k: v + torch.randn(v.shape, generator=g) * 0.01 for k, v in layer.state_dict().items()})      # a step's worth of change
    back, _ = W.load_lora(W.save_lora(str(tmp_path), layer.state_dict()))
    again = LoRAAttention.from_state_dict(_sd(layer), layer.prefix, back, cross=True).to(DEV, TDT[dtype])
    torch.cuda.synchronize()
    for group in ("w_fwd", "w_bwd"):
        a, b = getattr(layer, group), getattr(again, group)
        assert set(a) == set(b)
        for k in a:
            MC.same_bits(f"{group}[{k}]", b[k].cpu().view(torch.int16).numpy(), a[k].cpu().view(torch.int16).numpy())


def test_summary(lib):
    print()
    _WORST.show()
