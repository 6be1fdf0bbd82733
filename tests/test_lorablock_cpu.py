"""CPU checks of the LoRA transformer block (faceposegenerator_amd/lorablock.py) and its float64 oracle (tests/lorablock_oracle.py): the
closed-form oracle against torch autograd, the 16 adapter keys and the save / load round trip, the constructors' and the optimiser's
refusals, the optimiser's state dict, and the residual keyword's refusal on the attention layer."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lorablock_oracle as O  # noqa: E402
from faceposegenerator_amd import _lib as L, weights as W  # noqa: E402
from faceposegenerator_amd.lorablock import LoRAAdamW, LoRATransformerBlock  # noqa: E402
from faceposegenerator_amd.loraattn import NAMES, LoRAAttention  # noqa: E402


def _block(trained=True, rank=4, alpha=None, seed=5, context_dim=192):
    block = LoRATransformerBlock.from_synthetic(seed, 128, context_dim, rank, alpha).init_adapters(torch.Generator().manual_seed(seed + 1))
    if trained:
        g = torch.Generator().manual_seed(seed + 2)
        block.load_adapters({k: (v if "lora_A" in k else torch.randn(v.shape, generator=g) * 0.05) for k, v in block.state_dict().items()})
    return block


@pytest.mark.parametrize("trained", [False, True])
def test_oracle_matches_autograd(trained):
    """Closed form against autograd (F.layer_norm, F.gelu, unmerged adapters, SDPA), float64, 1e-12 relative per tensor."""
    block = _block(trained, rank=5, alpha=10.0)
    g = torch.Generator().manual_seed(9)
    x = torch.randn(2, 37, 128, generator=g, dtype=torch.float64)
    ctx = torch.randn(2, 11, 192, generator=g, dtype=torch.float64)
    go = torch.randn(2, 37, 128, generator=g, dtype=torch.float64)
    args = (block.frozen_state_dict(), block.prefix, block.state_dict(), block.attn1.scaling, x, ctx, go)
    a, b = O.run(*args), O.autograd_block(*args)
    assert set(a) == set(b) and len(a) == 19
    for k in a:
        assert O.deviation(a[k], b[k]) < 1e-12 or not (a[k].any() or b[k].any()), (k, O.deviation(a[k], b[k]))
    for mod in ("attn1", "attn2"):
        for n in NAMES:
            ka, kb = (f"{block.prefix}.{mod}.{n}.lora_{ab}.weight" for ab in "AB")
            assert a[kb].abs().max() > 0 and bool(a[ka].any()) == trained          # B = 0: every lora_A gradient vanishes, no lora_B one


def test_state_dict_keys_and_round_trip(tmp_path):
    block = _block()
    sd = block.state_dict()
    assert len(sd) == 16
    assert set(sd) == {f"{block.prefix}.{m}.{n}.lora_{ab}.weight" for m in ("attn1", "attn2") for n in NAMES for ab in "AB"}
    assert set(W.normalize_lora_keys(sd)) == set(sd)
    back, alphas = W.load_lora(W.save_lora(str(tmp_path), sd))
    assert alphas == {} and set(back) == set(sd)
    again = LoRATransformerBlock.from_state_dict(block.frozen_state_dict(), block.prefix, back)
    assert again.rank == block.rank and again.context_dim == 192 and again.inner == 512 and again.channels == 128
    for k, v in again.state_dict().items():
        assert torch.equal(v, sd[k]) and v.dtype == torch.float32
    for k, v in again.frozen_state_dict().items():
        assert torch.equal(v, block.frozen_state_dict()[k]), k
    fresh = LoRATransformerBlock.from_synthetic(3).init_adapters(torch.Generator().manual_seed(1))
    assert not any(v.any() for k, v in fresh.state_dict().items() if "lora_B" in k)
    assert all(v.any() for k, v in fresh.state_dict().items() if "lora_A" in k)


def test_refusals():
    block = _block()
    sd, p = block.frozen_state_dict(), block.prefix
    with pytest.raises(ValueError, match="multiple of 64"):
        LoRATransformerBlock(sd, p, 96, 192)
    with pytest.raises(ValueError, match="at most 1536"):
        LoRATransformerBlock(sd, p, 1600, 192)
    with pytest.raises(ValueError, match="expected"):
        LoRATransformerBlock(sd, p, 192, 192)
    with pytest.raises(ValueError, match="context_dim is required"):
        LoRATransformerBlock(sd, p, 128, None)
    bad = dict(sd)
    bad[f"{p}.ff.net.0.proj.weight"] = sd[f"{p}.ff.net.0.proj.weight"][:-64]
    with pytest.raises(ValueError, match="ff is"):
        LoRATransformerBlock(bad, p, 128, 192)
    bad = dict(sd)
    bad[f"{p}.norm2.weight"] = torch.ones(64)
    with pytest.raises(ValueError, match="norm2"):
        LoRATransformerBlock(bad, p, 128, 192)
    with pytest.raises(ValueError, match="HIP device"):
        block.to("cpu")
    with pytest.raises(ValueError, match="float16 or bfloat16"):
        block.to("cuda:0", torch.float32)
    with pytest.raises(L.IdbError, match="no CPU fallback"):
        block(torch.zeros(1, 4, 128, dtype=torch.float16), torch.zeros(1, 4, 192, dtype=torch.float16))
    block.device = block.attn2.device = torch.device("cpu")
    with pytest.raises(ValueError, match="needs a context"):
        block(torch.zeros(1, 4, 128, dtype=torch.float16), None)
    # the attention layer's new keyword: a residual of another shape is refused before any device work
    layer = LoRAAttention.from_synthetic(1)
    layer.device, layer.dtype = torch.device("cpu"), torch.float16
    with pytest.raises(ValueError, match="residual must match"):
        layer(torch.zeros(1, 4, 128, dtype=torch.float16), None, residual=torch.zeros(1, 5, 128, dtype=torch.float16))


def test_optimizer_host_side():
    block = _block()
    opt = LoRAAdamW(block)
    assert (opt.lr, opt.beta1, opt.beta2, opt.eps, opt.weight_decay, opt.max_norm, opt.steps) == (1e-4, 0.9, 0.999, 1e-8, 1e-2, 1.0, 0)
    assert set(opt.params()) == set(block.state_dict()) and len(opt.owners) == 2
    assert len(LoRAAdamW([block.attn1]).params()) == 8 and len(LoRAAdamW([block, LoRAAttention.from_synthetic(1, prefix="other.attn1")]).params()) == 24
    for kw in (dict(lr=-1.0), dict(betas=(1.0, 0.999)), dict(betas=(0.9, -0.1)), dict(eps=-1e-8), dict(weight_decay=-1.0), dict(max_norm=0.0)):
        with pytest.raises(ValueError, match="LoRAAdamW"):
            LoRAAdamW(block, **kw)
    with pytest.raises(ValueError, match="share a prefix"):
        LoRAAdamW([block, block.attn1])
    with pytest.raises(ValueError, match="takes a"):
        LoRAAdamW([])
    with pytest.raises(L.IdbError, match="no CPU fallback"):
        opt.step({k: torch.zeros_like(v) for k, v in opt.params().items()})
    # the state dict: hyper-parameters, steps, and moment buffers exactly after the first step
    sd = opt.state_dict()
    assert sd["steps"] == 0 and sd["exp_avg"] is None and sd["exp_avg_sq"] is None and sd["lr"] == 1e-4
    m = {k: torch.full_like(v, 0.5) for k, v in opt.params().items()}
    v = {k: torch.full_like(p, 0.25) for k, p in opt.params().items()}
    other = LoRAAdamW(block, lr=1.0)
    other.load_state_dict({**sd, "steps": 3, "lr": 2e-4, "exp_avg": m, "exp_avg_sq": v})
    back = other.state_dict()
    assert back["steps"] == 3 and back["lr"] == 2e-4 and all(torch.equal(back["exp_avg"][k], m[k]) and torch.equal(back["exp_avg_sq"][k], v[k]) for k in m)
    with pytest.raises(ValueError, match="exactly after the first step"):
        other.load_state_dict({**sd, "steps": 3})
    with pytest.raises(ValueError, match="without"):
        other.load_state_dict({k: x for k, x in sd.items() if k != "eps"})
    with pytest.raises(ValueError, match="keys and shapes"):
        other.load_state_dict({**sd, "steps": 1, "exp_avg": {}, "exp_avg_sq": v})
