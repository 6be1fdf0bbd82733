"""The CPU half of the (resnet, attention) stage's tests: the constructors' refusals (shapes, channels that are no multiple of 64, missing
keys), the closed-form float64 oracle (tests/lorastage_oracle.py) against torch autograd through F.group_norm, F.silu, F.conv2d, F.linear
and lorablock_oracle's block to 1e-12 for the three resnet forms, the transformer wrapper and a chain of two stages, the flipped-weight
identity on the packed [cout][tap][cin] layout's index map, the state_dict keys against weights.normalize_lora_keys, and that nothing
runs without a device."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lorastage_oracle as O  # noqa: E402
from faceposegenerator_amd import _lib as L  # noqa: E402
from faceposegenerator_amd import weights as W  # noqa: E402
from faceposegenerator_amd.loraattn import NAMES  # noqa: E402
from faceposegenerator_amd.lorablock import LoRAAdamW  # noqa: E402
from faceposegenerator_amd.lorastage import LoRAStage, LoRATransformer2D, TrainResnetBlock  # noqa: E402

RESNETS = ((64, 64, 0), (64, 128, 0), (128, 64, 64))          # (cin, cout, skip): no shortcut, shortcut, two sources with shortcut


trained, specs, two_stage_chain, chain_inputs = O.trained, O.specs, O.two_stage_chain, O.chain_inputs


def _close(a, b, what):
    assert O.deviation(a, b) < 1e-12, (what, O.deviation(a, b))


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_resnet_refusals():
    ok = TrainResnetBlock.from_synthetic(1, 64, 128)
    sd, p = ok.frozen_state_dict(), ok.prefix
    assert ok.has_shortcut and ok.time_embed_dim == 256
    for cin, cout, skip in ((0, 128, 0), (60, 128, 0), (64, 100, 0), (64, -64, 0), (64, 128, 32), (64, 128, -64)):
        with pytest.raises(ValueError, match="multiple of 64"):
            TrainResnetBlock(sd, p, cin, cout, skip)
    with pytest.raises(ValueError, match="groups"):
        TrainResnetBlock(sd, p, 64, 128, groups=48)
    for key in TrainResnetBlock.KEYS:
        with pytest.raises(KeyError, match=key.replace(".", r"\.")):
            TrainResnetBlock({k: v for k, v in sd.items() if k != f"{p}.{key}"}, p, 64, 128)
    with pytest.raises(ValueError, match="conv_shortcut"):
        TrainResnetBlock({k: v for k, v in sd.items() if "conv_shortcut" not in k}, p, 64, 128)
    with pytest.raises(ValueError, match="expected"):
        TrainResnetBlock(sd, p, 128, 128)
    with pytest.raises(ValueError, match="norm1"):
        TrainResnetBlock({**sd, f"{p}.norm1.weight": torch.ones(32)}, p, 64, 128)
    with pytest.raises(ValueError, match="time_emb_proj"):
        TrainResnetBlock({**sd, f"{p}.time_emb_proj.weight": torch.ones(64, 256)}, p, 64, 128)
    again = TrainResnetBlock.from_state_dict(sd, p)
    assert (again.cin, again.cout, again.skip, again.has_shortcut) == (64, 128, 0, True)
    assert not TrainResnetBlock.from_synthetic(2, 64, 64).has_shortcut
    two = TrainResnetBlock.from_state_dict(TrainResnetBlock.from_synthetic(3, 128, 64, 64).frozen_state_dict(), "mid_block.resnets.0", skip=64)
    assert (two.cin, two.cout, two.skip, two.has_shortcut) == (128, 64, 64, True)
    with pytest.raises(L.IdbError, match="no CPU fallback"):
        ok(torch.zeros(1, 4, 4, 64, dtype=torch.float16), torch.zeros(1, 256))
    with pytest.raises(ValueError, match="float16 or bfloat16"):
        ok.to("cuda:0", torch.float32)


def test_transformer_and_stage_refusals():
    ok = LoRATransformer2D.from_synthetic(4, 128, 128)
    sd, p = ok.frozen_state_dict(), ok.prefix
    for c in (0, 100, -64):
        with pytest.raises(ValueError, match="multiple of 64"):
            LoRATransformer2D(sd, p, c, 128)
    with pytest.raises(ValueError, match="depth"):
        LoRATransformer2D(sd, p, 128, 128, depth=0)
    with pytest.raises(ValueError, match="groups"):
        LoRATransformer2D(sd, p, 128, 128, groups=48)
    for key in ("norm.weight", "norm.bias", "proj_in.weight", "proj_in.bias", "proj_out.weight", "proj_out.bias"):
        with pytest.raises(KeyError, match=key.replace(".", r"\.")):
            LoRATransformer2D({k: v for k, v in sd.items() if k != f"{p}.{key}"}, p, 128, 128)
    with pytest.raises(KeyError):
        LoRATransformer2D(sd, p, 128, 128, depth=2)                         # no transformer_blocks.1
    with pytest.raises(ValueError, match="proj_in"):
        LoRATransformer2D({**sd, f"{p}.proj_in.weight": torch.ones(128, 64)}, p, 128, 128)
    conv_form = LoRATransformer2D({**sd, f"{p}.proj_in.weight": sd[f"{p}.proj_in.weight"].reshape(128, 128, 1, 1)}, p, 128, 128)
    assert torch.equal(conv_form.host["proj_in.weight"], ok.host["proj_in.weight"])          # a 1x1 convolution is the same matrix
    with pytest.raises(L.IdbError, match="no CPU fallback"):
        ok(torch.zeros(1, 4, 4, 128, dtype=torch.float16), torch.zeros(1, 77, 128, dtype=torch.float16))
    with pytest.raises(ValueError, match="LoRAStage"):
        LoRAStage(TrainResnetBlock.from_synthetic(5, 64, 64), ok)
    again = LoRATransformer2D.from_state_dict(sd, p, ok.init_adapters(torch.Generator().manual_seed(1)).state_dict())
    assert (again.channels, again.context_dim, again.depth, again.rank) == (128, 128, 1, 4)


# ---- the oracle is autograd -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cin,cout,skip", RESNETS)
def test_resnet_oracle_equals_autograd(cin, cout, skip):
    r = TrainResnetBlock.from_synthetic(7, cin, cout, skip)
    s = O.ResSpec(r.frozen_state_dict(), r.prefix, skip, r.groups, r.eps)
    g = torch.Generator().manual_seed(8)
    x, temb, go = torch.randn(2, 5, 3, cin, generator=g).double(), torch.randn(2, 256, generator=g), torch.randn(2, 5, 3, cout, generator=g).double()
    sk = torch.randn(2, 5, 3, skip, generator=g).double() if skip else None
    got = O.resnet_run(s, x, temb, sk, go)
    xa = x.clone().requires_grad_(True)
    ska = None if sk is None else sk.clone().requires_grad_(True)
    out = O._auto_resnet(s, xa, temb, ska)
    (out * go).sum().backward()
    _close(got["out"], out.detach(), "out")
    _close(got["input"], xa.grad, "input")
    assert (got["skip"] is None) == (skip == 0)
    if skip:
        _close(got["skip"], ska.grad, "skip")


@pytest.mark.parametrize("is_trained", (False, True))
def test_chain_oracle_equals_autograd(is_trained):
    stages = two_stage_chain(is_trained=is_trained)
    sp = [specs(s) for s in stages]
    x, temb, ctx, skips, go = chain_inputs()
    a, b = O.chain_run(sp, x, temb, ctx, skips, go), O.autograd_chain(sp, x, temb, ctx, skips, go)
    assert set(a) | {"context"} == set(b) and len([k for k in a if "lora_" in k]) == 32
    _close(a["out"], b["out"], "out")
    _close(a["input"], b["input"], "input")
    assert a["skips"][0] is None and b["skips"][0] is None
    _close(a["skips"][1], b["skips"][1], "skip")
    first = stages[0].transformer.prefix
    for k in a:
        if "lora_" not in k:
            continue
        if not (a[k].any() or b[k].any()):
            assert not is_trained and "lora_A" in k              # B = 0: every lora_A gradient vanishes
            continue
        _close(a[k], b[k], k)
    # the point of the chain: the first stage's adapters see the loss behind the second stage
    assert all(a[f"{first}.transformer_blocks.0.{m}.{n}.lora_B.weight"].abs().max() > 0 for m in ("attn1", "attn2") for n in NAMES)
    # the transformer alone, with its context gradient
    ts = sp[0][1]
    xt = torch.randn(2, 3, 3, 128, generator=torch.Generator().manual_seed(9)).double()
    got = O.transformer_run(ts, xt, ctx, torch.ones_like(xt))
    xa, ca = xt.clone().requires_grad_(True), ctx.clone().requires_grad_(True)
    par = {k: v.double().clone().requires_grad_(True) for k, v in ts.lora.items()}
    O._auto_transformer(ts, par, xa, ca).sum().backward()
    _close(got["input"], xa.grad, "transformer input")
    _close(got["context"], ca.grad, "transformer context")


# ---- the flipped weight on the packed layout --------------------------------------------------------------------------------------------
def _pack(w):
    """idb_pack_conv_weight's layout: [cout][cin][3][3] -> [cout][tap][cin] rows."""
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1)


def _gemm_conv(x, packed, cin):
    """The implicit GEMM over the packed rows: out[b][y][x][n] = sum over tap, ci of x[b][y + ky - 1][x + kx - 1][ci] packed[n][tap cin + ci]."""
    b, h, w_, _ = x.shape
    xp = torch.nn.functional.pad(x, (0, 0, 1, 1, 1, 1))
    cols = torch.cat([xp[:, ky:ky + h, kx:kx + w_] for ky in range(3) for kx in range(3)], -1)       # [b][h][w][9 cin], tap-major
    return cols @ packed.T


def test_flipped_weight_identity_on_the_packed_layout():
    g = torch.Generator().manual_seed(10)
    co, ci = 5, 3
    w = torch.randn(co, ci, 3, 3, generator=g).double()
    pf = _pack(O.flipped(w).contiguous())                                     # [ci][tap][co]
    for n in range(ci):
        for tap in range(9):
            for k in range(co):
                assert pf[n, O.packed_index(tap, k, co)] == w[k, n, (8 - tap) // 3, (8 - tap) % 3]      # tap t of the gradient reads tap 8 - t
    x = torch.randn(2, 4, 6, ci, generator=g).double().requires_grad_(True)
    go = torch.randn(2, 4, 6, co, generator=g).double()
    out = _gemm_conv(x, _pack(w), ci)
    _close(out.detach(), O._conv3(x.detach(), w), "the packed GEMM is the convolution")
    (out * go).sum().backward()
    _close(_gemm_conv(go, pf, co), x.grad, "the flipped packed GEMM is the input gradient")


# ---- adapters ---------------------------------------------------------------------------------------------------------------------------
def test_state_dict_keys_and_owners(tmp_path):
    stages = two_stage_chain()
    for st in stages:
        sd = st.state_dict()
        p = st.transformer.prefix
        assert set(sd) == {f"{p}.transformer_blocks.0.{m}.{n}.lora_{ab}.weight" for m in ("attn1", "attn2") for n in NAMES for ab in "AB"}
        assert set(W.normalize_lora_keys(sd)) == set(sd)
        back, alphas = W.load_lora(W.save_lora(str(tmp_path), sd))
        again = LoRATransformer2D.from_state_dict(st.transformer.frozen_state_dict(), p, back)
        assert alphas == {} and all(torch.equal(v, sd[k]) for k, v in again.state_dict().items())
        assert len(st.layers) == 2 and st.layers == st.transformer.layers
    for owners in (stages, stages[0], stages[0].transformer, [stages[0].transformer, stages[1]], list(stages[0].layers) + [stages[1]]):
        opt = LoRAAdamW(owners)
        assert len(opt.owners) == (4 if owners is stages or isinstance(owners, list) else 2)
    assert set(LoRAAdamW(stages).params()) == set(stages[0].state_dict()) | set(stages[1].state_dict())
    with pytest.raises(ValueError, match="share a prefix"):
        LoRAAdamW([stages[0], stages[0].transformer])
    two = LoRATransformer2D.from_synthetic(11, 64, 128, depth=2)
    assert len(two.layers) == 4 and len(two.state_dict()) == 32 and set(W.normalize_lora_keys(two.state_dict())) == set(two.state_dict())
