"""DINOv2 on the CPU: tests/dinov2_oracle.py against transformers' Dinov2Model (an independent implementation) and against Pillow,
the position-embedding interpolation, the loader (architecture inference, key spellings, refusals, LayerScale and patch-weight
folding), and the size of the storage-format error that the GPU tests use as their bound."""
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dinov2_oracle as O  # noqa: E402

from faceposegenerator_amd import dinov2 as D  # noqa: E402


def _hf_to_hub(hf):
    """transformers Dinov2Model state dict -> the hub layout."""
    sd = {"cls_token": hf["embeddings.cls_token"], "pos_embed": hf["embeddings.position_embeddings"],
          "patch_embed.proj.weight": hf["embeddings.patch_embeddings.projection.weight"],
          "patch_embed.proj.bias": hf["embeddings.patch_embeddings.projection.bias"],
          "norm.weight": hf["layernorm.weight"], "norm.bias": hf["layernorm.bias"]}
    i = 0
    while f"encoder.layer.{i}.norm1.weight" in hf:
        s, d = f"encoder.layer.{i}.", f"blocks.{i}."
        for n in ("norm1", "norm2", "mlp.fc1", "mlp.fc2"):
            for t in ("weight", "bias"):
                sd[f"{d}{n}.{t}"] = hf[f"{s}{n}.{t}"]
        for t in ("weight", "bias"):
            sd[f"{d}attn.qkv.{t}"] = torch.cat([hf[f"{s}attention.attention.{n}.{t}"] for n in ("query", "key", "value")], dim=0)
            sd[f"{d}attn.proj.{t}"] = hf[f"{s}attention.output.dense.{t}"]
        sd[d + "ls1.gamma"], sd[d + "ls2.gamma"] = hf[s + "layer_scale1.lambda1"], hf[s + "layer_scale2.lambda1"]
        i += 1
    return sd


def test_oracle_matches_transformers_dinov2():
    from transformers import Dinov2Config, Dinov2Model
    torch.manual_seed(0)
    m = Dinov2Model(Dinov2Config(hidden_size=128, num_hidden_layers=2, num_attention_heads=2, image_size=224, patch_size=14,
                                 layer_norm_eps=1e-6)).double().eval()
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for name, p in m.named_parameters():             # the defaults (zero biases, unit LayerScale, zero cls) would hide mistakes
            if name.endswith("bias") or "lambda1" in name or "cls_token" in name or "position_embeddings" in name:
                p.copy_(0.3 * torch.randn(p.shape, generator=g, dtype=torch.float64) + (0.5 if "lambda1" in name else 0.0))
    x = torch.randn(2, 3, 224, 224, generator=g, dtype=torch.float64)
    with torch.no_grad():
        ref = m(pixel_values=x).pooler_output
    got = O.forward(_hf_to_hub(m.state_dict()), x, heads=2)
    err = (got - ref).abs().max().item()
    print(f"oracle vs transformers: max-abs {err:.3e}, max|ref| {ref.abs().max().item():.3f}")
    assert err <= 1e-9 * ref.abs().max().item()


@pytest.mark.parametrize("s", [512, 768, 250, 224, 100])
def test_oracle_resize_bit_equal_to_pillow(s):
    img = np.random.default_rng(s).integers(0, 256, (s, s, 3), dtype=np.uint8)
    ref = np.asarray(Image.fromarray(img).resize((224, 224), Image.BICUBIC))
    assert np.array_equal(O.resize_pil_u8(img), ref)


def test_pos_embed_interpolation():
    g = torch.Generator().manual_seed(2)
    same = torch.randn(1, 257, 64, generator=g, dtype=torch.float64)
    assert torch.equal(O.interpolate_pos(same), same)
    assert torch.equal(D.interpolate_pos_embed(same.float()), same.float())
    pos = torch.randn(1, 1 + 37 * 37, 64, generator=g, dtype=torch.float64)
    got = O.interpolate_pos(pos)
    s = (16 + 0.1) / 37
    ref = F.interpolate(pos[:, 1:].reshape(1, 37, 37, 64).permute(0, 3, 1, 2), scale_factor=(s, s), mode="bicubic", antialias=False)
    assert tuple(ref.shape) == (1, 64, 16, 16)
    assert torch.equal(got[:, 1:], ref.permute(0, 2, 3, 1).reshape(1, 256, 64))
    assert torch.equal(got[:, 0], pos[:, 0])
    mine = D.interpolate_pos_embed(pos.float())                      # the engine's, in fp32 as upstream
    assert torch.equal(mine[:, 0], pos[:, 0].float())
    # fp32 source coordinates up to 37 carry ~37 * 2^-24 = 2e-6 of error; the cubic weights have slope <= 1.5 and four taps of up to
    # max|pos| add up: 2e-6 * 1.5 * 4 * max|pos| = 1.2e-5 max|pos|, next to which fp32 rounding of the products is small
    assert (mine.double() - got).abs().max().item() < 2e-5 * pos.abs().max().item()


@pytest.mark.parametrize("arch", ["vits14", "vitb14", "vitl14"])
def test_arch_inference(arch):
    dim, depth, heads = D.ARCHS[arch]
    sd = D.synth_weights(0, arch, depth=2)
    assert D.check_state_dict(sd) == (dim, 2, heads, 37 * 37)
    shapes = D.param_shapes(dim, depth)
    assert sum(1 for k in shapes if k.endswith("attn.qkv.weight")) == depth


def test_loader_key_spellings_and_strictness():
    sd = D.synth_weights(0, "vits14", depth=2)
    chunked = {(k.replace("blocks.", "blocks.0.", 1) if k.startswith("blocks.") else k): v for k, v in sd.items()}
    assert "blocks.0.1.attn.qkv.weight" in chunked
    a, b = D.fold_weights(sd), D.fold_weights(chunked)
    assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)
    assert "mask_token" in sd                                           # accepted and ignored
    missing = {k: v for k, v in sd.items() if k != "blocks.1.ls2.gamma"}
    with pytest.raises(ValueError, match="missing keys.*blocks.1.ls2.gamma"):
        D.check_state_dict(missing)
    extra = dict(sd, **{"blocks.0.attn.q_norm.weight": torch.zeros(64)})
    with pytest.raises(ValueError, match="unexpected keys.*q_norm"):
        D.check_state_dict(extra)
    bad = dict(sd, **{"blocks.0.mlp.fc1.weight": torch.zeros(1536, 385)})
    with pytest.raises(ValueError, match="fc1.weight has shape"):
        D.check_state_dict(bad)
    with pytest.raises(ValueError, match="missing keys"):
        D.DinoV2.from_state_dict(missing)


def test_loader_refusals():
    sd = D.synth_weights(0, "vits14", depth=1)
    swiglu = {k: v for k, v in sd.items() if ".mlp." not in k}
    swiglu["blocks.0.mlp.w12.weight"], swiglu["blocks.0.mlp.w3.weight"] = torch.zeros(2048, 384), torch.zeros(384, 1024)
    with pytest.raises(ValueError, match="SwiGLU"):
        D.check_state_dict(swiglu)
    with pytest.raises(ValueError, match="register"):
        D.check_state_dict(dict(sd, register_tokens=torch.zeros(1, 4, 384)))
    with pytest.raises(ValueError, match="head_dim"):
        D.check_state_dict(sd, num_heads=12)                             # 384 / 12 = 32
    odd = {k: v[..., :320] if k in ("cls_token", "pos_embed") else v for k, v in sd.items()}
    with pytest.raises(ValueError, match="head_dim"):
        D.check_state_dict(odd)                                          # a width none of the three architectures has
    with pytest.raises(ValueError, match="unknown DINOv2 arch"):
        D.synth_weights(0, "vitg14")


def test_folding():
    sd = D.synth_weights(3, "vits14", depth=2)
    f = D.fold_weights(sd)
    g = torch.Generator().manual_seed(4)
    for i in range(2):
        for lin, ls, q, k in (("attn.proj", "ls1", "proj", 384), ("mlp.fc2", "ls2", "fc2", 1536)):
            x = torch.randn(5, k, generator=g, dtype=torch.float64)
            w, b, gam = (sd[f"blocks.{i}.{n}"].double() for n in (lin + ".weight", lin + ".bias", ls + ".gamma"))
            ref = gam * (x @ w.T + b)
            wf = (gam[:, None] * w)                                      # the fold in float64 ...
            assert (x @ wf.T + gam * b - ref).abs().max().item() < 1e-12 * ref.abs().max().item()
            assert torch.equal(f[f"{i}.{q}.w"], wf.float()) and torch.equal(f[f"{i}.{q}.b"], (gam * b).float())   # ... then fp32
    pw = f["patch.w"]
    assert tuple(pw.shape) == (384, 640) and f["patch.w"].dtype == torch.float32
    assert int((pw != 0).any(dim=0).sum()) == 588 and bool((pw[:, 588:] == 0).all())
    orig = sd["patch_embed.proj.weight"].reshape(384, 588)
    assert torch.equal(torch.sort(pw[:, :588], dim=1).values, torch.sort(orig, dim=1).values)
    # the K order is the patchify order of the oracle: the padded product equals the conv
    x = torch.randn(1, 3, 224, 224, generator=g, dtype=torch.float64)
    conv = F.conv2d(x, sd["patch_embed.proj.weight"].double(), None, stride=14).flatten(2).transpose(1, 2)
    assert (O.patchify(x) @ pw[:, :588].double().T - conv).abs().max().item() < 1e-12
    assert tuple(f["pos"].shape) == (257, 384) and tuple(f["cls"].shape) == (384,)


def test_cpu_is_refused_and_inputs_are_checked():
    m = D.DinoV2.from_synthetic(0, "vits14", depth=1)
    with pytest.raises(ValueError, match="GPU only"):
        m.to("cpu")
    with pytest.raises(ValueError):
        m(torch.zeros(1, 3, 224, 200))
    with pytest.raises(ValueError, match="square"):
        m.features_u8(np.zeros((1, 64, 80, 3), np.uint8))
    with pytest.raises(ValueError, match="taps"):
        m.features_u8(np.zeros((1, 2048, 2048, 3), np.uint8))
    with pytest.raises(ValueError):
        D.DinoV2.from_synthetic(0, torch_dtype=torch.float32)
    assert D.resize_taps(768) == 15 and D.resize_taps(512) == 11 and D.resize_taps(100) == 5


def test_resize_rejects_large_reductions_on_the_host(lib):
    # argument validation happens before any HIP call, so it is testable without a GPU
    assert lib.idb_resize_bicubic_aa_u8(0x1000, 1, 2048, 224, 0x1000, None) == -1
    assert b"taps" in lib.idb_last_error()
    assert lib.idb_vit_patchify(0x1000, 1, 1, 0x1000, 7, None) == -1
    assert lib.idb_vit_tokens(0x1000, 0x1000, 0x1000, 0x1000, 1, 256, 100, 1, None) == -1
    assert lib.idb_vit_head(0x1000, 257, 0, 384, 0x1000, 0x1000, 1e-6, 0x1000, 1, None) == -1


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_emulated_error_is_a_usable_bound(dtype):
    """The GPU tests require max|gpu - float64| <= 3 e_emul with e_emul = max|oracle(emulate=dtype) - oracle(float64)|.  That bound is
    neither vacuous nor unmeetable: e_emul is positive and far below the spread of the features."""
    sd = D.synth_weights(0, "vits14")
    x = O.to_tensor_normalized(O.smooth_images(1, seed=11, size=224))
    ref = O.forward(sd, x, 6)
    emu = O.forward(sd, x, 6, emulate=dtype)
    e = (emu - ref).abs().max().item()
    spread = ref.std().item()
    print(f"{dtype}: e_emul {e:.3e}, feature std {spread:.3f}, max|ref| {ref.abs().max().item():.3f}")
    assert 0.0 < e < 0.1 * spread
    assert math.isfinite(e)
