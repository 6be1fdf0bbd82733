"""CPU checks of the LoRA attention layer (faceposegenerator_amd/loraattn.py) and its float64 oracle (tests/loraattn_oracle.py): the
closed-form oracle against torch autograd, the adapter key names and the save / load round trip, the transposed-merge identity the
input-gradient GEMMs rest on, and the constructor's and the layer's refusals."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loraattn_oracle as O  # noqa: E402
from faceposegenerator_amd import _lib as L, weights as W  # noqa: E402
from faceposegenerator_amd.loraattn import NAMES, LoRAAttention  # noqa: E402


def _layer(context_dim=None, trained=True, rank=4, alpha=None, seed=5):
    layer = LoRAAttention.from_synthetic(seed, 128, context_dim, rank, alpha).init_adapters(torch.Generator().manual_seed(seed + 1))
    if trained:
        g = torch.Generator().manual_seed(seed + 2)
        sd = layer.state_dict()
        layer.load_adapters({k: (v if "lora_A" in k else torch.randn(v.shape, generator=g) * 0.05) for k, v in sd.items()})
    return layer


def _sd(layer):
    sd = {f"{layer.prefix}.{n}.weight": layer.base[n] for n in NAMES}
    sd[f"{layer.prefix}.to_out.0.bias"] = layer.bias
    return sd


@pytest.mark.parametrize("context_dim", [None, 192])
@pytest.mark.parametrize("trained", [False, True])
def test_oracle_matches_autograd(context_dim, trained):
    """Closed form against autograd (unmerged adapters, F.scaled_dot_product_attention), float64, 1e-12 relative per tensor."""
    layer = _layer(context_dim, trained, rank=5, alpha=10.0)
    g = torch.Generator().manual_seed(9)
    x = torch.randn(2, 37, 128, generator=g, dtype=torch.float64)
    ctx = None if context_dim is None else torch.randn(2, 11, context_dim, generator=g, dtype=torch.float64)
    go = torch.randn(2, 37, 128, generator=g, dtype=torch.float64)
    a = O.run(_sd(layer), layer.prefix, layer.state_dict(), layer.scaling, x, ctx, go)
    b = O.autograd_layer(_sd(layer), layer.prefix, layer.state_dict(), layer.scaling, x, ctx, go)
    assert set(a) == set(b) and len(a) == 12
    for k in a:
        if a[k] is None:
            assert b[k] is None and context_dim is None
            continue
        assert O.deviation(a[k], b[k]) < 1e-12, (k, O.deviation(a[k], b[k]))
    if not trained:      # upstream's initial state: B = 0, so every lora_A gradient vanishes and no lora_B gradient does
        for n in NAMES:
            assert not a[f"{layer.prefix}.{n}.lora_A.weight"].any() and a[f"{layer.prefix}.{n}.lora_B.weight"].abs().max() > 0


def test_state_dict_keys_and_round_trip(tmp_path):
    layer = _layer(192)
    sd = layer.state_dict()
    assert set(sd) == {f"{layer.prefix}.{n}.lora_{ab}.weight" for n in NAMES for ab in "AB"}
    assert set(W.normalize_lora_keys(sd)) == set(sd)                       # already normalized: the keys load_lora_weights takes
    raw = {"unet." + k.replace(".lora_A.weight", ".lora.down.weight").replace(".lora_B.weight", ".lora.up.weight"): v for k, v in sd.items()}
    assert set(W.normalize_lora_keys(raw)) == set(sd)                      # and what the reference's checkpoints normalize to
    path = W.save_lora(str(tmp_path), sd)
    back, alphas = W.load_lora(path)
    assert alphas == {} and set(back) == set(sd)
    for k in sd:
        assert torch.equal(back[k], sd[k]) and back[k].dtype == torch.float32
    again = LoRAAttention.from_state_dict(_sd(layer), layer.prefix, back)
    assert again.rank == layer.rank and again.context_dim == 192 and again.scaling == 1.0
    for k, v in again.state_dict().items():
        assert torch.equal(v, sd[k])
    # init_adapters: upstream's gaussian init
    fresh = LoRAAttention.from_synthetic(3, 128, None, 8).init_adapters(torch.Generator().manual_seed(1))
    assert not any(v.any() for k, v in fresh.state_dict().items() if "lora_B" in k)
    a = fresh.state_dict()[f"{fresh.prefix}.to_q.lora_A.weight"]
    assert a.shape == (8, 128) and 0.8 / 8 < float(a.std()) < 1.2 / 8


def test_transposed_merge_identity():
    """(W + s B A)^T = W^T + s A^T B^T: idb_lora_merge given W^T with lora_b := A^T and lora_a := B^T builds the input-gradient operand."""
    g = torch.Generator().manual_seed(2)
    w, a, b, s = (torch.randn(96, 160, generator=g, dtype=torch.float64), torch.randn(5, 160, generator=g, dtype=torch.float64),
                  torch.randn(96, 5, generator=g, dtype=torch.float64), 0.75)
    merge = lambda w_, lora_a, lora_b: w_ + s * lora_b @ lora_a           # noqa: E731  (idb_lora_merge's definition)
    assert (merge(w, a, b).T - merge(w.T, b.T, a.T)).abs().max() < 1e-13


def test_refusals():
    sd = _sd(_layer())
    p = "mid_block.attentions.0.transformer_blocks.0.attn1"
    for kw, text in ((dict(channels=96), "multiple of 64"), (dict(channels=0), "multiple of 64"), (dict(channels=128, rank=0), "rank"),
                     (dict(channels=128, rank=L.IDB_LORA_MAX_RANK + 1), "rank"), (dict(channels=128, context_dim=100), "context_dim"),
                     (dict(channels=192), "expected")):
        with pytest.raises(ValueError, match=text):
            LoRAAttention(sd, p, **kw)
    layer = _layer()
    with pytest.raises(ValueError, match="HIP device"):
        layer.to("cpu")
    with pytest.raises(L.IdbError, match="no CPU fallback"):
        layer(torch.zeros(1, 4, 128, dtype=torch.float16))
    # context given to a self-attention layer (and none to a cross-attention layer): refused before any device work
    layer.device, layer.dtype = torch.device("cpu"), torch.float16
    with pytest.raises(ValueError, match="takes no context"):
        layer(torch.zeros(1, 4, 128, dtype=torch.float16), torch.zeros(1, 4, 128, dtype=torch.float16))
    cross = _layer(192)
    cross.device, cross.dtype = torch.device("cpu"), torch.float16
    with pytest.raises(ValueError, match="needs a context"):
        cross(torch.zeros(1, 4, 128, dtype=torch.float16))
    with pytest.raises(ValueError, match="expected rank"):
        _layer().load_adapters(_layer(rank=8).state_dict())
