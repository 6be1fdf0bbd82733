"""The exact number of kernel launches of one UNet forward (``HipEngine.last_forward_launches``) per engine configuration.  Which
launch runs where is decided on the host (plan queries, the IDB_* switches, the statistics hand-off), so the count is
deterministic: a change in it means a fused path was lost or a launch was added, long before an output tolerance notices."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# Batch 2, 77 context tokens, 16x16 latents: at this side the reduced graph takes both forms of the norm-to-conv pairs that it can
# reach — conv1 over cat[x, skip] fused 6 times and unfused 6, Transformer2DModel.norm + proj_in fused 10 and unfused 6, single-source
# resnet convs fused 7 and unfused 11.  conv2 with a shortcut segment is asked 14 times and fuses nowhere (nor at 32x32, nor in the
# full-size CFG forward at batch 1).
SIDE = 16
SWITCHES = ("IDB_GN_SYNC", "IDB_GN_FUSE", "IDB_LN_FOLD", "IDB_FF_CHUNK_MB", "IDB_GN_EPILOGUE", "IDB_GN_CONV", "IDB_GN_CONV_RESNET",
            "IDB_GN_CONV_MAX_C", "IDB_W_TILED")

# case: (dtype, switches set before construction, LoRA groups)
CASES = {
    "f16": ("f16", {}, 0),
    "bf16": ("bf16", {}, 0),
    "fp8": ("fp8", {}, 0),
    "gn_conv_off": ("f16", {"IDB_GN_CONV": "0"}, 0),
    "gn_conv_resnet_off": ("f16", {"IDB_GN_CONV_RESNET": "0"}, 0),
    "ln_fold_off": ("f16", {"IDB_LN_FOLD": "0"}, 0),
    "gn_fuse_off": ("f16", {"IDB_GN_FUSE": "0"}, 0),
    "lora_groups": ("f16", {}, 2),
}
# measured on the MI355X at commit cec1a66 (the last one before the host engine's norm-to-conv paths were merged into one)
EXPECTED = {"f16": 337, "bf16": 337, "fp8": 355, "gn_conv_off": 360, "gn_conv_resnet_off": 350, "ln_fold_off": 385, "gn_fuse_off": 361,
            "lora_groups": 379}


@pytest.fixture(scope="module")
def unet_sd():
    from faceposegenerator_amd import spec as S, weights as W
    return W.synth_unet(S.TINY_UNET, 7)


def forward_launches(case: str, unet_sd, side: int, setenv, delenv) -> int:
    from faceposegenerator_amd import spec as S, weights as W
    from faceposegenerator_amd.engine import HipEngine
    dtype, env, groups = CASES[case]
    for name in SWITCHES:                       # read in HipEngine.__init__
        delenv(name, raising=False)
    for name, value in env.items():
        setenv(name, value)
    ucfg = S.TINY_UNET
    eng = HipEngine(ucfg, S.TINY_VAE, unet_sd, None, DEV, dtype)
    if groups:
        eng.set_lora_groups([W.normalize_lora_keys(W.synth_lora(ucfg, seed=3 + i)) for i in range(groups)])
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 4, side, side, generator=g)
    ctx = torch.randn(2, 77, ucfg.cross_attention_dim, generator=g)
    out = eng.unet_forward(x, 501, ctx)
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()
    return eng.last_forward_launches


@pytest.mark.parametrize("case", list(CASES))
def test_unet_forward_launch_count(lib, unet_sd, monkeypatch, case):
    n = forward_launches(case, unet_sd, SIDE, monkeypatch.setenv, monkeypatch.delenv)
    print(f"{case}: {n} launches")
    assert n == EXPECTED[case]
