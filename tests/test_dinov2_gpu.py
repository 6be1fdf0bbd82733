"""DINOv2 on the GPU against tests/dinov2_oracle.py (float64): the Pillow-exact bicubic resize, the patchify / token / head kernels,
one transformer block teacher-forced, the full network and features_u8 end to end, in f16 and bf16 with synthetic weights.

The network comparisons take no tolerance constant.  For the inputs at hand the test computes e_emul = max|oracle(emulate=dtype) -
oracle(float64)|, the error of storing every intermediate tensor in the operand dtype (test_dinov2_cpu.py shows it is positive and far
below the features' spread), and requires max|gpu - float64| <= 3 e_emul over every element: the factor covers what the emulation does
not model — MFMA accumulation order, the fp32 online softmax with its operand-dtype probabilities, fp32 LayerNorm statistics."""
import functools
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dinov2_oracle as O  # noqa: E402

from faceposegenerator_amd import _lib  # noqa: E402
from faceposegenerator_amd import dinov2 as D  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.float16, torch.bfloat16]
FACTOR = 3.0
NTOK = 257


@functools.lru_cache(maxsize=None)
def weights(arch, depth):
    return D.synth_weights(0, arch, depth)


@functools.lru_cache(maxsize=None)
def net_input():
    """Normalised float32 [3,3,224,224] (what model(x) takes) from smooth images."""
    return O.to_tensor_normalized(O.smooth_images(3, seed=5, size=224)).float()


@functools.lru_cache(maxsize=None)
def full_ref(emulate):
    return O.forward(weights("vits14", None), net_input().double(), 6, emulate)


@functools.lru_cache(maxsize=None)
def tokens_ref(arch, emulate):
    return O.patch_tokens(weights(arch, None if arch == "vits14" else 1), net_input()[:2].double(), emulate)


@functools.lru_cache(maxsize=None)
def u8_images():
    return O.smooth_images(5, seed=4, size=512)


@functools.lru_cache(maxsize=None)
def u8_ref(emulate):
    return O.features_u8(weights("vits14", None), u8_images(), 6, emulate)


@pytest.fixture(scope="module", params=DTYPES, ids=["f16", "bf16"])
def model(request):
    return D.DinoV2.from_state_dict(weights("vits14", None), request.param).to(DEV)


@pytest.fixture(scope="module", params=DTYPES, ids=["f16", "bf16"])
def large_block(request):
    return D.DinoV2.from_state_dict(weights("vitl14", 1), request.param).to(DEV)


def _check(name, got, ref, emu):
    """max|got - ref| <= FACTOR * max|emu - ref| over every element; prints both relative to max|ref|."""
    got = got.detach().double().cpu().reshape(ref.shape)
    scale = ref.abs().max().item()
    e_emul = (emu - ref).abs().max().item()
    err = (got - ref).abs().max().item()
    print(f"{name}: max|gpu - f64| {err:.3e} ({err / scale:.3e} of max|ref|), e_emul {e_emul:.3e} ({e_emul / scale:.3e}), ratio {err / e_emul:.2f}")
    assert bool(torch.isfinite(got).all())
    assert e_emul > 0.0
    assert err <= FACTOR * e_emul, (name, err, e_emul)


@pytest.mark.parametrize("s", [512, 768, 250, 224, 100])
def test_resize_bit_exact_with_pillow(s):
    imgs = np.random.default_rng(s * 7).integers(0, 256, (3, s, s, 3), dtype=np.uint8)
    m = D.DinoV2.from_state_dict(weights("vits14", 1)).to(DEV)
    got = m.resize(torch.from_numpy(imgs).to(DEV)).cpu().numpy()
    for i in range(3):
        ref = np.asarray(Image.fromarray(imgs[i]).resize((224, 224), Image.BICUBIC))
        assert np.array_equal(got[i], ref), (s, i, int((got[i] != ref).sum()))


def test_resize_refuses_what_needs_more_taps():
    m = D.DinoV2.from_state_dict(weights("vits14", 1)).to(DEV)
    before = m.lib.idb_launch_count()
    with pytest.raises(_lib.IdbError, match="taps"):
        m.resize(torch.zeros((1, 2048, 2048, 3), dtype=torch.uint8, device=DEV))
    assert m.lib.idb_launch_count() == before
    with pytest.raises(ValueError, match="taps"):
        m.features_u8(torch.zeros((1, 2048, 2048, 3), dtype=torch.uint8, device=DEV))


def _ulp(ref, dtype):
    """Spacing of dtype's values at |ref| (float64 tensor)."""
    bits, emin = (10, -14) if dtype == torch.float16 else (7, -126)
    e = torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** emin))).clamp_min(emin)
    return torch.pow(2.0, e - bits)


def test_patchify(model):
    imgs = O.smooth_images(2, seed=9, size=224)
    imgs[1] = np.random.default_rng(1).integers(0, 256, (224, 224, 3), dtype=np.uint8)
    x64 = O.to_tensor_normalized(imgs)
    ref = O.patchify(x64).reshape(2 * 256, 588)
    got = model.patchify(torch.from_numpy(imgs).to(DEV), True).double().cpu()
    assert tuple(got.shape) == (512, 640)
    assert bool((got[:, 588:] == 0).all())
    assert bool(((got[:, :588] - ref).abs() <= _ulp(ref, model.tdt)).all())
    x32 = x64.float()
    got = model.patchify(x32.to(DEV), False).double().cpu()
    ref = O.patchify(x32.double()).reshape(512, 588)
    assert bool((got[:, 588:] == 0).all())
    assert bool(((got[:, :588] - ref).abs() <= _ulp(ref, model.tdt)).all())
    # row order: patch (i, j) is the constant 16 i + j
    idx = (torch.arange(16).view(16, 1) * 16 + torch.arange(16).view(1, 16)).to(torch.uint8)
    img = idx.repeat_interleave(14, 0).repeat_interleave(14, 1).view(1, 224, 224, 1).expand(1, 224, 224, 3).contiguous().numpy()
    got = model.patchify(torch.from_numpy(img).to(DEV), True).double().cpu()
    want = O.to_tensor_normalized(idx.view(1, 256, 1, 1).expand(1, 256, 1, 3).contiguous().numpy())     # [1][3][256][1]
    want = want[0, :, :, 0].T.repeat_interleave(196, 1)                                                  # [256][588]
    assert bool(((got[:, :588] - want).abs() <= _ulp(want, model.tdt)).all())


def test_patch_embed_and_tokens(model):
    got = model.patch_tokens(net_input()[:2].to(DEV), False)
    assert tuple(got.shape) == (2 * NTOK, 384)
    _check(f"tokens {model.tdt}", got, tokens_ref("vits14", None), tokens_ref("vits14", model.tdt))


@pytest.mark.parametrize("dim", [384, 1024])
def test_head_crafted(model, dim):
    """idb_vit_head on a constant row, a row with one large outlier and a generic row, every other row of x NaN: fp32 LayerNorm of at
    most 1024 terms against float64 within 1e-5 max|ref|."""
    g = torch.Generator().manual_seed(dim)
    stride = 5
    x = torch.full((3 * stride, dim), float("nan"))
    x[0] = 0.7
    x[stride] = torch.randn(dim, generator=g)
    x[stride, 17] = 1000.0
    x[2 * stride] = 3.0 * torch.randn(dim, generator=g) + 1.5
    xd = x.to(DEV, model.tdt)
    gamma = (0.5 + torch.rand(dim, generator=g)).to(DEV)
    beta = (0.1 * torch.randn(dim, generator=g)).to(DEV)
    out = torch.empty((3, dim), device=DEV)
    _lib.check(model.lib.idb_vit_head(xd.data_ptr(), stride, 3, dim, gamma.data_ptr(), beta.data_ptr(), 1e-6, out.data_ptr(), model.dt,
                                      model._stream()), "idb_vit_head")
    rows = xd[::stride].double().cpu()
    ref = torch.nn.functional.layer_norm(rows, (dim,), gamma.double().cpu(), beta.double().cpu(), 1e-6)
    err = (out.double().cpu() - ref).abs().max().item()
    print(f"head D={dim} {model.tdt}: max-abs {err:.3e}, max|ref| {ref.abs().max().item():.3f}")
    assert err <= 1e-5 * ref.abs().max().item()
    assert torch.equal(out[0], beta)                         # a constant row has an exact mean


def _block_case(m, arch, heads, batch):
    """Block 0 on the oracle's float64 tokens rounded to the operand dtype: M = 257 and 514 rows (a row tail on the GEMM M side and on
    the attention query and key sides)."""
    sd = weights(arch, None if arch == "vits14" else 1)
    xin = tokens_ref(arch, None)[:batch].to(m.tdt)
    x64 = xin.double()
    ref = O.block(sd, 0, x64, heads)
    emu = O.block(sd, 0, x64, heads, emulate=m.tdt)
    got = m.block(0, xin.reshape(batch * NTOK, m.dim).to(DEV).contiguous())
    _check(f"block D={m.dim} B={batch} {m.tdt}", got, ref, emu)


@pytest.mark.parametrize("batch", [1, 2])
def test_one_block_teacher_forced_d384(model, batch):
    _block_case(model, "vits14", 6, batch)


@pytest.mark.parametrize("batch", [1, 2])
def test_one_block_teacher_forced_d1024(large_block, batch):
    _block_case(large_block, "vitl14", 16, batch)


@pytest.mark.parametrize("batch", [3, 1])
def test_full_net_against_oracle(model, batch):
    got = model(net_input()[:batch].to(DEV))
    assert got.dtype == torch.float32 and tuple(got.shape) == (batch, 384)
    _check(f"full vits14 B={batch} {model.tdt}", got, full_ref(None)[:batch], full_ref(model.tdt)[:batch])


def test_features_u8_end_to_end(model):
    model.chunk = 2
    try:
        got = model.features_u8(u8_images())
        again = model.features_u8(torch.from_numpy(u8_images()).to(DEV))
    finally:
        model.chunk = 64
    assert tuple(got.shape) == (5, 384)
    assert torch.equal(got, again)
    _check(f"features_u8 {model.tdt}", got, u8_ref(None), u8_ref(model.tdt))
    with pytest.raises(ValueError, match="square"):
        model.features_u8(np.zeros((1, 64, 80, 3), np.uint8))
