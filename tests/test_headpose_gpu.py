"""6DRepNet head pose on the GPU: idb_gemm's ReLU epilogue (act = 3) bitwise against act = 0 + torch.relu over tile families and
split-K factors, grouped convs as per-group launches, the Pillow-exact resize, the stem, the head, and the full network with
synthetic weights against tests/headpose_oracle.py (bounds from test_headpose_cpu.py's emulated-autocast figures)."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import headpose_oracle as O  # noqa: E402

from faceposegenerator_amd import _lib  # noqa: E402
from faceposegenerator_amd import headpose as H  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.float16, torch.bfloat16]
BOUNDS = {torch.float16: (1.5e-3, 0.1), torch.bfloat16: (1.2e-2, 0.6)}      # (R max-abs, angle max-abs in degrees)


@pytest.fixture(scope="module")
def sd():
    return {k: v.float() for k, v in H.deploy_state_dict(H.synth_weights(0)).items()}


@pytest.fixture(scope="module", params=DTYPES, ids=["f16", "bf16"])
def model(request):
    return H.HeadPose.from_synthetic(0, request.param).to(DEV)


def _conv_case(m, B, Hh, cin, n, stride, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, Hh, Hh, cin, generator=g).to(DEV, m.tdt)
    w = (torch.randn(n, 9 * cin, generator=g) * (2.0 / (9 * cin)) ** 0.5).to(DEV, m.tdt)
    b = (0.1 * torch.randn(n, generator=g)).to(DEV)
    oh = (Hh + stride - 1) // stride
    return x, w, b, oh


def _run(m, x, w, b, n, oh, stride, act, split_k=0, tile=0):
    out = torch.empty((x.shape[0], oh, oh, n), dtype=m.tdt, device=DEV)
    m.gemm(x.data_ptr(), x.shape[3], x.shape[1], x.shape[2], x.shape[0], w.data_ptr(), b.data_ptr(), n, out.data_ptr(), n, stride, act,
           split_k, tile)
    return out


# tiles of each family the planner picks for the pose layers (2-stage ring 9, loader waves 74 / 79, 256-row loader waves 89) plus the
# other ring / loader-wave families on the same shapes; split-K forced through {1, 2, 4, 8}
RELU_CASES = [(1, 14, 512, 512, 1), (1, 28, 256, 256, 1), (64, 14, 256, 256, 1), (4, 56, 128, 128, 1), (2, 28, 256, 512, 2)]
TILES = [0, 9, 19, 29, 2, 74, 79, 57, 69, 89]


# (tile, split) pairs the planner accepts for every case: TILES x {0, 1, 2, 4, 8} but tile id 29, which is not built
RELU_RAN = 45


def _plans(m, B, Hh, cin, n, stride, act, sk, tile):
    """idb_gemm_plan's answer for the descriptor HeadPose.gemm would build (host-only: nothing is launched)."""
    import ctypes as C
    from faceposegenerator_amd import _lib as L
    d = L.GemmDesc()
    oh = (Hh + stride - 1) // stride
    d.dtype, d.batch, d.out_h, d.out_w, d.stride, d.n, d.nsrc = m.dt, B, oh, oh, stride, n, 1
    d.src[0].ptr, d.src[0].channels, d.src[0].taps, d.src[0].in_h, d.src[0].in_w = 1 << 20, cin, 9, Hh, Hh
    d.w, d.bias, d.out, d.out_dtype, d.out_ld = 1 << 20, 1 << 20, 1 << 20, m.dt, n
    d.act, d.split_k, d.tile = act, sk, tile
    return m.lib.idb_gemm_plan(C.byref(d), None, None, None) == 0


@pytest.mark.parametrize("case", RELU_CASES)
def test_relu_epilogue_bitwise(model, case):
    B, Hh, cin, n, stride = case
    x, w, b, oh = _conv_case(model, B, Hh, cin, n, stride)
    ran = 0
    for tile in TILES:
        for sk in (0, 1, 2, 4, 8):
            ok = _plans(model, B, Hh, cin, n, stride, 3, sk, tile)
            assert ok == _plans(model, B, Hh, cin, n, stride, 0, sk, tile), (tile, sk)   # the ReLU twin exists wherever the plain kernel runs
            if not ok:
                continue                                       # this tile is not built
            ref = torch.relu(_run(model, x, w, b, n, oh, stride, 0, sk, tile))
            got = _run(model, x, w, b, n, oh, stride, 3, sk, tile)
            assert bool((got == ref).all()), (tile, sk)
            ran += 1
    assert ran == RELU_RAN


def test_grouped_conv(model):
    """Grouped 3x3 conv (groups 2) as two launches writing column halves of one tensor (out_ld = n) against F.conv2d(groups=2) in
    fp32 and, bitwise, against two dense launches into separate tensors."""
    B, Hh, c = 2, 28, 256
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, B, Hh, Hh, c // 2, generator=g).to(DEV, model.tdt)      # the split input: [G][B][H][W][c / 2]
    wt = torch.randn(c, c // 2, 3, 3, generator=g) * (2.0 / (9 * c / 2)) ** 0.5
    bt = 0.1 * torch.randn(c, generator=g)
    wp = wt.permute(0, 2, 3, 1).reshape(c, -1).to(DEV, model.tdt).contiguous()
    bd = bt.to(DEV)
    full = torch.empty((B, Hh, Hh, c), dtype=model.tdt, device=DEV)
    es, K = wp.element_size(), wp.shape[1]
    for q in range(2):
        model.gemm(x[q].data_ptr(), c // 2, Hh, Hh, B, wp.data_ptr() + q * (c // 2) * K * es, bd.data_ptr() + q * (c // 2) * 4, c // 2,
                   full.data_ptr() + q * (c // 2) * es, c, 1)
    for q in range(2):
        sep = _run(model, x[q], wp[q * (c // 2):(q + 1) * (c // 2)].contiguous(), bd[q * (c // 2):(q + 1) * (c // 2)].contiguous(), c // 2,
                   Hh, 1, 3)
        assert torch.equal(full[..., q * (c // 2):(q + 1) * (c // 2)], sep)
    xin = torch.cat([x[0], x[1]], dim=3).float().permute(0, 3, 1, 2).cpu()
    ref = F.relu(F.conv2d(xin, wp.float().cpu().view(c, 3, 3, c // 2).permute(0, 3, 1, 2), bt, 1, 1, groups=2)).permute(0, 2, 3, 1)
    err = (full.float().cpu() - ref).abs().max().item() / ref.abs().max().item()
    assert err < (4e-3 if model.tdt == torch.float16 else 2e-2), err


@pytest.mark.parametrize("s,pad", [(512, 30), (768, 30), (250, 0), (224, 30), (100, 30), (100, 0)])
def test_resize_bit_exact_with_pillow(s, pad):
    imgs = np.random.default_rng(s * 7 + pad).integers(0, 256, (3, s, s, 3), dtype=np.uint8)
    m = H.HeadPose.from_synthetic(0).to(DEV)
    got = m.resize(torch.from_numpy(imgs).to(DEV), pad).cpu().numpy()
    for i in range(3):
        ref = np.asarray(Image.fromarray(np.pad(imgs[i], ((pad, pad), (pad, pad), (0, 0)))).resize((224, 224), Image.BILINEAR))
        assert np.array_equal(got[i], ref), (s, pad, i, int((got[i] != ref).sum()))


def test_stem(model, sd):
    imgs = O.smooth_images(2, seed=9, size=224)
    ref = O.conv_block(sd, "layer0", O.to_tensor_normalized(imgs), 2, 1).permute(0, 2, 3, 1)
    got_u8 = model.stem(torch.from_numpy(imgs).to(DEV), True).float().cpu()
    got_f = model.stem(O.to_tensor_normalized(imgs).to(DEV).contiguous(), False).float().cpu()
    tol = 2e-3 if model.tdt == torch.float16 else 1.6e-2
    scale = ref.abs().max().item()
    assert (got_u8 - ref).abs().max().item() < tol * scale
    assert (got_f - ref).abs().max().item() < tol * scale


def test_head_crafted(model):
    """idb_pose_head on crafted features: the 6D output is set through linear_reg so that the cases include identity, a generic
    rotation, the singular branch (x column (0, 0, -1)) and a near-zero vector; fp64 reference of the same math."""
    six = torch.tensor([[1.0, 0, 0, 0, 1, 0], [0.3, -0.8, 0.5, 0.9, 0.2, -0.4], [0.0, 0, -1, 0, 1, 0], [1e-9, 0, 0, 0, 1, 0]])
    B = six.shape[0]
    x = torch.ones((B, 49, 2048), dtype=model.tdt, device=DEV)
    w = torch.zeros((6, 2048), device=DEV)
    bias = torch.zeros(6, device=DEV)
    R = torch.empty((B, 3, 3), device=DEV)
    ang = torch.empty((B, 3), device=DEV)
    for i in range(B):
        bias.copy_(six[i].to(DEV))
        _lib.check(model.lib.idb_pose_head(x[i:i + 1].data_ptr(), 1, 49, 2048, w.data_ptr(), bias.data_ptr(), R[i:i + 1].data_ptr(),
                                           ang[i:i + 1].data_ptr(), model.dt, model._stream()), "idb_pose_head")
    Rr = O.rotation_from_6d(six)
    ar = O.euler_from_rotation(Rr)
    assert (R.cpu().double() - Rr).abs().max().item() < 1e-6
    assert (ang.cpu().double() - ar).abs().max().item() < 1e-4
    assert ang[2, 2].item() == 0.0 and abs(ang[2, 1].item() - 90.0) < 1e-4
    # pooling + linear on random features against fp64
    g = torch.Generator().manual_seed(2)
    xf = torch.rand((3, 49, 2048), generator=g).to(DEV, model.tdt)
    wl = (torch.randn(6, 2048, generator=g) / 45.0).to(DEV)
    bl = torch.tensor([1.0, 0, 0, 0, 1, 0], device=DEV)
    R2 = torch.empty((3, 3, 3), device=DEV)
    a2 = torch.empty((3, 3), device=DEV)
    _lib.check(model.lib.idb_pose_head(xf.data_ptr(), 3, 49, 2048, wl.data_ptr(), bl.data_ptr(), R2.data_ptr(), a2.data_ptr(), model.dt,
                                       model._stream()), "idb_pose_head")
    o = xf.double().mean(1) @ wl.double().T + bl.double()
    assert (a2.cpu().double() - O.euler_from_rotation(O.rotation_from_6d(o.cpu()))).abs().max().item() < 1e-3


def test_full_net_against_oracle(model, sd):
    rb, ab = BOUNDS[model.tdt]
    x = O.to_tensor_normalized(np.stack([O.resize_pil_u8(im, 224, 30) for im in O.smooth_images()]))
    st_ref = []
    Rr, ar = O.forward(sd, x, None, st_ref)
    st = []
    feat = model.features(x.to(DEV).contiguous(), False, st)
    R, ang = model.head(feat)
    # per-stage teacher forcing: each stage run on the oracle's input to it, error relative to the stage's max
    errs = []
    bl = H.blocks()
    starts = [1] + [i for i, b in enumerate(bl) if b[0].endswith(".0") and i > 1] + [len(bl)]
    for s in range(4):
        xin = st_ref[s].permute(0, 2, 3, 1).to(DEV, model.tdt).contiguous()
        if bl[starts[s]][4] > 1:
            raise AssertionError("a stage starts with a grouped block")
        y = xin
        for i in range(starts[s], starts[s + 1]):
            y = model.block(i, y, i + 1 < len(bl) and bl[i + 1][4] > 1)
        ref = st_ref[s + 1].permute(0, 2, 3, 1)
        errs.append((y.float().cpu() - ref).abs().max().item() / ref.abs().max().item())
    print("stage errors", errs)
    tol = 1e-2 if model.tdt == torch.float16 else 6e-2
    assert all(e < tol for e in errs), errs
    Rm = model(x.to(DEV))
    assert torch.equal(Rm, R)
    rerr = (R.cpu().double() - Rr).abs().max().item()
    aerr = (ang.cpu().double() - ar).abs().max().item()
    print(f"{model.tdt}: R max-abs {rerr:.3e}, angle max-abs {aerr:.4f} deg")
    assert rerr < rb and aerr < ab, (rerr, aerr)


def test_predict_u8_end_to_end(model, sd):
    imgs = O.smooth_images(6, seed=4)
    p, y, r = model.predict_u8(imgs)
    _, ar = O.predict_u8(sd, imgs, 30)
    got = torch.stack([p, y, r], 1).cpu().double()
    assert got.shape == (6, 3)
    assert (got - ar).abs().max().item() < BOUNDS[model.tdt][1]
    with pytest.raises(ValueError):
        model.predict_u8(np.zeros((1, 64, 80, 3), np.uint8))


def test_deterministic(model):
    imgs = torch.from_numpy(O.smooth_images(3, seed=8)).to(DEV)
    a = model.predict_u8(imgs)
    b = model.predict_u8(imgs)
    assert all(torch.equal(u, v) for u, v in zip(a, b))


def test_batch_one(model, sd):
    imgs = O.smooth_images(1, seed=6)
    got = torch.stack(model.predict_u8(imgs), 1).cpu().double()
    _, ar = O.predict_u8(sd, imgs, 30)
    assert (got - ar).abs().max().item() < BOUNDS[model.tdt][1]
