"""6DRepNet head pose on CPU: the architecture table, the strict loader, the training-form -> deploy fold, the Pillow resize
restatement against the installed Pillow, the 6D head math, pose_summary, the emulated-autocast error that sets the GPU bounds, and
the host-side planning of idb_gemm's ReLU epilogue (act = 3; no GPU call is made)."""
import ctypes as C
import json
import math
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


def test_architecture_table():
    bl = H.blocks()
    assert len(bl) == 28
    assert bl[0] == ("layer0", 3, 64, 2, 1)
    assert [k for k, *_ in bl if k.endswith(".0")] == ["layer1.0", "layer2.0", "layer3.0", "layer4.0"]
    assert [i for i, b in enumerate(bl) if b[4] == 2] == list(range(2, 27, 2))
    assert [i for i, b in enumerate(bl) if b[3] == 2] == [0, 1, 5, 11, 27]
    assert bl[-1] == ("layer4.0", 512, 2048, 2, 1)
    assert round(H.gflops(), 1) == 17.6
    shapes = H.param_shapes()
    assert shapes["layer3.1.rbr_reparam.weight"] == (512, 256, 3, 3)          # groups = 2: cin / 2 per output channel
    assert shapes["layer3.2.rbr_reparam.weight"] == (512, 512, 3, 3)
    assert shapes["linear_reg.weight"] == (6, 2048)
    train = H.param_shapes(deploy=False)
    assert "layer1.1.rbr_identity.running_var" in train and "layer1.0.rbr_identity.weight" not in train
    assert "layer0.rbr_identity.weight" not in train and train["layer2.3.rbr_1x1.conv.weight"] == (256, 128, 1, 1)


def test_loader_is_strict(tmp_path):
    sd = H.synth_weights(1)
    H.check_state_dict(sd)
    H.check_state_dict({"module." + k: v for k, v in sd.items()})                 # DataParallel prefix
    H.check_state_dict({"model_state_dict": sd})                                   # wrapped checkpoint
    H.check_state_dict(H.synth_weights(1, deploy=False))
    bad = dict(sd)
    del bad["layer2.3.rbr_reparam.bias"]
    with pytest.raises(ValueError, match="layer2.3.rbr_reparam.bias"):
        H.check_state_dict(bad)
    bad = dict(sd)
    bad["layer5.0.rbr_reparam.weight"] = torch.zeros(1)
    with pytest.raises(ValueError, match="layer5.0.rbr_reparam.weight"):
        H.check_state_dict(bad)
    bad = dict(sd)
    bad["layer1.1.rbr_reparam.weight"] = torch.zeros(128, 128, 3, 3)              # a dense weight where groups = 2
    with pytest.raises(ValueError, match="layer1.1.rbr_reparam.weight"):
        H.check_state_dict(bad)
    tr = H.synth_weights(1, deploy=False)
    del tr["layer3.4.rbr_identity.running_mean"]
    with pytest.raises(ValueError, match="layer3.4.rbr_identity.running_mean"):
        H.HeadPose.from_state_dict(tr)
    with pytest.raises(ValueError):
        H.HeadPose.from_state_dict(sd, torch.float32)
    path = tmp_path / "6DRepNet.pth"
    torch.save(sd, path)
    m = H.HeadPose.from_pretrained(str(path))
    assert torch.equal(m._fw["layer4.0.w"], H.fold_weights(sd)["layer4.0.w"])


def test_fold_weights_layout():
    sd = H.synth_weights(2)
    f = H.fold_weights(sd)
    assert f["layer0.w"].shape == (64, 27) and f["layer1.1.w"].shape == (128, 9 * 64) and f["layer4.0.w"].shape == (2048, 9 * 512)
    w = sd["layer1.1.rbr_reparam.weight"]
    assert torch.equal(f["layer1.1.w"].view(128, 3, 3, 64), w.permute(0, 2, 3, 1).float())     # [n][ky][kx][cin / g]
    assert all(v.dtype == torch.float32 and v.is_contiguous() for v in f.values())


@pytest.mark.parametrize("idx", [0, 1, 2, 3, 12])
def test_training_form_fold_is_exact(idx):
    """RepVGG re-parameterisation in float64: the folded 3x3 conv + bias equals dense + 1x1 + identity branches with their BNs."""
    sd = H.synth_weights(3, deploy=False)
    key, cin, cout, stride, g = H.blocks()[idx]
    h = {0: 32, 1: 32, 2: 16, 3: 16, 12: 8}[idx]
    x = torch.randn(2, cin, h, h, generator=torch.Generator().manual_seed(idx), dtype=torch.float64)
    ref = O.block_train_form({k: v.double() for k, v in sd.items() if v.ndim > 0}, key, x, stride, g)
    d = H.deploy_state_dict(sd)
    got = F.conv2d(x, d[f"{key}.rbr_reparam.weight"], d[f"{key}.rbr_reparam.bias"], stride, 1, groups=g)
    assert (got - ref).abs().max().item() < 1e-10 * max(1.0, ref.abs().max().item())


@pytest.mark.parametrize("s", [512, 768, 250, 224, 100])
@pytest.mark.parametrize("pad", [30, 0])
def test_resize_restatement_is_bit_exact_with_pillow(s, pad):
    img = np.random.default_rng(s + pad).integers(0, 256, (s, s, 3), dtype=np.uint8)
    ref = np.asarray(Image.fromarray(np.pad(img, ((pad, pad), (pad, pad), (0, 0)))).resize((224, 224), Image.BILINEAR))
    assert np.array_equal(O.resize_pil_u8(img, 224, pad), ref)


def test_head_math():
    ident = torch.tensor([[1.0, 0, 0, 0, 1.0, 0]])
    R = O.rotation_from_6d(ident)
    assert torch.allclose(R, torch.eye(3, dtype=torch.float64)[None])
    assert O.euler_from_rotation(R).abs().max().item() == 0.0
    # Euler -> R -> first two columns as the 6D input -> Euler round-trips (regular branch, |yaw| < 90)
    g = torch.Generator().manual_seed(0)
    deg = torch.stack([torch.rand(64, generator=g) * 340 - 170, torch.rand(64, generator=g) * 170 - 85, torch.rand(64, generator=g) * 340 - 170], 1)
    R = O.rotation_from_euler(deg)
    six = torch.cat([R[:, :, 0] * 2.5, R[:, :, 1] * 0.7 + R[:, :, 0] * 0.3], dim=1)          # unnormalised, not orthogonal: Gram-Schmidt fixes it
    back = O.euler_from_rotation(O.rotation_from_6d(six))
    assert (back - deg.double()).abs().max().item() < 1e-9
    # singular branch: x column = (0, 0, -1) gives sy = 0, roll = 0, yaw = +90
    R = O.rotation_from_6d(torch.tensor([[0.0, 0, -1, 0, 1, 0]]))
    e = O.euler_from_rotation(R)
    assert abs(e[0, 1].item() - 90.0) < 1e-9 and e[0, 2].item() == 0.0 and abs(e[0, 0].item()) < 1e-9
    # near-zero-norm input: the 1e-8 floor keeps the result finite
    R = O.rotation_from_6d(torch.tensor([[1e-12, 0, 0, 0, 1e-12, 0], [0.0, 0, 0, 0, 0, 0]]))
    assert torch.isfinite(R).all() and torch.isfinite(O.euler_from_rotation(R)).all()


def test_pose_summary():
    names = ["3_a.png", "3_b.png", "12_x.png"]
    s = H.pose_summary(names, torch.tensor([1.0, 2.0, 3.0]), np.array([4.0, 5.0, 6.0]), [7.0, 8.0, 9.0])
    assert s == {"yaw": [4.0, 5.0, 6.0], "yaw_per_id": {"3": [4.0, 5.0], "12": [6.0]}, "pitch": [1.0, 2.0, 3.0],
                 "pitch_per_id": {"3": [1.0, 2.0], "12": [3.0]}, "roll": [7.0, 8.0, 9.0], "roll_per_id": {"3": [7.0, 8.0], "12": [9.0]}}
    json.dumps(s)
    with pytest.raises(ValueError):
        H.pose_summary(names[:2], [1.0], [1.0], [1.0])


def test_synthetic_net_and_emulated_autocast_error():
    """The bounds of the GPU end-to-end tests are set from this emulation (batch 4 of O.smooth_images(), synthetic seed 0, pad 30).
    Measured: activation RMS per stage 1.07 / 0.83 / 0.67 / 0.53 / 0.52 (no vanishing or explosion over 28 ReLU layers); angles
    -31..-25 / 8..9 / 23..27 deg (pitch / yaw / roll), well away from 0; emulated fp16 autocast vs fp32: R max-abs 3.2e-4, angles
    0.021 deg; bf16: 4.0e-3, 0.19 deg.  GPU bounds (test_headpose_gpu.py): f16 R 1.5e-3 / 0.1 deg, bf16 R 1.2e-2 / 0.6 deg (about
    3-5x the emulation)."""
    sd = {k: v.float() for k, v in H.deploy_state_dict(H.synth_weights(0)).items()}
    st = []
    x = O.to_tensor_normalized(np.stack([O.resize_pil_u8(im, 224, 30) for im in O.smooth_images()]))
    R, a = O.forward(sd, x, None, st)
    rms = [s.pow(2).mean().sqrt().item() for s in st]
    assert len(rms) == 5 and all(0.1 < r < 3.0 for r in rms), rms
    assert a.abs().max().item() > 5.0 and a.std(dim=0).max().item() > 0.3
    for em, rb, ab in ((torch.float16, 1.5e-3, 0.1), (torch.bfloat16, 1.2e-2, 0.6)):
        R2, a2 = O.forward(sd, x, em)
        assert (R2 - R).abs().max().item() < rb / 2 and (a2 - a).abs().max().item() < ab / 2


# ---- idb_gemm act = 3 planning (host only) ---------------------------------------------------------------------------------
def _desc(B, H_, cin, n, stride=1, act=3, split_k=0, tile=0, dt=1):
    d = _lib.GemmDesc()
    d.dtype, d.batch, d.stride, d.n, d.nsrc = dt, B, stride, n, 1
    d.out_h, d.out_w = (H_ + stride - 1) // stride, (H_ + stride - 1) // stride
    d.src[0].ptr, d.src[0].channels, d.src[0].taps, d.src[0].in_h, d.src[0].in_w = 4096, cin, 9, H_, H_
    d.w, d.bias, d.out, d.out_dtype, d.out_ld = 4096, 4096, 4096, dt, n
    d.act, d.split_k, d.tile = act, split_k, tile
    return d


def _plan(d):
    lib = _lib.load()
    t, s, b = C.c_int32(), C.c_int32(), C.c_int32()
    rc = lib.idb_gemm_plan(C.byref(d), C.byref(t), C.byref(s), C.byref(b))
    return rc, t.value, s.value, b.value


POSE_GEMMS = [(112, 64, 128, 2), (56, 64, 64, 1), (56, 128, 128, 1), (56, 128, 256, 2), (28, 128, 128, 1), (28, 256, 256, 1),
              (28, 256, 512, 2), (14, 256, 256, 1), (14, 512, 512, 1), (14, 512, 2048, 2)]


@pytest.mark.parametrize("B", [1, 64, 256])
def test_relu_plans_like_no_activation(B):
    """act = 3 keeps the plan of act = 0 on every pose layer (same tile, same split-K: ReLU does not disable the split), and the
    batch-1 stage 3/4 layers do run split-K."""
    for H_, cin, n, st in POSE_GEMMS:
        p3, p0 = _plan(_desc(B, H_, cin, n, st)), _plan(_desc(B, H_, cin, n, st, act=0))
        assert p3[0] == 0 and p3 == p0, (B, H_, cin, n, p3, p0)
        if B == 1 and H_ == 14:
            assert p3[2] > 1


def test_relu_refusals():
    lib = _lib.load()
    d = _desc(1, 14, 512, 512)
    d.residual = 4096
    assert _plan(d)[0] != 0
    d = _desc(1, 14, 512, 512)
    d.gn_partials, d.gn_groups = 4096, 32
    assert _plan(d)[0] != 0
    assert _plan(_desc(1, 14, 512, 512, tile=33))[0] != 0                  # register-staged tile: no ReLU twin
    assert "act 3" in lib.idb_last_error().decode()
    for sk in (1, 2, 4, 8):
        assert _plan(_desc(1, 14, 512, 512, split_k=sk))[2] == sk
    assert _plan(_desc(1, 14, 512, 512, act=4))[0] != 0
