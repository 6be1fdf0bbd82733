"""The trunk's training blocks without a GPU: the float64 oracle (tests/frblock_oracle.py) against a recording of the reference's own
IBasicBlock and stem (tests/golden/frblock_reference.*, written by tests/golden/make_frblock_reference.py), its backward against a
central finite difference of its forward, the conv-weight layout round trips, the C ABI's declarations and refusals, and the order of
BackboneSGD's parameters."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import frblock_oracle as BO  # noqa: E402

from faceposegenerator_amd import _lib as L  # noqa: E402
from faceposegenerator_amd import arcface as A  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NEW_ENTRIES = ("idb_blk_conv_workspace_bytes", "idb_blk_conv_forward", "idb_blk_conv_dgrad", "idb_blk_conv_wgrad", "idb_blk_bn_workspace_bytes",
               "idb_blk_bn_forward", "idb_blk_bn_backward", "idb_blk_affine", "idb_blk_pack_images", "idb_sgd_clip_table_workspace_bytes",
               "idb_sgd_clip_step_table")


def _rel(got, want):
    return float(np.abs(np.asarray(got) - np.asarray(want)).max() / max(float(np.abs(np.asarray(want)).max()), 1e-300))


def _summary_close(rec, name, a, stride, tol=1e-12):
    a = np.ascontiguousarray(a).reshape(a.shape[0], -1)
    assert _rel(a.sum(1), rec[f"{name}.rowsum"]) <= 1e-11, name
    assert _rel(a.sum(0), rec[f"{name}.colsum"]) <= 1e-11, name
    assert _rel(a.reshape(-1)[::stride], rec[f"{name}.sample"]) <= tol, name


def _nchw(a):
    return np.ascontiguousarray(a.transpose(0, 3, 1, 2))


def test_oracle_equals_reference_recording():
    """Every recorded quantity of the reference's IBasicBlock (three cases) and stem in float64 train mode, at the tolerance
    test_frtail_cpu.py uses for its float64-against-float64 comparison."""
    meta = json.load(open(os.path.join(GOLD, "frblock_reference.json")))
    rec = np.load(os.path.join(GOLD, "frblock_reference.npz"))
    st, tol = meta["stride"], 1e-12
    assert [tuple(c) for c in meta["cases"]] == [BO.BLOCK_CASES[0], BO.BLOCK_CASES[1], BO.BLOCK_CASES[2]]
    seen = set()
    for case in meta["cases"]:
        tag = "x".join(str(v) for v in case)
        x, prm, g = BO.case_inputs(*case)
        fw = BO.block_forward(x, prm, case[5])
        bw = BO.block_backward(x, prm, case[5], g, fw)
        _summary_close(rec, f"{tag}.out", _nchw(fw["out"]), st)
        _summary_close(rec, f"{tag}.grad.input", _nchw(bw["input"]), st)
        bns = ["bn1", "bn2", "bn3"] + (["downsample.1"] if "downsample.0.weight" in prm else [])
        convs = ["conv1", "conv2"] + (["downsample.0"] if "downsample.0.weight" in prm else [])
        for k in convs:
            _summary_close(rec, f"{tag}.grad.{k}.weight", BO.w_to_upstream(bw[f"{k}.weight"]), st)
        assert _rel(bw["prelu.weight"], rec[f"{tag}.grad.prelu.weight"]) <= tol
        for k in bns:
            for f in ("weight", "bias"):
                scale = float(np.abs(rec[f"{tag}.grad.bn2.weight"]).max())      # d bn3.bias-like sums may be 0 up to rounding
                assert float(np.abs(bw[f"{k}.{f}"] - rec[f"{tag}.grad.{k}.{f}"]).max()) <= tol * max(scale, float(np.abs(bw[f"{k}.{f}"]).max())), (tag, k, f)
            for f in ("running_mean", "running_var"):
                assert _rel(fw["running"][f"{k}.{f}"], rec[f"{tag}.running.{k}.{f}"]) <= tol, (tag, k, f)
            assert meta["tracked"][tag][k] == 1
        seen.update(k.split(".", 1)[1] for k in rec.files if k.startswith(tag + "."))
    assert any(k.startswith("grad.downsample.0.weight") for k in seen)
    B, H, W = meta["stem"]
    img, prm, g = BO.stem_inputs(B, H, W)
    fw = BO.stem_forward(img, prm)
    bw = BO.stem_backward(img, prm, g, fw)
    _summary_close(rec, "stem.out", _nchw(fw["out"]), st)
    _summary_close(rec, "stem.grad.conv1.weight", BO.w_to_upstream(bw["conv1.weight"]), st)
    for k in ("prelu.weight", "bn1.weight", "bn1.bias"):
        assert _rel(bw[k], rec[f"stem.grad.{k}"]) <= tol, k
    for f in ("running_mean", "running_var"):
        assert _rel(fw["running"][f"bn1.{f}"], rec[f"stem.running.bn1.{f}"]) <= tol
    assert meta["tracked"]["stem"] == {"bn1": 1}


@pytest.mark.parametrize("cin,planes,stride", [(3, 3, 1), (3, 4, 2)])
def test_oracle_backward_equals_finite_difference(cin, planes, stride):
    """L = sum(out * g) on a tiny block (the oracle has no channel restriction): every gradient against (L(+h) - L(-h)) / 2h."""
    x, prm, g = BO.case_inputs(2, cin, planes, 5, 4, stride)
    bw = BO.block_backward(x, prm, stride, g, BO.block_forward(x, prm, stride))

    def loss(xx, pp):
        return float((BO.block_forward(xx, pp, stride)["out"] * g).sum())

    h = 1e-6
    keys = [k for k in BO.BLOCK_GRADS if k in prm]
    assert len(keys) == (12 if stride == 2 else 9)
    for k in keys + ["input"]:
        base = x if k == "input" else prm[k]
        got = bw[k]
        assert got.shape == base.shape
        flat = np.arange(base.size)[:: max(1, base.size // 7)]
        for i in flat:
            d = np.zeros(base.size)
            d[i] = h
            d = d.reshape(base.shape)
            if k == "input":
                fd = (loss(x + d, prm) - loss(x - d, prm)) / (2 * h)
            else:
                fd = (loss(x, {**prm, k: base + d}) - loss(x, {**prm, k: base - d})) / (2 * h)
            assert abs(fd - got.reshape(-1)[i]) <= 1e-6 * max(1.0, float(np.abs(got).max())), (k, i, fd, got.reshape(-1)[i])


def test_oracle_terms_are_visible():
    """Each omitted term moves some output by far more than any bound: the comparisons can see it."""
    case = BO.BLOCK_CASES[0]
    x, prm, g = BO.case_inputs(*case)
    fw = BO.block_forward(x, prm, case[5], bounds=True)
    bw = BO.block_backward(x, prm, case[5], g, fw, bounds=True)
    wrong = BO.block_forward(x, prm, case[5], omit="pad_zero")
    ring = np.abs(wrong["c1"] - fw["c1"])
    assert ring[:, 1:-1, 1:-1].max() == 0.0 and ring[:, 0].mean() > 100 * fw["bound"]["c1"].max()
    for omit in ("bn_mean_term", "bn_xhat_term", "prelu_bwd", "identity"):
        other = BO.block_backward(x, prm, case[5], g, fw, omit=omit)
        assert max(np.abs(other[k] - bw[k]).max() / b.max() for k, b in bw["bound"].items()) > 50, omit
    for k, b in bw["bound"].items():
        assert b.shape == bw[k].shape and (b >= 0).all() and b.max() > 0, k


def test_conv_weight_layout_round_trips():
    from faceposegenerator_amd import frtrunk as T
    w = torch.arange(2 * 3 * 3 * 3, dtype=torch.float32).reshape(2, 3, 3, 3)
    d = T.conv_to_device(w)
    assert d.shape == (2, 3, 3, 3) and d.is_contiguous() and d[1, 2, 0, 1] == w[1, 1, 2, 0]
    assert torch.equal(T.conv_to_upstream(d), w)
    wn = np.arange(4 * 5 * 3 * 3, dtype=np.float64).reshape(4, 5, 3, 3)
    assert np.array_equal(BO.w_to_upstream(BO.w_to_device(wn)), wn)
    assert np.array_equal(BO.w_to_device(wn), T.conv_to_device(torch.from_numpy(wn)).numpy())
    # the device order is fold_weights' / pack_conv's: [cout][ky][kx][cin]
    from faceposegenerator_amd import _hipnet as N
    assert np.array_equal(N.pack_conv(torch.from_numpy(wn)).numpy().reshape(4, 3, 3, 5), BO.w_to_device(wn))


def test_abi_declares_the_new_entries(lib):
    header = open(os.path.join(os.path.dirname(GOLD), "..", "include", "idb_kernels.h")).read()
    for name in NEW_ENTRIES:
        assert name in L.EXPORTS and f"{name}(" in header and hasattr(lib, name), name
    assert "idb_blk_conv_desc" in header and L.BlkConvDesc._fields_[0][0] == "b"


def test_refusals_before_any_launch(lib):
    """Out-of-bounds shapes come back as IDB_EINVAL from the host checks (no device is needed to see them)."""
    assert lib.idb_blk_conv_workspace_bytes(2, 8, 8, 64, 64, 3, 1, None, None) > 0
    for bad in ((2, 8, 8, 32, 64, 3, 1), (2, 8, 8, 64, 96, 3, 1), (2, 129, 8, 64, 64, 3, 1), (2, 8, 0, 64, 64, 3, 1), (1025, 8, 8, 64, 64, 3, 1),
                (2, 8, 8, 64, 64, 5, 1), (2, 8, 8, 64, 64, 3, 3), (2, 8, 8, 2112, 64, 3, 1), (2, 8, 8, 64, 2112, 3, 1)):
        assert lib.idb_blk_conv_workspace_bytes(*bad, None, None) == 0, bad
        d = L.BlkConvDesc()
        d.b, d.h, d.w, d.cin, d.cout, d.ksize, d.stride = bad
        d.x = d.weight = 4096
        assert lib.idb_blk_conv_forward(C.byref(d), 4096, None) != 0, bad
        assert lib.idb_blk_conv_wgrad(C.byref(d), 4096, 4096, 4096, 1 << 40, None) != 0, bad
    d = L.BlkConvDesc()
    d.b, d.h, d.w, d.cin, d.cout, d.ksize, d.stride = 2, 8, 8, 4, 64, 3, 1
    d.x = d.weight = 4096
    assert lib.idb_blk_conv_dgrad(C.byref(d), 4096, 4096, None) != 0 and b"cin" in lib.idb_last_error()
    assert lib.idb_blk_bn_workspace_bytes(128, 64, None) > 0 and lib.idb_blk_bn_workspace_bytes(128, 96, None) == 0
    assert lib.idb_blk_bn_forward(4096, 1, 64, 1, 1e-5, 0.1, 4096, 4096, 4096, 4096, 4096, 4096, 4096, 4096, 1 << 40, None) != 0
    assert b"training" in lib.idb_last_error()
    assert lib.idb_sgd_clip_table_workspace_bytes(0) == 0 and lib.idb_sgd_clip_table_workspace_bytes(1025) == 0
    assert lib.idb_sgd_clip_table_workspace_bytes(1024) == 8 * 1024 * 1024
    assert lib.idb_sgd_clip_step_table(1025, 4096, 4096, 4096, 4096, 0.1, 0.9, 5e-4, 5.0, 1, 4096, 4096, 1 << 40, None) != 0


def test_plans_split_wgrad_and_dgrad(lib):
    """The plan query alone: some case runs wgrad in >= 2 slices and some dgrad in >= 2 row tiles."""
    from faceposegenerator_amd import frtrunk as T
    _, slices, _ = T.conv_plan(5, 12, 12, 64, 64, 3, 1)
    _, _, tiles = T.conv_plan(3, 7, 7, 64, 128, 3, 1)
    assert slices >= 2 and tiles == 2


def test_backbone_sgd_parameter_order():
    from faceposegenerator_amd import frtail, frtrunk as T
    for arch in ("r18", "r34", "r50", "r100"):
        shapes = A.param_shapes(arch)
        trunk_keys = [k for k in shapes if not k.startswith(("bn2.", "fc.", "features."))]
        assert list(T.trunk_param_shapes(A.ARCHS[arch]).items()) == [(k, shapes[k]) for k in trunk_keys]
    sd = A.synth_weights("r18", seed=3)
    trunk = T.Trunk(sd, arch="r18")
    stage = frtail.EmbeddingStage.from_state_dict(sd)
    opt = T.BackboneSGD(trunk, stage, lr=0.1)
    shapes = A.param_shapes("r18")
    want = [k for k in shapes if not k.endswith(("running_mean", "running_var", "num_batches_tracked")) and k != "features.weight"]
    assert opt.keys == want and len(want) == 93
    # the state dict is upstream's, and merges into a strict backbone state dict
    merged = trunk.merged_state_dict(stage)
    A.check_state_dict(merged, "r18")
    assert list(merged) == list(shapes)
    for k in ("conv1.weight", "layer2.0.downsample.0.weight", "layer4.1.conv2.weight", "fc.weight", "layer3.0.bn1.running_var"):
        assert torch.equal(merged[k], sd[k].float()), k


def test_python_refusals():
    from faceposegenerator_amd import frtrunk as T
    sd = A.synth_weights("r18", seed=1)
    with pytest.raises(NotImplementedError, match="SE"):
        T.Trunk({**sd, "layer1.0.se_block.fc1.weight": torch.zeros(4, 64)}, arch="r18")
    with pytest.raises(NotImplementedError, match="IBottleneck"):
        T.Trunk({**sd, "layer1.0.conv3.weight": torch.zeros(64, 64, 1, 1)}, arch="r18")
    with pytest.raises(NotImplementedError, match="dilation"):
        T.Trunk(sd, arch="r18", dilation=2)
    with pytest.raises(NotImplementedError, match="sharding"):
        T.Trunk(sd, arch="r18", world_size=2)
    with pytest.raises(ValueError, match="lacks"):
        T.Trunk({k: v for k, v in sd.items() if k != "layer3.1.bn2.bias"}, arch="r18")
    with pytest.raises(ValueError, match="downsample"):
        T.TrainBlock({k: v for k, v in sd.items() if "downsample" not in k}, "layer2.0", 64, 128, 2)
    with pytest.raises(ValueError, match="HIP device"):
        T.Trunk(sd, arch="r18").to("cpu")
    blk = T.TrainBlock(sd, "layer1.1", 64, 64, 1)
    assert len(blk.trainable()) == 9 and len(T.TrainBlock(sd, "layer2.0", 64, 128, 2).trainable()) == 12
    with pytest.raises(L.IdbError, match="not on a device"):
        blk(torch.zeros(2, 8, 8, 64))
