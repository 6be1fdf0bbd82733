"""Recorder of tests/golden/frblock_reference.{npz,json}: the reference's own IBasicBlock and the stem lines of its IResNet.forward
driven through autograd in float64 train mode.

    python tests/golden/make_frblock_reference.py <path to the reference's FR_training directory>

Run once on a CPU; no test imports this file and nothing on a GPU machine needs it.  Inputs, parameters and cotangents come from
frblock_oracle.case_inputs / stem_inputs -- integer arithmetic, no RNG, so the test rebuilds them instead of storing them.  The
downsample branch is an nn.Sequential(conv1x1, BatchNorm2d), as the reference's _make_layer builds it.  The stem is the reference's
iresnet18 run on the images up to layer1 (a hook on layer1 takes its input and stops the forward).  Recorded per case: the
per-channel gradients and the running statistics in full, num_batches_tracked, and for the output, the conv-weight gradients and the
input gradient their row sums, column sums and a strided sample (upstream's layouts)."""
import importlib.util
import json
import os
import sys

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import frblock_oracle as BO  # noqa: E402

CASES = (BO.BLOCK_CASES[0], BO.BLOCK_CASES[1], BO.BLOCK_CASES[2])
STRIDE = 97


def summary(rec, name, a):
    a = np.ascontiguousarray(a).reshape(a.shape[0], -1)
    rec[f"{name}.rowsum"], rec[f"{name}.colsum"], rec[f"{name}.sample"] = a.sum(1), a.sum(0), a.reshape(-1)[::STRIDE].copy()


def set_bn(m, prm, key):
    with torch.no_grad():
        for f in ("weight", "bias", "running_mean", "running_var"):
            getattr(m, f).copy_(torch.from_numpy(prm[f"{key}.{f}"]))


def set_conv(m, prm, key):
    with torch.no_grad():
        m.weight.copy_(torch.from_numpy(BO.w_to_upstream(prm[f"{key}.weight"])))


def record_bn(rec, tag, m, key):
    rec[f"{tag}.grad.{key}.weight"], rec[f"{tag}.grad.{key}.bias"] = m.weight.grad.numpy(), m.bias.grad.numpy()
    rec[f"{tag}.running.{key}.running_mean"], rec[f"{tag}.running.{key}.running_var"] = m.running_mean.numpy(), m.running_var.numpy()
    return int(m.num_batches_tracked)


class _Stop(Exception):
    pass


def main(ref_dir: str) -> None:
    spec = importlib.util.spec_from_file_location("ref_iresnet", os.path.join(ref_dir, "backbones", "iresnet.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    rec, meta = {}, {"stride": STRIDE, "torch": torch.__version__, "cases": [list(c) for c in CASES], "stem": list(BO.STEM_CASE), "tracked": {}}
    for case in CASES:
        B, cin, planes, H, W, stride = case
        tag = "x".join(str(v) for v in case)
        x, prm, g = BO.case_inputs(*case)
        ds = None
        if "downsample.0.weight" in prm:
            ds = nn.Sequential(mod.conv1x1(cin, planes, stride), nn.BatchNorm2d(planes, eps=1e-05))
        blk = mod.IBasicBlock(cin, planes, stride, ds).double().train()
        for key in ("bn1", "bn2", "bn3"):
            set_bn(getattr(blk, key), prm, key)
        set_conv(blk.conv1, prm, "conv1")
        set_conv(blk.conv2, prm, "conv2")
        with torch.no_grad():
            blk.prelu.weight.copy_(torch.from_numpy(prm["prelu.weight"]))
        if ds is not None:
            set_conv(ds[0], prm, "downsample.0")
            set_bn(ds[1], prm, "downsample.1")
        xt = torch.from_numpy(np.ascontiguousarray(x.transpose(0, 3, 1, 2))).requires_grad_(True)
        out = blk(xt)
        out.backward(torch.from_numpy(np.ascontiguousarray(g.transpose(0, 3, 1, 2))))
        summary(rec, f"{tag}.out", out.detach().numpy())
        summary(rec, f"{tag}.grad.input", xt.grad.numpy())
        summary(rec, f"{tag}.grad.conv1.weight", blk.conv1.weight.grad.numpy())
        summary(rec, f"{tag}.grad.conv2.weight", blk.conv2.weight.grad.numpy())
        rec[f"{tag}.grad.prelu.weight"] = blk.prelu.weight.grad.numpy()
        tracked = {key: record_bn(rec, tag, getattr(blk, key), key) for key in ("bn1", "bn2", "bn3")}
        if ds is not None:
            summary(rec, f"{tag}.grad.downsample.0.weight", ds[0].weight.grad.numpy())
            tracked["downsample.1"] = record_bn(rec, tag, ds[1], "downsample.1")
        meta["tracked"][tag] = tracked
    # the stem lines of IResNet.forward
    B, H, W = BO.STEM_CASE
    img, prm, g = BO.stem_inputs(B, H, W)
    model = mod.iresnet18(num_features=64).double().train()
    set_conv(model.conv1, prm, "conv1")
    set_bn(model.bn1, prm, "bn1")
    with torch.no_grad():
        model.prelu.weight.copy_(torch.from_numpy(prm["prelu.weight"]))
    seen = {}

    def take(m, i):
        seen["stem"] = i[0]
        raise _Stop()

    model.layer1.register_forward_pre_hook(take)
    try:
        model(torch.from_numpy(img))
    except _Stop:
        pass
    seen["stem"].backward(torch.from_numpy(np.ascontiguousarray(g.transpose(0, 3, 1, 2))))
    summary(rec, "stem.out", seen["stem"].detach().numpy())
    summary(rec, "stem.grad.conv1.weight", model.conv1.weight.grad.numpy())
    rec["stem.grad.prelu.weight"] = model.prelu.weight.grad.numpy()
    meta["tracked"]["stem"] = {"bn1": record_bn(rec, "stem", model.bn1, "bn1")}
    np.savez_compressed(os.path.join(HERE, "frblock_reference.npz"), **rec)
    with open(os.path.join(HERE, "frblock_reference.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
    print(meta, sum(v.nbytes for v in rec.values()), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
