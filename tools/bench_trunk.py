#!/usr/bin/env python3
"""The backbone's trunk in training at the loop's shape (faceposegenerator_amd/frtrunk.py): iresnet18 at B = 128 on 112 x 112 images.
Columns:
  block_forward    TrainBlock(x) of --block (default layer2.1: 128 -> 128 at 28 x 28, stride 1)
  block_backward   TrainBlock.backward(out, g)
  trunk_forward    Trunk(images); trunk_backward: Trunk.backward(out, g)
  train_step_full  frtrunk.train_step_full with a CosFace header of --classes identities (everything, both optimiser steps)
  torch_*          a plain fp32 eager restatement on the same GPU, written here from stock modules (nn.BatchNorm2d, nn.Conv2d,
                   nn.PReLU; channels_last left to torch's default), autograd's backward(), clip_grad_norm_ + torch.optim.SGD
Each figure is the median wall clock over --reps calls after two warm-up calls; every call ends in a device-to-host read.  "cold": a
512 MB buffer is overwritten before each timed call; "hot": back-to-back calls.  Also the FLOPs of the block's products (forward
2 M N K per conv, backward twice that) against the times, as TFLOP/s, and the peak extra device memory of a step.  One JSON line.

    python tools/bench_trunk.py [--batch 128] [--reps 10] [--classes 10572] [--block layer2.1]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import torch.nn as nn
import torch.nn.functional as F

from faceposegenerator_amd import arcface as A
from faceposegenerator_amd import frhead as H
from faceposegenerator_amd import frtail
from faceposegenerator_amd import frtrunk as T

DEV = torch.device("cuda:0")


def timed(fn, reps, flush):
    fn()
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        if flush is not None:
            flush.add_(1)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(out), 4), round(min(out), 4)


def peak_extra(fn):
    fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(DEV)
    base = torch.cuda.memory_allocated(DEV)
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated(DEV) - base) / 2 ** 20


class TorchBlock(nn.Module):
    """IBasicBlock restated from stock modules."""

    def __init__(self, cin, planes, stride, ds):
        super().__init__()
        self.bn1, self.conv1 = nn.BatchNorm2d(cin), nn.Conv2d(cin, planes, 3, 1, 1, bias=False)
        self.bn2, self.prelu = nn.BatchNorm2d(planes), nn.PReLU(planes)
        self.conv2, self.bn3 = nn.Conv2d(planes, planes, 3, stride, 1, bias=False), nn.BatchNorm2d(planes)
        self.downsample = nn.Sequential(nn.Conv2d(cin, planes, 1, stride, bias=False), nn.BatchNorm2d(planes)) if ds else None

    def forward(self, x):
        out = self.bn3(self.conv2(self.prelu(self.bn2(self.conv1(self.bn1(x))))))
        return out + (x if self.downsample is None else self.downsample(x))


class TorchNet(nn.Module):
    def __init__(self, layers, n):
        super().__init__()
        self.conv1, self.bn1, self.prelu = nn.Conv2d(3, 64, 3, 1, 1, bias=False), nn.BatchNorm2d(64), nn.PReLU(64)
        cin = 64
        for i, (nb, planes) in enumerate(zip(layers, A.PLANES)):
            blocks = [TorchBlock(cin if j == 0 else planes, planes, 2 if j == 0 else 1, j == 0) for j in range(nb)]
            setattr(self, f"layer{i + 1}", nn.Sequential(*blocks))
            cin = planes
        self.bn2, self.dropout, self.fc, self.features = nn.BatchNorm2d(512), nn.Dropout(0.4), nn.Linear(512 * 49, n), nn.BatchNorm1d(n)
        self.features.weight.requires_grad = False

    def forward(self, x):
        x = self.prelu(self.bn1(self.conv1(x)))
        x = self.layer4(self.layer3(self.layer2(self.layer1(x))))
        return self.features(self.fc(self.dropout(torch.flatten(self.bn2(x), 1))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--classes", type=int, default=10572)
    ap.add_argument("--block", default="layer2.1")
    args = ap.parse_args()
    B, n = args.batch, 512
    flush = torch.zeros(512 << 18, dtype=torch.int32, device=DEV)
    g = torch.Generator().manual_seed(0)
    sd = A.synth_weights("r18", seed=1)
    trunk = T.Trunk(sd, arch="r18").to(DEV)
    stage = frtail.EmbeddingStage.from_state_dict(sd).to(DEV)
    header = H.MarginHeader.from_synthetic(n, args.classes, 1, "CosFace").to(DEV)
    opt_b, opt_h = T.BackboneSGD(trunk, stage, 1e-4), H.HeaderSGD(header, 1e-4)
    images = (torch.rand(B, 3, 112, 112, generator=g) * 2 - 1).to(DEV)
    labels = torch.randint(0, args.classes, (B,), generator=g)
    blk = next(b for b in trunk.blocks if b.prefix == args.block + ".")
    li = int(args.block[5]) - 1
    side = 112 >> (li + 1) if blk.stride == 1 else 112 >> li
    xb = torch.randn(B, side, side, blk.cin, generator=g).to(DEV)
    so = T.conv_out(side, 3, blk.stride)
    gb = (torch.randn(B, so, so, blk.planes, generator=g) / B).to(DEV)
    gmap = (torch.randn(B, 7, 7, 512, generator=g) / B).to(DEV)

    net = TorchNet(A.ARCHS["r18"], n).to(DEV).train()
    net.load_state_dict({k: v for k, v in sd.items()}, strict=True)
    tblk = getattr(net, args.block.split(".")[0])[int(args.block.split(".")[1])]
    t_params = [q for q in net.parameters() if q.requires_grad]
    t_opt = torch.optim.SGD(t_params, lr=1e-4, momentum=0.9, weight_decay=5e-4)
    t_kernel = header.kernel.clone().to(DEV).requires_grad_(True)
    xb_nchw = xb.permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    gb_nchw = gb.permute(0, 3, 1, 2).contiguous()
    state = {}

    def b_fwd():
        state["bo"] = blk(xb)
        return state["bo"].output[0, 0, 0, 0].item()

    def b_bwd():
        state["bg"] = blk.backward(state["bo"], gb)
        return state["bg"].input[0, 0, 0, 0].item()

    def t_fwd_():
        state["to"] = trunk(images)
        return state["to"].map[0, 0, 0, 0].item()

    def t_bwd_():
        state["tg"] = trunk.backward(state["to"], gmap)
        return state["tg"]["bn1.bias"][0].item()

    def step():
        return T.train_step_full(trunk, stage, header, opt_b, opt_h, images, labels)["loss"]

    def tb_fwd():
        state["tbo"] = tblk(xb_nchw)
        return state["tbo"][0, 0, 0, 0].item()

    def tb_bwd():
        for q in list(tblk.parameters()) + [xb_nchw]:
            q.grad = None
        state["tbo"].backward(gb_nchw, retain_graph=True)
        return xb_nchw.grad[0, 0, 0, 0].item()

    def t_step():
        for q in t_params + [t_kernel]:
            q.grad = None
        emb = F.normalize(net(images))
        cos = emb @ F.normalize(t_kernel, dim=0)
        logits = 64.0 * (cos - 0.35 * F.one_hot(labels.to(DEV), args.classes))
        loss = F.cross_entropy(logits, labels.to(DEV))
        loss.backward()
        torch.nn.utils.clip_grad_norm_(t_params, 5.0)
        t_opt.step()
        return loss.item()

    b_fwd(), b_bwd(), tb_fwd(), tb_bwd()
    res = {"batch": B, "block": args.block, "block_shape": [blk.cin, blk.planes, side, blk.stride], "reps": args.reps,
           "max_abs_diff_block_out": (state["bo"].output.permute(0, 3, 1, 2) - state["tbo"]).abs().max().item(),
           "max_abs_diff_block_d_input": (state["bg"].input.permute(0, 3, 1, 2) - xb_nchw.grad).abs().max().item(),
           "max_abs_block_d_input": xb_nchw.grad.abs().max().item()}
    for name, fn in (("block_forward", b_fwd), ("block_backward", b_bwd), ("trunk_forward", t_fwd_), ("trunk_backward", t_bwd_),
                     ("train_step_full", step), ("torch_block_forward", tb_fwd), ("torch_block_backward", tb_bwd), ("torch_train_step", t_step)):
        res[name + "_cold_ms"], res[name + "_cold_min_ms"] = timed(fn, args.reps, flush)
        res[name + "_hot_ms"], res[name + "_hot_min_ms"] = timed(fn, args.reps, None)
    res["peak_extra_mib"] = round(peak_extra(step), 1)
    res["torch_peak_extra_mib"] = round(peak_extra(t_step), 1)
    flops = 2.0 * B * side * side * blk.planes * 9 * blk.cin + 2.0 * B * so * so * blk.planes * 9 * blk.planes
    if blk.has_ds:
        flops += 2.0 * B * so * so * blk.planes * blk.cin
    res["block_forward_flops"] = flops
    res["block_forward_tflops_hot"] = round(flops / (res["block_forward_hot_ms"] * 1e-3) / 1e12, 2)
    res["block_backward_tflops_hot"] = round(2 * flops / (res["block_backward_hot_ms"] * 1e-3) / 1e12, 2)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
