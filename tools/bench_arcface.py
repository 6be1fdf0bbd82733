#!/usr/bin/env python3
"""ArcFace r100 embedding throughput (synthetic weights, f16): faces/s and per-stage device time of the HIP path at batch 1 / 64 / 256,
against the same restated network run by torch's own fp16 GPU convolutions (channels_last, unfolded eval-mode BatchNorm, PReLU, the
head's fc in fp32 — the way the reference executes it under autocast).  One JSON line per batch size.

    python tools/bench_arcface.py [--arch r100] [--batches 1,64,256] [--iters 10]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from faceposegenerator_amd import arcface as A

DEV = "cuda:0"


def torch_forward(sd, arch, x):
    """The restated network on torch's fp16 GPU kernels (channels_last), BatchNorm unfolded, fc in fp32 outside autocast."""
    def bn(t, k):
        return F.batch_norm(t, sd[f"{k}.running_mean"], sd[f"{k}.running_var"], sd[f"{k}.weight"], sd[f"{k}.bias"], False, 0.0, 1e-5)
    x = F.prelu(bn(F.conv2d(x, sd["conv1.weight"], None, 1, 1), "bn1"), sd["prelu.weight"])
    for i, nb in enumerate(A.ARCHS[arch]):
        for j in range(nb):
            k, s = f"layer{i + 1}.{j}", 2 if j == 0 else 1
            o = F.conv2d(bn(x, f"{k}.bn1"), sd[f"{k}.conv1.weight"], None, 1, 1)
            o = F.prelu(bn(o, f"{k}.bn2"), sd[f"{k}.prelu.weight"])
            o = bn(F.conv2d(o, sd[f"{k}.conv2.weight"], None, s, 1), f"{k}.bn3")
            idt = x if j else bn(F.conv2d(x, sd[f"{k}.downsample.0.weight"], None, s, 0), f"{k}.downsample.1")
            x = o + idt
    x = bn(x, "bn2").contiguous().flatten(1)
    y = F.linear(x.float(), sd["fc.weight"].float(), sd["fc.bias"].float())
    return F.batch_norm(y, sd["features.running_mean"].float(), sd["features.running_var"].float(), sd["features.weight"].float(),
                        sd["features.bias"].float(), False, 0.0, 1e-5)


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def stage_times(m, x, iters):
    """Device ms of stem, layer1..4 and head (events around each part of one forward, averaged)."""
    acc = [0.0] * 6
    for _ in range(iters):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(7)]
        ev[0].record()
        h, hb = m.stem(x, False)
        ev[1].record()
        for i in range(4):
            h, hb = m.stage(i, h, hb)
            ev[i + 2].record()
        m.head(h)
        ev[6].record()
        torch.cuda.synchronize()
        for i in range(6):
            acc[i] += ev[i].elapsed_time(ev[i + 1]) / iters
    return dict(zip(["stem", "layer1", "layer2", "layer3", "layer4", "head"], [round(a, 3) for a in acc]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arch", default="r100")
    ap.add_argument("--batches", default="1,64,256")
    ap.add_argument("--iters", type=int, default=10)
    args = ap.parse_args()
    sd = A.synth_weights(args.arch, 0)
    m = A.ArcFace.from_state_dict(sd, args.arch, torch.float16).to(DEV)
    m.chunk = 1 << 30
    sd16 = {k: (v.to(DEV, torch.float16) if v.is_floating_point() else v.to(DEV)) for k, v in sd.items()}
    sd16 = {k: (v.contiguous(memory_format=torch.channels_last) if v.ndim == 4 else v) for k, v in sd16.items()}
    for B in [int(b) for b in args.batches.split(",")]:
        x = (torch.rand(B, 3, 112, 112, generator=torch.Generator().manual_seed(B)) * 2 - 1).to(DEV)
        ours = timed(lambda: m(x), args.iters)
        xt = x.half().contiguous(memory_format=torch.channels_last)
        with torch.no_grad():
            ref = timed(lambda: torch_forward(sd16, args.arch, xt), args.iters)
            cos = F.cosine_similarity(m(x), torch_forward(sd16, args.arch, xt), dim=1).min().item()
        print(json.dumps({"arch": args.arch, "batch": B, "dtype": "f16", "hip_ms": round(ours, 3), "hip_faces_per_s": round(B * 1e3 / ours, 1),
                          "torch_ms": round(ref, 3), "torch_faces_per_s": round(B * 1e3 / ref, 1), "speedup": round(ref / ours, 3),
                          "min_cosine_vs_torch": round(cos, 6), "hip_stage_ms": stage_times(m, x, args.iters)}), flush=True)


if __name__ == "__main__":
    main()
