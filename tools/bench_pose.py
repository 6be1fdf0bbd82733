#!/usr/bin/env python3
"""6DRepNet head-pose throughput (synthetic weights, f16): images/s of predict_u8 on 512x512 uint8 images (30-pixel border, resize,
network, head) at batch 1 / 64 / 256, against the same folded deploy-form network run by torch's own fp16 GPU convolutions
(F.conv2d, channels_last, groups = 2 where the network has them: MIOpen) on the same resized input.  The torch side includes no resize
(it starts from the normalised [B,3,224,224] tensor), so it is the network alone.  One JSON line per batch size.

    python tools/bench_pose.py [--batches 1,64,256] [--iters 10]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from faceposegenerator_amd import headpose as H

DEV = "cuda:0"


def torch_forward(sd, x):
    """Folded deploy-form network on torch's fp16 convolutions; pooling + linear_reg in fp32, 6D head in fp32 torch ops."""
    for key, _, _, stride, g in H.blocks():
        x = F.relu(F.conv2d(x, sd[f"{key}.rbr_reparam.weight"], sd[f"{key}.rbr_reparam.bias"], stride, 1, groups=g))
    o = F.linear(x.float().mean(dim=(2, 3)), sd["linear_reg.weight"].float(), sd["linear_reg.bias"].float())
    a = F.normalize(o[:, 0:3], dim=1, eps=1e-8)
    z = F.normalize(torch.linalg.cross(a, o[:, 3:6], dim=1), dim=1, eps=1e-8)
    y = torch.linalg.cross(z, a, dim=1)
    return torch.stack([a, y, z], dim=2)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,64,256")
    ap.add_argument("--iters", type=int, default=10)
    args = ap.parse_args()
    sd = H.synth_weights(0)
    m = H.HeadPose.from_state_dict(sd, torch.float16).to(DEV)
    m.chunk = 1 << 30
    d = H.deploy_state_dict(sd)
    sd16 = {k: v.to(DEV, torch.float16) for k, v in d.items()}
    sd16 = {k: (v.contiguous(memory_format=torch.channels_last) if v.ndim == 4 else v) for k, v in sd16.items()}
    for B in [int(b) for b in args.batches.split(",")]:
        imgs = (torch.rand(B, 512, 512, 3, generator=torch.Generator().manual_seed(B)) * 255).to(torch.uint8).to(DEV)
        ours = timed(lambda: m.predict_u8(imgs), args.iters)
        u8 = m.resize(imgs, H.PAD).permute(0, 3, 1, 2).float() / 255
        x = ((u8 - torch.tensor(H.MEAN, device=DEV).view(1, 3, 1, 1)) / torch.tensor(H.STD, device=DEV).view(1, 3, 1, 1))
        xt = x.half().contiguous(memory_format=torch.channels_last)
        net = timed(lambda: m(x), args.iters)
        with torch.no_grad():
            ref = timed(lambda: torch_forward(sd16, xt), args.iters)
            dr = (m(x) - torch_forward(sd16, xt)).abs().max().item()
        print(json.dumps({"batch": B, "dtype": "f16", "hip_predict_u8_ms": round(ours, 3), "hip_images_per_s": round(B * 1e3 / ours, 1),
                          "hip_net_ms": round(net, 3), "hip_net_tflops": round(B * H.gflops() / net, 1),
                          "torch_net_ms": round(ref, 3), "torch_images_per_s": round(B * 1e3 / ref, 1),
                          "speedup_net": round(ref / net, 3), "max_abs_R_vs_torch": round(dr, 6)}), flush=True)


if __name__ == "__main__":
    main()
