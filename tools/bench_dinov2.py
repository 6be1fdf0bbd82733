#!/usr/bin/env python3
"""DINOv2 feature throughput (synthetic weights, f16): images/s of features_u8 on 512x512 uint8 images (Pillow-exact bicubic resize,
patch embedding, the transformer blocks, class-token head) at batch 64 and batch 1, and the split of one forward over its stages and
the six launches of a block (each timed alone with device events, so the parts need not add up to the whole exactly).  One JSON line
per batch size.

    python tools/bench_dinov2.py [--arch vitl14] [--batches 64,1] [--iters 10] [--once]

--once runs a single features_u8 call per batch size and nothing else (for a rocprofv3 --kernel-trace --stats run).
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from faceposegenerator_amd import _lib as L
from faceposegenerator_amd import dinov2 as D

DEV = "cuda:0"


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


def split(m, imgs, iters):
    """ms per stage of one forward; the block launches are those of block 0 times the depth."""
    d, n, B = m.dim, D.NPATCH + 1, imgs.shape[0]
    out = {"resize": timed(lambda: m.resize(imgs), iters)}
    u8 = m.resize(imgs)
    out["patchify"] = timed(lambda: m.patchify(u8, True), iters)
    p = m.patchify(u8, True)
    out["patch_gemm"] = timed(lambda: m.linear(p, "patch"), iters)
    out["patch_tokens_all"] = timed(lambda: m.patch_tokens(u8, True), iters)
    x = m.patch_tokens(u8, True)
    h = m.layernorm(x, "0.ln1")
    qkv = m.linear(h, "0.qkv")
    o = torch.empty((B * n, d), dtype=m.tdt, device=m.device)
    ptr, es = qkv.data_ptr(), qkv.element_size()

    def attn():
        L.check(m.lib.idb_attention(ptr, 3 * d, ptr + d * es, ptr + 2 * d * es, 3 * d, o.data_ptr(), d, B, m.heads, n, n, n, 0.125, 0, m.dt,
                                    m._stream()), "idb_attention")
    attn()
    x2 = m.linear(o, "0.proj", residual=x)
    mm = m.linear(m.layernorm(x2, "0.ln2"), "0.fc1", act=1)
    per_block = {"layernorm_x2": 2 * timed(lambda: m.layernorm(x, "0.ln1"), iters), "qkv": timed(lambda: m.linear(h, "0.qkv"), iters),
                 "attention": timed(attn, iters), "proj": timed(lambda: m.linear(o, "0.proj", residual=x), iters),
                 "fc1_gelu": timed(lambda: m.linear(h, "0.fc1", act=1), iters), "fc2": timed(lambda: m.linear(mm, "0.fc2", residual=x2), iters)}
    for k, v in per_block.items():
        out["blocks." + k] = v * m.depth
    out["head"] = timed(lambda: m.head(x), iters)
    return {k: round(v, 3) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arch", default="vitl14")
    ap.add_argument("--batches", default="64,1")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    m = D.DinoV2.from_synthetic(0, args.arch, torch_dtype=torch.float16).to(DEV)
    for B in [int(b) for b in args.batches.split(",")]:
        m.chunk = B
        imgs = (torch.rand(B, 512, 512, 3, generator=torch.Generator().manual_seed(B)) * 255).to(torch.uint8).to(DEV)
        if args.once:
            m.features_u8(imgs)
            torch.cuda.synchronize()
            continue
        ms = timed(lambda: m.features_u8(imgs), args.iters)
        u8 = m.resize(imgs)
        net = timed(lambda: m.head(_blocks(m, m.patch_tokens(u8, True))), args.iters)
        print(json.dumps({"arch": args.arch, "batch": B, "dtype": "f16", "features_u8_ms": round(ms, 3), "images_per_s": round(B * 1e3 / ms, 1),
                          "net_ms": round(net, 3), "net_tflops": round(B * D.gflops(m.dim, m.depth) / net, 1),
                          "split_ms": split(m, imgs, args.iters)}), flush=True)


def _blocks(m, t):
    for i in range(m.depth):
        t = m.block(i, t)
    return t


if __name__ == "__main__":
    main()
