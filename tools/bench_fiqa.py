#!/usr/bin/env python3
"""CR-FIQA scoring throughput (synthetic weights, f16): images/s of ``FaceQuality.get_batch_feature`` on device-resident uint8 images,
and the split of one batch into resize / network / tail (device events around each part).  One JSON line.

    timeout -k 10 300 python tools/bench_fiqa.py [--arch r50] [--batch 256] [--size 512] [--iters 10] [--limit 240]

The process also ends itself after ``--limit`` seconds (SIGALRM with the default action), so a hung device cannot hold it."""
import argparse
import json
import os
import signal
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from faceposegenerator_amd import fiqa as F

DEV = "cuda:0"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arch", default="r50")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--limit", type=int, default=240)
    args = ap.parse_args()
    signal.alarm(args.limit)
    if not torch.cuda.is_available():
        raise SystemExit("bench_fiqa needs a GPU: there is no CPU path to time")
    m = F.FaceQuality.from_synthetic(args.arch, 0, torch.float16).to(DEV)
    m.chunk = args.batch
    B, S = args.batch, args.size
    imgs = torch.randint(0, 256, (B, S, S, 3), generator=torch.Generator().manual_seed(0), dtype=torch.uint8).to(DEV)

    def events(n):
        return [torch.cuda.Event(enable_timing=True) for _ in range(n)]

    for _ in range(2):                                            # warm-up: code objects, the coefficient tables, the workspace
        m.get_batch_feature(imgs)
    torch.cuda.synchronize()
    e = events(2)
    e[0].record()
    for _ in range(args.iters):
        m.get_batch_feature(imgs)
    e[1].record()
    torch.cuda.synchronize()
    total = e[0].elapsed_time(e[1]) / args.iters
    acc = [0.0, 0.0, 0.0]
    for _ in range(args.iters):
        ev = events(4)
        ev[0].record()
        crops = m.resize(imgs)
        ev[1].record()
        emb = m._forward(crops, True)
        ev[2].record()
        m.tail(emb)
        ev[3].record()
        torch.cuda.synchronize()
        for i in range(3):
            acc[i] += ev[i].elapsed_time(ev[i + 1]) / args.iters
    src_bytes = B * S * S * 3
    print(json.dumps({"arch": args.arch, "dtype": "f16", "batch": B, "size": S, "iters": args.iters, "batch_ms": round(total, 3),
                      "images_per_s": round(B * 1e3 / total, 1), "resize_ms": round(acc[0], 4), "network_ms": round(acc[1], 3),
                      "tail_ms": round(acc[2], 4), "resize_source_GB_per_s": round(src_bytes / acc[0] / 1e6, 1)}), flush=True)


if __name__ == "__main__":
    main()
