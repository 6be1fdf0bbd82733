#!/usr/bin/env python3
"""Where an evaluation's time goes: the GPU feature metrics (prdc, authpct, kd of faceposegenerator_amd/metrics.py) at N rows per set
for each DINOv2 width, next to a host restatement of the same all-pairs work on the same box (float32 and float64: the distance
matrices by torch.cdist / matmul, the way dgm-eval forms them) and next to the encoder's time for the 2 N images behind the features
(DinoV2.features_u8, synthetic weights, f16, measured on --encoder-images images and scaled).  One JSON line per width.

    python tools/bench_metrics.py [--n 10000] [--dims 384,768,1024] [--host-n 10000] [--no-host] [--no-encoder]

--host-n runs the host restatement on fewer rows (its cost is quadratic: the line reports the rows it used).
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from faceposegenerator_amd import dinov2 as D
from faceposegenerator_amd import metrics as M

DEV = "cuda:0"
ARCH = {384: "vits14", 768: "vitb14", 1024: "vitl14"}


def features(n, d, seed):
    """Clustered features with a non-zero mean (the generator of tests/metrics_oracle.py, restated)."""
    rng = np.random.default_rng(seed)
    centres, lift = rng.normal(size=(8, 6)) * 1.5, rng.normal(size=(6, d)) / np.sqrt(6.0)

    def draw(shift):
        z = centres[rng.integers(0, 8, size=n)] + 0.7 * rng.normal(size=(n, 6)) + shift
        return (z @ lift + 0.05 * rng.normal(size=(n, d)) + 2.0).astype(np.float32)

    return draw(0.0), draw(0.25)


def gpu_ms(fn):
    fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def host_ms(real, gen, dtype, k=5):
    """prdc, authpct and 10 kd subsets of 1000 on the host in `dtype`; kd is scaled to 100 subsets."""
    r, g = torch.from_numpy(real).to(dtype), torch.from_numpy(gen).to(dtype)
    out = {}
    t = time.perf_counter()
    rr, gg, rg = torch.cdist(r, r), torch.cdist(g, g), torch.cdist(r, g)
    rad_r, rad_g = rr.kthvalue(k + 1, dim=1).values, gg.kthvalue(k + 1, dim=1).values
    inside = rg < rad_r[:, None]
    res = (inside.any(0).float().mean(), (rg < rad_g[None, :]).any(1).float().mean(), inside.sum(0).float().mean() / k,
           (rg.min(1).values < rad_r).float().mean())
    out["prdc"] = (time.perf_counter() - t) * 1e3
    t = time.perf_counter()
    rr.fill_diagonal_(float("inf"))
    near = rg.min(0)
    float((rr.min(0).values[near.indices] < near.values).float().mean())
    out["authpct"] = (time.perf_counter() - t) * 1e3 + _cdist_ms(r, g)      # the reference forms its two matrices again
    del rr, gg, rg, res
    m = min(1000, len(real), len(gen))
    rng = np.random.default_rng(0)
    t = time.perf_counter()
    for _ in range(10):
        x, y = r[rng.choice(len(real), m, replace=False)], g[rng.choice(len(gen), m, replace=False)]
        gamma = 1.0 / r.shape[1]
        kxx, kyy, kxy = (gamma * x @ x.T + 1) ** 3, (gamma * y @ y.T + 1) ** 3, (gamma * x @ y.T + 1) ** 3
        float((kxx.sum() - kxx.diagonal().sum() + kyy.sum() - kyy.diagonal().sum()) / (m * (m - 1)) - 2 * kxy.sum() / (m * m))
    out["kd"] = (time.perf_counter() - t) * 1e3 * 10
    return {k_: round(v, 1) for k_, v in out.items()}


def _cdist_ms(r, g):
    t = time.perf_counter()
    torch.cdist(r, r)
    torch.cdist(r, g)
    return (time.perf_counter() - t) * 1e3


def encoder_ms_per_image(arch, images):
    m = D.DinoV2.from_synthetic(0, arch, torch_dtype=torch.float16).to(DEV)
    m.chunk = 64
    imgs = (torch.rand(images, 512, 512, 3, generator=torch.Generator().manual_seed(1)) * 255).to(torch.uint8).to(DEV)
    return gpu_ms(lambda: m.features_u8(imgs)) / images


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--dims", default="384,768,1024")
    ap.add_argument("--host-n", type=int, default=None)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--no-encoder", action="store_true")
    ap.add_argument("--encoder-images", type=int, default=256)
    args = ap.parse_args()
    for d in [int(v) for v in args.dims.split(",")]:
        real, gen = features(args.n, d, d)
        r, g = torch.from_numpy(real).to(DEV), torch.from_numpy(gen).to(DEV)
        rng = np.random.default_rng(0)
        line = {"n": args.n, "d": d, "gpu_ms": {
            "prdc": round(gpu_ms(lambda: M.prdc(r, g)), 1), "authpct": round(gpu_ms(lambda: M.authpct(r, g)), 1),
            "kd_100x1000": round(gpu_ms(lambda: M.kd(r, g, rng=rng)), 1)}}
        # useful flops of the three distance passes of prdc (2 N^2 D each) over its time
        line["prdc_tflops"] = round(3 * 2.0 * args.n * args.n * d / line["gpu_ms"]["prdc"] / 1e9, 1)
        if not args.no_host:
            hn = min(args.host_n or args.n, args.n)
            line["host_n"] = hn
            line["host_f32_ms"] = host_ms(real[:hn], gen[:hn], torch.float32)
            line["host_f64_ms"] = host_ms(real[:hn], gen[:hn], torch.float64)
        if not args.no_encoder and d in ARCH:
            per = encoder_ms_per_image(ARCH[d], args.encoder_images)
            line["encoder"] = {"arch": ARCH[d], "ms_per_image": round(per, 3), "ms_for_2n_images": round(per * 2 * args.n, 0)}
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
