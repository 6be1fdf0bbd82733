#!/usr/bin/env python3
"""Where the pair benchmark's time goes (faceposegenerator_amd/frbench.py) at LFW's size: 6000 pairs = 12 000 synthetic crops, both
mirrors, r18 and r50 backbones with synthetic weights.  GPU time of the embedding, pair_distances, fold_counts at 400 and at 4000
thresholds and the whole test(), next to the vectorised numpy restatement of the same steps on the host (float64, one broadcast
comparison per fold instead of upstream's loop over thresholds).  Also prints the worst distance error against the float64 host
distances and its bound (16 d + 48) 2^-53.  One JSON line.

    python tools/bench_frbench.py [--pairs 6000] [--archs r18,r50] [--no-host]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import frbench_oracle as O
from faceposegenerator_amd import arcface as A
from faceposegenerator_amd import frbench as F


def gpu_ms(fn, reps=5):
    fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, (time.perf_counter() - t0) * 1e3)
    return best


def host_counts(dist, issame, thr, nfolds):
    """counts [nfolds, T, 2] by one broadcast np.less per fold."""
    b = O.kfold_bounds(len(dist), nfolds)
    out = np.zeros((nfolds, len(thr), 2), dtype=np.int64)
    for f in range(nfolds):
        below = np.less(dist[b[f]:b[f + 1], None], thr[None, :])
        s = issame[b[f]:b[f + 1], None]
        out[f, :, 0], out[f, :, 1] = (below & s).sum(0), (below & ~s).sum(0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=6000)
    ap.add_argument("--archs", default="r18,r50")
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    torch.set_num_threads(16)
    P = args.pairs
    g = torch.Generator().manual_seed(0)
    crops = torch.randint(0, 256, (2 * P, 112, 112, 3), generator=g, dtype=torch.uint8)
    issame = np.random.default_rng(0).random(P) < 0.5
    dev = torch.device("cuda:0")
    d_crops = crops.to(dev)
    res = {"pairs": P}
    e0, e1, same = O.pair_embeddings(P, 512, seed=1)
    t0, t1 = torch.from_numpy(e0).to(dev), torch.from_numpy(e1).to(dev)
    thr400, thr4000 = O.thresholds(0.01), O.thresholds(0.001)
    dist, _ = F.pair_distances(t0, t1)
    res["gpu_pair_distances_ms"] = round(gpu_ms(lambda: F.pair_distances(t0, t1)), 3)
    res["gpu_fold_counts_400_ms"] = round(gpu_ms(lambda: F.fold_counts(dist, same, thr400)), 3)
    res["gpu_fold_counts_4000_ms"] = round(gpu_ms(lambda: F.fold_counts(dist, same, thr4000)), 3)
    res["gpu_evaluate_ms"] = round(gpu_ms(lambda: F.evaluate(t0, t1, same)), 3)
    for arch in args.archs.split(","):
        m = A.ArcFace.from_synthetic(arch, 0).to(dev)
        res[f"gpu_embed_both_mirrors_{arch}_ms"] = round(gpu_ms(lambda: F.embed_with_flip(d_crops, m), reps=2), 1)
        res[f"gpu_test_{arch}_ms"] = round(gpu_ms(lambda: F.test(d_crops, issame, m), reps=2), 1)
        del m
    if not args.no_host:
        t = time.perf_counter()
        hd, _ = O.pair_dist(e0, e1)
        res["host_pair_distances_ms"] = round((time.perf_counter() - t) * 1e3, 2)
        for name, thr in (("400", thr400), ("4000", thr4000)):
            t = time.perf_counter()
            hc = host_counts(hd, same, thr, 10)
            res[f"host_fold_counts_{name}_ms"] = round((time.perf_counter() - t) * 1e3, 2)
            got = F.fold_counts(dist, same, thr)[0]
            res[f"counts_{name}_equal_host"] = bool(np.array_equal(got, hc))
        res["dist_max_abs_err"], res["dist_bound"] = float(np.abs(dist.cpu().numpy() - hd).max()), (16 * 512 + 48) * 2.0 ** -53
    print(json.dumps(res))


if __name__ == "__main__":
    main()
