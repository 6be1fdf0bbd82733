#!/usr/bin/env python3
"""Where the identity-verification report's time goes (faceposegenerator_amd/verification.py) at the reference's scale: GPU time of
the cosine scores, the sort, the ROC reductions and the whole report from embeddings, next to a host restatement on 16 threads (numpy
float64 scores, np.sort, the full threshold curves of tests/verification_oracle.py).  Also prints the worst score error against the
float64 host scores and its bound (2 d + 8) 2^-53.  One JSON line.

    python tools/bench_verification.py [--ids 200] [--per-id 100] [--dim 512] [--no-host]
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

import verification_oracle as O
from faceposegenerator_amd import verification as V


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ids", type=int, default=200)
    ap.add_argument("--per-id", type=int, default=100)
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    torch.set_num_threads(16)
    rng = np.random.default_rng(0)
    centres = rng.standard_normal((args.ids, args.dim))
    x = np.repeat(centres, args.per_id, axis=0) + 0.8 * rng.standard_normal((args.ids * args.per_id, args.dim))
    embs = (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    names = [f"{k:04d}_{j}.png" for k in range(args.ids) for j in range(args.per_id)]

    t0 = time.perf_counter()
    grouped, counts, _ = V.group_by_identity(embs, names)
    ga, gb, ia, ib = V.pairs_among_synth(counts)
    pairs_ms = (time.perf_counter() - t0) * 1e3
    dev = torch.device("cuda:0")
    e = torch.from_numpy(grouped).to(dev)
    dga, dgb, dia, dib = (torch.from_numpy(v).to(dev) for v in (ga, gb, ia, ib))
    gen, imp = V.cos_scores(e, e, dga, dgb), V.cos_scores(e, e, dia, dib)
    res = {"ids": args.ids, "per_id": args.per_id, "dim": args.dim, "genuine_pairs": len(ga), "impostor_pairs": len(ia),
           "host_pairs_ms": round(pairs_ms, 2)}
    res["gpu_scores_ms"] = round(gpu_ms(lambda: (V.cos_scores(e, e, dga, dgb), V.cos_scores(e, e, dia, dib))), 3)
    res["gpu_sort_ms"] = round(gpu_ms(lambda: (torch.sort(gen), torch.sort(imp))), 3)
    gs, is_ = torch.sort(gen).values, torch.sort(imp).values
    res["gpu_roc_ms"] = round(gpu_ms(lambda: V.roc_points(gs, is_)), 3)
    res["gpu_report_ms"] = round(gpu_ms(lambda: V.verification_report(e, names), reps=2), 2)
    if not args.no_host:
        t0 = time.perf_counter()
        chunked = lambda a, b: np.concatenate([O.cos_scores(grouped, grouped, a[k:k + 65536], b[k:k + 65536])   # noqa: E731
                                               for k in range(0, len(a), 65536)])
        hg, hi = chunked(ga, gb), chunked(ia, ib)
        res["host_scores_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        t0 = time.perf_counter()
        np.sort(hg), np.sort(hi)
        res["host_sort_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        t0 = time.perf_counter()
        want = O.report(hg, hi)
        res["host_stats_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        err = max(np.abs(gen.cpu().numpy() - hg).max(), np.abs(imp.cpu().numpy() - hi).max())
        res["score_max_abs_err"], res["score_bound"] = float(err), (2 * args.dim + 8) * 2.0 ** -53
        got = V.verification_report(e, names)["report"]
        res["report_max_abs_diff_vs_host"] = float(max(abs(got[k] - want[k]) for k in want))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
