#!/usr/bin/env python3
"""The FR-training input stage (``ra_4_16``: flip + RandAugment(4, 16) + ToTensor + Normalize) at 112 x 112, two measurements.

  * the idb_randaug launch: device events round ``augment.apply(..., "float")`` on a device-resident uint8 batch after warm-up, the
    median of ``--iters`` launches, at batch 128 and batch 1024 — the time includes the upload of the plan's slot arguments, which
    every real call pays — and, separately, the host time of ``RandAugment.plan`` (the draws) and of ``slot_args`` (plan -> kernel
    arguments), medians of host-clock timings;
  * the reference's path on the same machine: the same chain per image on Pillow (tests/randaug_oracle.py part (a), which restates
    the reference's transform on the library it calls), in 1 process and in ``--procs`` processes, images/s of a host clock.

One JSON line.  No figure is a pass condition.

    timeout -k 10 420 python tools/bench_augment.py [--iters 50] [--procs 16] [--pillow-images 1024] [--limit 400]

The process also ends itself after ``--limit`` seconds (SIGALRM with the default action), so a hung device cannot hold it."""
import argparse
import json
import multiprocessing as mp
import os
import signal
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

SIZE = 112


def _pillow_worker(job):
    """one worker of the reference's path: seeds the global generators as a DataLoader worker has its own, runs the chain per image"""
    seed, count = job
    import warnings

    import torch

    import randaug_oracle as R
    torch.set_num_threads(1)
    torch.manual_seed(seed)
    np.random.seed(seed)
    x = np.random.default_rng(seed).integers(0, 256, (count, SIZE, SIZE, 3), dtype=np.uint8)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        t0 = time.perf_counter()
        R.chain(x, 4, 16, 0.5)
        return time.perf_counter() - t0


def pillow_rate(total, procs):
    """images/s of ``total`` images split over ``procs`` fresh processes (wall clock of the slowest worker's chain, start-up excluded)"""
    jobs = [(100 + i, total // procs) for i in range(procs)]
    if procs == 1:
        worst = _pillow_worker(jobs[0])
    else:
        with mp.get_context("spawn").Pool(procs) as pool:
            worst = max(pool.map(_pillow_worker, jobs))
    return (total // procs) * procs / worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--procs", type=int, default=16)
    ap.add_argument("--pillow-images", type=int, default=1024)
    ap.add_argument("--limit", type=int, default=400)
    args = ap.parse_args()
    signal.alarm(args.limit)
    import torch

    from faceposegenerator_amd import augment as A
    if not torch.cuda.is_available():
        raise SystemExit("bench_augment needs a GPU: there is no CPU path to time")
    dev = "cuda:0"
    out = {"size": SIZE, "policy": "ra_4_16", "output": "float", "iters": args.iters}
    ra = A.RandAugment(4, 16)
    for batch in (128, 1024):
        x = torch.randint(0, 256, (batch, SIZE, SIZE, 3), generator=torch.Generator().manual_seed(batch), dtype=torch.uint8).to(dev)
        g, r = torch.Generator().manual_seed(1), np.random.RandomState(1)
        plan_s, slot_s, dev_ms = [], [], []
        for it in range(args.iters + 3):                          # 3 warm-up rounds: code object, allocator, the slot tables
            t0 = time.perf_counter()
            plan = ra.plan(batch, g, r)
            t1 = time.perf_counter()
            A.slot_args(plan, SIZE, SIZE)
            t2 = time.perf_counter()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            A.apply(x, plan, "float")
            e1.record()
            torch.cuda.synchronize()
            if it >= 3:
                plan_s.append(t1 - t0)
                slot_s.append(t2 - t1)
                dev_ms.append(e0.elapsed_time(e1))
        ms = statistics.median(dev_ms)
        out[f"b{batch}"] = {"apply_ms": round(ms, 4), "apply_ms_min": round(min(dev_ms), 4), "apply_ms_max": round(max(dev_ms), 4),
                            "images_per_s": round(batch * 1e3 / ms, 1), "host_plan_ms": round(statistics.median(plan_s) * 1e3, 3),
                            "host_slot_args_ms": round(statistics.median(slot_s) * 1e3, 4)}
    out["pillow_1proc_images_per_s"] = round(pillow_rate(max(args.pillow_images // 4, 1), 1), 1)
    out[f"pillow_{args.procs}proc_images_per_s"] = round(pillow_rate(args.pillow_images, args.procs), 1)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
