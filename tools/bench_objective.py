#!/usr/bin/env python3
"""Step time of the training objective's forward pass (faceposegenerator_amd/objective.py) at SD-2.1 size with synthetic weights, f16,
batch [1 instance; 1 prior] at 512 x 512: one ``step_losses`` with which_loss "" and one with "identity" (MTCNN + ArcFace r100 on the
decoded x0), wall-clock with a synchronisation per step, and the device time of each new kernel beside the bytes it moves.  One JSON
line.  New measurements: there is no earlier figure to compare them with.

    timeout -k 10 600 python tools/bench_objective.py [--iters 5] [--kernel-iters 50] [--limit 540]

With synthetic detector weights and a synthetic image the detector's first box need not be usable (none found, or a regressed box
that is empty after the reference's clipping); the identity step then continues with a fixed box so that the crop, ArcFace and the
loss kernel are part of the time (``mtcnn_found`` / ``mtcnn_box_usable`` say how often the detector's own box was found / kept).
The process ends itself after ``--limit`` seconds (SIGALRM with the default action), so a hung device cannot hold it."""
import argparse
import json
import os
import signal
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from faceposegenerator_amd import arcface as A
from faceposegenerator_amd import mtcnn as M
from faceposegenerator_amd import objective as OB
from faceposegenerator_amd import spec as S
from faceposegenerator_amd import weights as W
from faceposegenerator_amd.pipeline import StableDiffusionPipeline

DEV = "cuda:0"


def device_us(fn, iters):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--kernel-iters", type=int, default=50)
    ap.add_argument("--limit", type=int, default=540)
    args = ap.parse_args()
    signal.alarm(args.limit)
    if not torch.cuda.is_available():
        raise SystemExit("bench_objective needs a GPU: there is no CPU path to time")
    pipe = StableDiffusionPipeline.from_synthetic(torch_dtype=torch.float16).to(DEV)
    pipe.set_vae_encoder_weights(W.synth_vae_encoder(S.SD21_VAE))
    arc = A.ArcFace.from_synthetic("r100", 0, torch.float16).to(DEV)
    det = M.MTCNN(image_size=112, margin=0, device=DEV)
    g = torch.Generator().manual_seed(0)
    x = torch.rand(2, 3, 512, 512, generator=g) * 2 - 1
    emb = torch.randn(2, 512, generator=g)
    ehs = torch.randn(2, 77, S.SD21_UNET.cross_attention_dim, generator=g)
    found, usable, last_box = [], [], []

    def detector(images):
        boxes = det.detect(images, landmarks=False)[0]
        found.append(boxes[0] is not None)
        ok = [b is not None and OB.clip_box(b[0], images.shape[1]) is not None for b in boxes]
        usable.append(ok[0])
        last_box[:] = [] if boxes[0] is None else [round(float(v), 1) for v in boxes[0][0]]
        return [b if k else np.array([[128.0, 96.0, 384.0, 416.0]]) for b, k in zip(boxes, ok)]

    out = {"dtype": "f16", "batch": "1+1", "size": 512, "iters": args.iters}
    for which in ("", "identity"):
        obj = OB.TrainingObjective(pipe, arcface=arc, mtcnn=det, which_loss=which)
        times = []
        for it in range(args.iters + 1):                          # the first step packs weights and fills the arena: not timed
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = obj.step_losses(x, emb, ehs, generator=torch.Generator().manual_seed(it), detector=detector if which else None)
            torch.cuda.synchronize()
            if it:
                times.append((time.perf_counter() - t0) * 1e3)
        out[f"step_ms_{which or 'plain'}"] = round(statistics.median(times), 2)
        out[f"combined_{which or 'plain'}"] = round(r["combined"], 5)
        out[f"detected_{which or 'plain'}"] = r["detected"]
    out["mtcnn_found"], out["mtcnn_box_usable"] = f"{sum(found)}/{len(found)}", f"{sum(usable)}/{len(usable)}"
    out["last_first_box"] = last_box

    # the new kernels on this step's shapes: device time per call, bytes read + written
    ac = pipe.scheduler.alphas_cumprod.float().to(DEV)
    ts = torch.tensor([400, 700], dtype=torch.int32, device=DEV)
    lat, nz = torch.randn(2, 4, 64, 64, device=DEV), torch.randn(2, 4, 64, 64, device=DEV)
    noisy, target = OB.diffuse_targets(lat, nz, ts, ac, False)
    pred = torch.randn(2 * 64 * 64, 4, device=DEV)
    img = torch.rand(1, 512, 512, 3, device=DEV) * 255
    box = np.array([[0, 96, 416, 128, 384]], dtype=np.int32)
    full = np.array([[0, 0, 512, 0, 512]], dtype=np.int32)
    feat, pos = torch.randn(1, 512, device=DEV), torch.randn(1, 512, device=DEV)
    nlat = lat.numel() * 4
    kernels = {
        "idb_diffuse_targets": (lambda: OB.diffuse_targets(lat, nz, ts, ac, False), 4 * nlat),
        "idb_objective_mse_x0": (lambda: OB.mse_x0(pred, target, noisy, ts, ac, False, pred_nhwc=True), 4 * nlat),
        "idb_crop_resize_bilinear_f32": (lambda: OB.crop_resize_bilinear(img, box), 320 * 256 * 12 + 3 * 112 * 112 * 4),
        "idb_crop_resize_area_f32 (512 -> 308, pyramid level 0)": (lambda: det._resample(img, full, 308, 308), 512 * 512 * 12 + 3 * 308 * 308 * 4),
        "idb_identity_losses": (lambda: OB.identity_losses(feat, pos), 2 * 512 * 4 + 8),
    }
    out["kernels"] = {}
    for name, (fn, nbytes) in kernels.items():
        us = device_us(fn, args.kernel_iters)                     # includes the output allocation of the Python wrapper
        out["kernels"][name] = {"us": round(us, 2), "bytes": nbytes, "GB_per_s": round(nbytes / us / 1e3, 1)}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
