#!/usr/bin/env python3
"""The backbone's embedding stage in training at the loop's shape (faceposegenerator_amd/frtail.py): B = 128 feature maps of
7 x 7 x 512 through bn2 -> dropout -> fc (25 088 -> 512) -> features -> F.normalize, backward, and the clipped SGD step.  Columns:
  forward     stage(feature_map, keep)                            (idb_tail_forward)
  backward    stage.backward(out, g)                              (idb_tail_backward)
  sgd         StageSGD.step(grad)                                 (idb_sgd_clip_step, csrc/idb_sgd.hip)
  train_step  frtail.train_step with a CosFace header of --classes identities (both backwards, both optimiser steps)
  torch_*     a plain fp32 eager restatement on the same GPU, written here: nn.BatchNorm2d -> flatten -> x * keep / (1 - p) ->
              nn.Linear -> nn.BatchNorm1d (weight frozen) -> F.normalize, autograd's backward(), clip_grad_norm_ + torch.optim.SGD
Each figure is the median wall clock over --reps calls after two warm-up calls; every call ends in a device-to-host read.  "cold": a
512 MB buffer is overwritten before each timed call (in a training step the trunk runs between two calls of the stage); "hot":
back-to-back calls.  Also: the bytes every large launch must move and its FLOPs against 6.0 TB/s of achievable HBM bandwidth and
155 TFLOP/s of f32 matrix rate (the floor of each launch is the larger of the two times), and the peak extra device memory of a step.
One JSON line.

    python tools/bench_tail.py [--batch 128] [--reps 20] [--classes 10572]
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

from faceposegenerator_amd import frhead as H
from faceposegenerator_amd import frtail as T

DEV = torch.device("cuda:0")
HBM, F32_MATRIX = 6.0e12, 155e12


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--classes", type=int, default=10572)
    args = ap.parse_args()
    B, ch, hw, n, p = args.batch, 512, 49, 512, 0.4
    K = ch * hw
    flush = torch.zeros(512 << 18, dtype=torch.int32, device=DEV)            # 512 MB, twice the Infinity Cache
    g = torch.Generator().manual_seed(0)
    stage = T.EmbeddingStage.from_synthetic(1, ch, hw, n, dropout=p).to(DEV)
    opt = T.StageSGD(stage, 1e-4)
    header = H.MarginHeader.from_synthetic(n, args.classes, 1, "CosFace").to(DEV)
    opt_h = H.HeaderSGD(header, 1e-4)
    x = torch.randn(B, 7, 7, ch, generator=g).to(DEV)
    keep_up = (torch.rand(B, K, generator=g) >= p).to(DEV)
    labels = torch.randint(0, args.classes, (B,), generator=g)
    cot = (torch.randn(B, n, generator=g) / B).to(DEV)

    # the eager restatement, from the same parameters
    sd = stage.state_dict()
    bn2, fc, feat = nn.BatchNorm2d(ch).to(DEV), nn.Linear(K, n).to(DEV), nn.BatchNorm1d(n).to(DEV)
    with torch.no_grad():
        for mod, name in ((bn2, "bn2"), (feat, "features")):
            for key in ("weight", "bias", "running_mean", "running_var"):
                getattr(mod, key).copy_(sd[f"{name}.{key}"])
        fc.weight.copy_(sd["fc.weight"])
        fc.bias.copy_(sd["fc.bias"])
    feat.weight.requires_grad = False
    params = [bn2.weight, bn2.bias, fc.weight, fc.bias, feat.bias]
    t_opt = torch.optim.SGD(params, lr=1e-4, momentum=0.9, weight_decay=5e-4)
    x_nchw = x.permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    keep_f = keep_up.float() / (1 - p)
    state = {}

    def fwd():
        state["out"] = stage(x, keep=keep_up)
        return state["out"].norms.cpu()

    def bwd():
        state["grad"] = stage.backward(state["out"], cot)
        return state["grad"].fc_bias.cpu()

    def sgd():
        return opt.step(state["grad"])

    def step():
        return T.train_step(stage, header, opt, opt_h, x, labels, keep=keep_up)["loss"]

    def t_fwd():
        state["t_emb"] = F.normalize(feat(fc(bn2(x_nchw).flatten(1) * keep_f)))
        return state["t_emb"].norm(dim=1).cpu()

    def t_bwd():
        for q in params + [x_nchw]:
            q.grad = None
        state["t_emb"].backward(cot, retain_graph=True)
        return fc.bias.grad.cpu()

    def t_sgd():
        norm = torch.nn.utils.clip_grad_norm_(params, 5.0)
        t_opt.step()
        return norm.item()

    def t_all():
        t_fwd()
        t_bwd()
        return t_sgd()

    def ours_all():
        fwd()
        bwd()
        return sgd()

    fwd(), bwd(), t_fwd(), t_bwd()
    gw_up = state["grad"].fc_weight_upstream()
    res = {"batch": B, "shape": [ch, hw, n], "reps": args.reps, "plan": stage.plan(B),
           "max_abs_diff_emb": (state["out"].embeddings - state["t_emb"]).abs().max().item(),
           "max_abs_diff_d_fc_weight": (gw_up - fc.weight.grad).abs().max().item(), "max_abs_d_fc_weight": fc.weight.grad.abs().max().item(),
           "max_abs_diff_d_input": (state["grad"].input.permute(0, 3, 1, 2) - x_nchw.grad).abs().max().item(),
           "max_abs_d_input": x_nchw.grad.abs().max().item()}
    for name, fn in (("forward", fwd), ("backward", bwd), ("sgd", sgd), ("train_step", step), ("torch_forward", t_fwd),
                     ("torch_backward", t_bwd), ("torch_sgd", t_sgd)):
        res[name + "_cold_ms"], res[name + "_cold_min_ms"] = timed(fn, args.reps, flush)
        res[name + "_hot_ms"], res[name + "_hot_min_ms"] = timed(fn, args.reps, None)
    res["peak_extra_mib"] = round(peak_extra(ours_all), 1)
    res["torch_peak_extra_mib"] = round(peak_extra(t_all), 1)
    ks = stage.plan(B)[0]
    w_bytes, x_bytes, m_bytes, flops = 4 * n * K, 4 * B * K, B * K, 2.0 * B * K * n
    floors = {"fc": (w_bytes + x_bytes + m_bytes + 4 * ks * B * n, flops), "dgrad": (w_bytes + 2 * x_bytes + m_bytes, flops),
              "wgrad": (w_bytes + x_bytes + m_bytes, flops), "dx": (3 * x_bytes, 0.0), "sgd": (6 * w_bytes, 0.0)}            # grad twice (norm, step), weight and buffer read and written
    res["floors_us"] = {k: {"bytes": b, "flops": f, "hbm_us": round(b / HBM * 1e6, 1), "matrix_us": round(f / F32_MATRIX * 1e6, 1)}
                        for k, (b, f) in floors.items()}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
