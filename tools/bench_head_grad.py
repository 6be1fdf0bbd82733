#!/usr/bin/env python3
"""The FR loss head's backward and optimiser step at the training loop's shapes (faceposegenerator_amd/frhead.py): B = 128 embeddings
of D = 512 against C = 10 572 (a WebFace-sized set) and 70 722 (AdaFace's default) identities.  Columns per shape and loss:
  grad     header.loss_and_grad(...): loss, top-1 and both gradients without a B x C matrix (idb_head_loss_grad)
  sgd      HeaderSGD.step(grad.kernel): clip_grad_norm_, SGD with momentum and weight decay, repack (idb_head_sgd_step)
  torch    a plain fp32 eager restatement on the same GPU, written here: the header's forward as upstream writes it (the kernel
           re-normalised on every call), cross_entropy, loss.backward() through autograd into the embeddings and the kernel
  torch_sgd  torch.nn.utils.clip_grad_norm_ + torch.optim.SGD(momentum 0.9, weight decay 5e-4).step() on the same gradient
Each figure is the median wall clock of a call that ends in a device synchronise (every route returns host numbers), over --reps calls
after two warm-up calls.  "cold": a 512 MB buffer is overwritten before each timed call, so no operand is left in L2 or the Infinity
Cache (in a training step the backbone runs between two calls of the head); "hot": back-to-back calls.  One JSON line.

    python tools/bench_head_grad.py [--classes 10572,70722] [--batch 128] [--reps 20]
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from faceposegenerator_amd import frhead as H

DEV = torch.device("cuda:0")
EPS = 1e-3


def torch_forward(loss, kernel, s, m, h, emb, labels, norms):
    """thetas [B, C] by torch ops, differentiable in emb and kernel; every intermediate a B x C fp32 tensor, as upstream has it."""
    wn = kernel / torch.norm(kernel, 2, 0, True)
    if loss == "AdaFace":
        cos = torch.mm(emb, wn).clamp(-1 + EPS, 1 - EPS)
        safe = torch.clip(norms, min=0.001, max=100).clone().detach()
        scaler = torch.clip((safe - safe.mean()) / (safe.std() + EPS) * h, -1, 1)
        m_arc = torch.zeros_like(cos)
        m_arc.scatter_(1, labels.reshape(-1, 1), 1.0)
        theta = torch.clip(cos.acos() + m_arc * (m * scaler * -1), min=EPS, max=math.pi - EPS)
        m_cos = torch.zeros_like(cos)
        m_cos.scatter_(1, labels.reshape(-1, 1), 1.0)
        return (theta.cos() - m_cos * (m + m * scaler)) * s
    cos = torch.mm(emb / torch.norm(emb, 2, 1, True), wn).clamp(-1, 1)
    m_hot = torch.zeros_like(cos)
    m_hot.scatter_(1, labels[:, None], m)
    if loss == "ArcFace":
        return (cos.acos() + m_hot).cos() * s
    return (cos - m_hot) * s


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--classes", default="10572,70722")
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--losses", default="CosFace,ArcFace,AdaFace")
    args = ap.parse_args()
    B, D = args.batch, args.dim
    flush = torch.zeros(512 << 18, dtype=torch.int32, device=DEV)            # 512 MB, twice the Infinity Cache
    g = torch.Generator().manual_seed(0)
    res = {"batch": B, "dim": D, "reps": args.reps, "rows": []}
    for Cn in [int(c) for c in args.classes.split(",")]:
        for loss in args.losses.split(","):
            header = H.MarginHeader.from_synthetic(D, Cn, 1, loss).to(DEV)
            opt = H.HeaderSGD(header, 1e-4)                                  # a small step: the timed repeats leave the header usable
            raw = torch.randn(B, D, generator=g)
            norms = raw.norm(dim=1, keepdim=True).to(DEV)
            emb = (raw / raw.norm(dim=1, keepdim=True)).to(DEV) if loss == "AdaFace" else raw.to(DEV)
            labels = torch.randint(0, Cn, (B,), generator=g)
            d_labels = labels.to(DEV)
            kw = dict(norms=norms) if loss == "AdaFace" else {}
            t_kernel = torch.nn.Parameter(header.kernel.to(DEV).clone())
            t_emb = emb.clone().requires_grad_(True)
            t_opt = torch.optim.SGD([t_kernel], lr=1e-4, momentum=0.9, weight_decay=5e-4)

            def via_grad():
                return header.loss_and_grad(emb, labels, **kw)

            def via_torch():
                t_kernel.grad = t_emb.grad = None
                thetas = torch_forward(loss, t_kernel, header.s, header.m, header.h, t_emb, d_labels, norms)
                value = torch.nn.functional.cross_entropy(thetas, d_labels)
                correct = (torch.argmax(thetas, dim=1) == d_labels).sum()
                value.backward()
                return value.item(), correct.item()

            out, grad = via_grad()
            value, _ = via_torch()
            scale = t_kernel.grad.abs().max().item()
            row = {"loss": loss, "classes": Cn, "grad_plan": header.grad_plan(B), "value": [round(out.loss, 6), round(value, 6)],
                   "max_abs_diff_d_kernel": (grad.kernel - t_kernel.grad).abs().max().item(), "max_abs_d_kernel": scale,
                   "max_abs_diff_d_emb": (grad.embeddings - t_emb.grad).abs().max().item(), "max_abs_d_emb": t_emb.grad.abs().max().item()}
            g_ours, g_torch = grad.kernel.clone(), t_kernel.grad.clone()

            def via_sgd():
                return opt.step(g_ours)

            def via_torch_sgd():
                t_kernel.grad = g_torch.clone()
                norm = torch.nn.utils.clip_grad_norm_([t_kernel], 5.0)
                t_opt.step()
                return norm.item()

            for name, fn in (("grad", via_grad), ("torch", via_torch), ("sgd", via_sgd), ("torch_sgd", via_torch_sgd)):
                row[name + "_cold_ms"], row[name + "_cold_min_ms"] = timed(fn, args.reps, flush)
                row[name + "_hot_ms"], row[name + "_hot_min_ms"] = timed(fn, args.reps, None)
            row["torch_over_grad_cold"] = round(row["torch_cold_ms"] / row["grad_cold_ms"], 3)
            row["torch_over_grad_hot"] = round(row["torch_hot_ms"] / row["grad_hot_ms"], 3)
            res["rows"].append(row)
            del header, opt, t_kernel, t_opt
    print(json.dumps(res))


if __name__ == "__main__":
    main()
