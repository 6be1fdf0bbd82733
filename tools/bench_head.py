#!/usr/bin/env python3
"""The FR loss head at the training loop's shapes (faceposegenerator_amd/frhead.py): B = 128 embeddings of D = 512 against C = 1000,
10 572 (a WebFace-sized set) and 70 722 (AdaFace's default) identities, for CosFace, ArcFace and AdaFace.  Three columns per shape:
  loss     header.loss(...): loss and top-1 without the B x C matrix (idb_head_loss)
  logits   header(...) + torch.nn.functional.cross_entropy + argmax: the B x C matrix written once (idb_head_logits), then torch
  torch    the reference's op sequence restated in torch on the same GPU: normalize, column norms, mm, clamp, scatter, acos / cos,
           scale, cross_entropy, argmax (fp32; the kernel re-normalised on every call, as upstream does)
Each figure is the median wall clock of a call that ends in a device synchronise (every route returns host numbers), over --reps calls.
"cold": a 512 MB buffer is overwritten before each timed call, so no operand is left in L2 or the Infinity Cache (in a training step
the backbone runs between two calls of the head); "hot": back-to-back calls.  One JSON line.

    python tools/bench_head.py [--classes 1000,10572,70722] [--batch 128] [--reps 20]
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


def torch_route(loss, kernel, s, m, h, state, emb, labels, norms):
    """(loss, correct) by torch ops, every intermediate a B x C fp32 tensor as upstream has it."""
    rows = torch.arange(emb.shape[0], device=emb.device)
    wn = kernel / torch.norm(kernel, 2, 0, True)
    if loss == "AdaFace":
        cos = torch.mm(emb, wn).clamp(-1 + EPS, 1 - EPS)
        safe = torch.clip(norms, min=0.001, max=100)
        state[0], state[1] = safe.mean(), safe.std()
        scaler = torch.clip((safe - state[0]) / (state[1] + EPS) * h, -1, 1)
        m_arc = torch.zeros_like(cos)
        m_arc.scatter_(1, labels.reshape(-1, 1), 1.0)
        theta = torch.clip(cos.acos() + m_arc * (m * scaler * -1), min=EPS, max=math.pi - EPS)
        m_cos = torch.zeros_like(cos)
        m_cos.scatter_(1, labels.reshape(-1, 1), 1.0)
        thetas = (theta.cos() - m_cos * (m + m * scaler)) * s
    else:
        cos = torch.mm(emb / torch.norm(emb, 2, 1, True), wn).clamp(-1, 1)
        m_hot = torch.zeros_like(cos)
        m_hot.scatter_(1, labels[:, None], m)
        if loss == "ArcFace":
            cos.acos_()
            cos += m_hot
            thetas = cos.cos_().mul_(s)
        else:
            cos -= m_hot
            thetas = cos * s
    value = torch.nn.functional.cross_entropy(thetas, labels)
    correct = (torch.argmax(thetas, dim=1) == labels).sum()
    return value.item(), correct.item()


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
    ap.add_argument("--classes", default="1000,10572,70722")
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
            raw = torch.randn(B, D, generator=g)
            norms = raw.norm(dim=1, keepdim=True).to(DEV)
            emb = (raw / raw.norm(dim=1, keepdim=True)).to(DEV) if loss == "AdaFace" else raw.to(DEV)
            labels = torch.randint(0, Cn, (B,), generator=g)
            d_labels = labels.to(DEV)
            kernel = header.kernel.to(DEV)
            state = [torch.tensor(20.0, device=DEV), torch.tensor(100.0, device=DEV)]
            kw = dict(norms=norms) if loss == "AdaFace" else {}

            def via_loss():
                return header.loss(emb, labels, **kw)

            def via_logits():
                thetas = header(emb, norms, labels) if loss == "AdaFace" else header(emb, labels)
                value = torch.nn.functional.cross_entropy(thetas, d_labels)
                return value.item(), (torch.argmax(thetas, dim=1) == d_labels).sum().item()

            def via_torch():
                return torch_route(loss, kernel, header.s, header.m, header.h, state, emb, d_labels, norms)

            a, b, c = via_loss(), via_logits(), via_torch()
            row = {"loss": loss, "classes": Cn, "plan": header.plan(B), "value": [round(a.loss, 6), round(b[0], 6), round(c[0], 6)],
                   "correct": [a.correct, b[1], c[1]]}
            for name, fn in (("loss", via_loss), ("logits", via_logits), ("torch", via_torch)):
                row[name + "_cold_ms"], row[name + "_cold_min_ms"] = timed(fn, args.reps, flush)
                row[name + "_hot_ms"], row[name + "_hot_min_ms"] = timed(fn, args.reps, None)
            res["rows"].append(row)
            del header, kernel
    print(json.dumps(res))


if __name__ == "__main__":
    main()
