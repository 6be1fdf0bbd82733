#!/usr/bin/env python3
"""PLMS (PNDMScheduler) cost: the fused step kernel ``idb_cfg_plms_step`` beside ``idb_cfg_ddpm_step`` on 64x64 latents at batch 1 and
64 (back-to-back launches on one stream, device events), and the default 50-step PLMS ``__call__`` (51 UNet calls) beside the
30-step DDPM ``__call__`` at batch 1 on the full SD-2.1 graph (synthetic weights, f16, HIP graph, latent output: the VAE decode is the
same for both).  Every figure is the median of ``--repeats`` timed windows after a warm-up, with min and max.  One JSON line.

    timeout -k 10 600 python tools/bench_pndm.py [--launches 2000] [--repeats 5] [--no-pipeline] [--limit 540]

The process also ends itself after ``--limit`` seconds (SIGALRM with the default action), so a hung device cannot hold it."""
import argparse
import json
import os
import signal
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from faceposegenerator_amd import _lib as L
from faceposegenerator_amd import spec as S

DEV = "cuda:0"


def _timed(fn, repeats):
    """fn() enqueues one window of work; returns (median, min, max) milliseconds over `repeats` windows."""
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out), min(out), max(out)


def bench_steps(lib, B, launches, repeats):
    C, hw = 4, 64 * 64
    g = torch.Generator().manual_seed(0)
    eps = torch.randn(2 * B, hw, C, generator=g).to(DEV)
    lat = torch.randn(B, C, 64, 64, generator=g).to(DEV)
    noise = torch.randn(B, C, 64, 64, generator=g).to(DEV)
    hist = torch.randn(L.IDB_PLMS_SLOTS + 1, B, C, 64, 64, generator=g).to(DEV)
    # contractive scalars (|c_sample| + |c_eps| sum|w| < 1) so that thousands of in-place updates stay finite
    plms = torch.tensor([0.25, -0.25, 0.25, -0.25, 0.9, 0.4, 0.5, 0.05, 1.5], dtype=torch.float32).to(DEV)
    ddpm = torch.tensor([0.9, 0.4, 0.05, 0.5, 0.01, 1.5], dtype=torch.float32).to(DEV)
    st = torch.cuda.current_stream().cuda_stream

    def run_plms():                                              # the steady-state form: four terms, one slot written
        for _ in range(launches):
            lib.idb_cfg_plms_step(eps.data_ptr(), lat.data_ptr(), hist.data_ptr(), hist[L.IDB_PLMS_SLOTS].data_ptr(), plms.data_ptr(),
                                  B, C, hw, 2, 0, 0, 4, 3, 2, 1, L.IDB_PLMS_KEEP, st)

    def run_ddpm():
        for _ in range(launches):
            lib.idb_cfg_ddpm_step(eps.data_ptr(), lat.data_ptr(), noise.data_ptr(), ddpm.data_ptr(), None, B, C, hw, 1, 0, st)

    res = {}
    for name, fn, nbytes in (("plms", run_plms, (2 + 2 + 3 + 1) * B * C * hw * 4), ("ddpm", run_ddpm, (2 + 2 + 1) * B * C * hw * 4)):
        fn()                                                      # warm-up: code object, clocks
        torch.cuda.synchronize()
        med, lo, hi = _timed(fn, repeats)
        assert torch.isfinite(lat).all()
        res[name] = {"us_per_launch": round(1e3 * med / launches, 3), "min": round(1e3 * lo / launches, 3),
                     "max": round(1e3 * hi / launches, 3), "bytes_per_launch": nbytes}
    return res


def bench_pipeline(repeats):
    from faceposegenerator_amd import weights as W
    from faceposegenerator_amd.pipeline import StableDiffusionPipeline
    from faceposegenerator_amd.scheduler import DDPMScheduler, PNDMScheduler
    pipe = StableDiffusionPipeline(S.SD21_UNET, S.SD21_VAE, W.synth_unet(S.SD21_UNET, 1234), W.synth_vae(S.SD21_VAE, 1235),
                                   torch_dtype=torch.float16).to(DEV)
    g = torch.Generator().manual_seed(1)
    pe, ne = torch.randn(1, 77, 1024, generator=g), torch.randn(1, 77, 1024, generator=g)
    modes = {"plms_50": (PNDMScheduler.from_config(pipe.scheduler.config), dict(num_inference_steps=50, guidance_scale=7.5)),
             "ddpm_30": (DDPMScheduler.from_config(pipe.scheduler.config), dict(num_inference_steps=30, guidance_scale=5.0))}

    def call(name):
        sch, kw = modes[name]
        pipe.scheduler = sch
        return pipe(prompt_embeds=pe, negative_prompt_embeds=ne, output_type="latent", generator=torch.Generator().manual_seed(2), **kw)

    for name in modes:                                            # warm-up: eager pass + graph capture, then one replay
        call(name), call(name)
    torch.cuda.synchronize()
    times = {name: [] for name in modes}
    for _ in range(repeats):                                      # alternate the two so that drift hits both alike
        for name in modes:
            med, _, _ = _timed(lambda: call(name), 1)
            times[name].append(med)
    res = {name: {"call_ms": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)} for name, v in times.items()}
    res["plms_50_over_ddpm_30"] = round(res["plms_50"]["call_ms"] / res["ddpm_30"]["call_ms"], 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-pipeline", action="store_true")
    ap.add_argument("--limit", type=int, default=540)
    args = ap.parse_args()
    if args.repeats < 3:
        raise SystemExit("--repeats must be at least 3")
    signal.alarm(args.limit)
    if not torch.cuda.is_available():
        raise SystemExit("bench_pndm needs a GPU: there is no CPU path to time")
    lib = L.load()
    out = {"launches": args.launches, "repeats": args.repeats,
           "step": {f"b{B}": bench_steps(lib, B, args.launches, args.repeats) for B in (1, 64)}}
    if not args.no_pipeline:
        out["call_b1_512_f16"] = bench_pipeline(args.repeats)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
