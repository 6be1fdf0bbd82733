#!/usr/bin/env python3
"""One (resnet, attention) stage of the UNet in training at SD-2.1's shapes (batch 2, context 77 x 1024, time_embed_dim 1280):
idb_groupnorm_bwd alone (time, and bytes moved / time against the achievable HBM figure, 6.3 TB/s: x and dy are read twice, add once, dx
written once, six tensor passes; at these sizes the tensors also fit the Infinity Cache, so a figure above it is cache bandwidth), then
TrainResnetBlock, LoRATransformer2D and LoRAStage forward and backward, next to torch's own stage on the same device in the same dtype
(F.group_norm, F.silu, F.conv2d, F.linear, the block of tools/bench_lorablock.py with unmerged trainable adapters; forward under
no_grad, and forward + backward to the input and the 16 adapters).  HIP-event timed back to back after a warm-up, each figure a CALL time
(all of the call's launches), the median of 5 windows.  IDB_DTYPE selects the operand type (default f16, the reference's mixed
precision).  Writes nothing; profiles/lorastage/README.md holds a recorded run."""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from bench_lorablock import timed, torch_block  # noqa: E402
from faceposegenerator_amd import _lib as L  # noqa: E402
from faceposegenerator_amd.lorastage import LoRAStage, LoRATransformer2D, TrainResnetBlock  # noqa: E402

BATCH, HBM, CTX, TED = 2, 6.3e12, (77, 1024), 1280
KERNEL_SHAPES = ((320, 0, 64), (640, 0, 32), (1280, 0, 16), (1280, 1280, 16), (1280, 0, 8))       # c0, c1, side; 2560 = 1280 | 1280, the up path
STAGES = ((320, 320, 0, 64), (320, 640, 0, 32), (640, 1280, 0, 16), (1280, 1280, 1280, 16), (1280, 1280, 0, 8))      # cin, cout, skip, side


def bench_kernel(lib, dev, tdt, dt, name):
    st = torch.cuda.current_stream().cuda_stream
    for c0, c1, side in KERNEL_SHAPES:
        hw, c, G = side * side, c0 + c1, 32
        x0 = torch.randn(BATCH, hw, c0, device=dev).to(tdt)
        x1 = torch.randn(BATCH, hw, c1, device=dev).to(tdt) if c1 else None
        dy, add = torch.randn(BATCH, hw, c, device=dev).to(tdt), torch.randn(BATCH, hw, c, device=dev).to(tdt)
        gamma, beta = torch.rand(c, device=dev) + 0.5, torch.randn(c, device=dev) * 0.1
        part = torch.empty(BATCH * 64 * G * 2, device=dev)
        chunks = C.c_int32()
        p1 = None if x1 is None else x1.data_ptr()
        L.check(lib.idb_groupnorm_stats(x0.data_ptr(), c0, p1, c1, BATCH, hw, G, part.data_ptr(), part.numel() * 4, C.byref(chunks), dt, st), "stats")
        dx0 = torch.empty_like(x0)
        dx1 = None if x1 is None else torch.empty_like(x1)
        need = lib.idb_groupnorm_bwd_workspace_bytes(BATCH, hw, G)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        plan = [C.c_int32() for _ in range(5)]
        L.check(lib.idb_groupnorm_bwd_plan(c0, c1, BATCH, hw, G, *[C.byref(v) for v in plan]), "plan")
        for silu, with_add in ((1, True), (0, True), (1, False)):
            def run():
                L.check(lib.idb_groupnorm_bwd(x0.data_ptr(), c0, p1, c1, part.data_ptr(), chunks.value, dy.data_ptr(), add.data_ptr() if with_add else None,
                                              gamma.data_ptr(), beta.data_ptr(), 1e-5, silu, dx0.data_ptr(), None if dx1 is None else dx1.data_ptr(), BATCH, hw,
                                              G, dt, ws.data_ptr(), need, st), "idb_groupnorm_bwd")
            t = timed(run, 50)
            nbytes = (5 + with_add) * BATCH * hw * c * 2
            print(f"idb_groupnorm_bwd c={c0}+{c1} {side}x{side} silu={silu} add={int(with_add)} {name}: {t:7.1f} us (2 launches; slices of {plan[0].value} x "
                  f"{plan[1].value}, {plan[2].value} chunks, {plan[4].value} apply blocks), {nbytes / 2 ** 20:6.1f} MiB moved: {nbytes / t / 1e6:6.2f} TB/s = "
                  f"{100 * nbytes / t / 1e-6 / HBM:5.1f} % of 6.3 TB/s", flush=True)


def torch_stage(stage, tdt, dev):
    """The same stage from torch ops (NCHW, as upstream), everything in the operand dtype, the adapters unmerged and trainable."""
    r, tr = stage.resnet, stage.transformer
    sd = {k: v.to(dev).to(tdt) for k, v in stage.frozen_state_dict().items()}
    p, q, c, G = r.prefix, tr.prefix, tr.channels, r.groups
    block, par = torch_block(tr.blocks[0], tdt, dev)

    def forward(x, temb, ctx, skip):
        cat = x if skip is None else torch.cat([x, skip], 1)
        h = F.silu(F.group_norm(cat, G, sd[f"{p}.norm1.weight"], sd[f"{p}.norm1.bias"], r.eps))
        h = F.conv2d(h, sd[f"{p}.conv1.weight"], sd[f"{p}.conv1.bias"], padding=1)
        h = h + F.linear(F.silu(temb), sd[f"{p}.time_emb_proj.weight"], sd[f"{p}.time_emb_proj.bias"])[:, :, None, None]
        h = F.silu(F.group_norm(h, G, sd[f"{p}.norm2.weight"], sd[f"{p}.norm2.bias"], r.eps))
        h = F.conv2d(h, sd[f"{p}.conv2.weight"], sd[f"{p}.conv2.bias"], padding=1)
        h = h + (F.conv2d(cat, sd[f"{p}.conv_shortcut.weight"], sd[f"{p}.conv_shortcut.bias"]) if r.has_shortcut else cat)
        b, _, hh, ww = h.shape
        t = F.group_norm(h, G, sd[f"{q}.norm.weight"], sd[f"{q}.norm.bias"], tr.eps).permute(0, 2, 3, 1).reshape(b, hh * ww, c)
        t = block(F.linear(t, sd[f"{q}.proj_in.weight"], sd[f"{q}.proj_in.bias"]), ctx)
        t = F.linear(t, sd[f"{q}.proj_out.weight"], sd[f"{q}.proj_out.bias"])
        return t.reshape(b, hh, ww, c).permute(0, 3, 1, 2) + h

    return forward, par


def main():
    if not torch.cuda.is_available():
        raise SystemExit("bench_lorastage needs a HIP device (no CPU fallback: a CPU time says nothing)")
    lib, dev = L.load(), "cuda:0"
    name = os.environ.get("IDB_DTYPE", "f16")
    tdt, dt = (torch.float16, L.IDB_F16) if name == "f16" else (torch.bfloat16, L.IDB_BF16)
    bench_kernel(lib, dev, tdt, dt, name)
    for cin, cout, skip, side in STAGES:
        r = TrainResnetBlock.from_synthetic(1, cin, cout, skip, TED)
        tr = LoRATransformer2D.from_synthetic(2, cout, CTX[1]).init_adapters(torch.Generator().manual_seed(3))
        stage = LoRAStage(r, tr).to(dev, tdt)
        x = torch.randn(BATCH, side, side, cin, device=dev).to(tdt)
        sk = torch.randn(BATCH, side, side, skip, device=dev).to(tdt) if skip else None
        temb = torch.randn(BATCH, TED, device=dev)
        ctx = torch.randn(BATCH, CTX[0], CTX[1], device=dev).to(tdt)
        go = torch.randn(BATCH, side, side, cout, device=dev).to(tdt)
        reps = 10 if side >= 32 else 30
        rf = r(x, temb, sk)
        tf_ = tr(rf.out, ctx)
        sf = stage(x, temb, ctx, sk)
        t = {"resnet fwd": timed(lambda: r(x, temb, sk), reps), "resnet bwd": timed(lambda: r.backward(rf, go), reps),
             "transformer2d fwd": timed(lambda: tr(rf.out, ctx), reps), "transformer2d bwd": timed(lambda: tr.backward(tf_, go), reps),
             "stage fwd": timed(lambda: stage(x, temb, ctx, sk), reps), "stage bwd": timed(lambda: stage.backward(sf, go), reps)}
        # torch's own stage, NCHW
        fwd, par = torch_stage(stage, tdt, dev)
        xn = x.permute(0, 3, 1, 2).contiguous()
        skn = None if sk is None else sk.permute(0, 3, 1, 2).contiguous()
        gon = go.permute(0, 3, 1, 2).contiguous()
        tembt = temb.to(tdt)
        xg = xn.clone().requires_grad_(True)
        skg = None if skn is None else skn.clone().requires_grad_(True)

        def t_fwd():
            with torch.no_grad():
                fwd(xn, tembt, ctx, skn)

        def t_both():
            xg.grad = None
            if skg is not None:
                skg.grad = None
            for v in par.values():
                v.grad = None
            fwd(xg, tembt, ctx, skg).backward(gon)

        s_f, s_fb = timed(t_fwd, reps), timed(t_both, reps)
        ours = t["stage fwd"] + t["stage bwd"]
        print(f"stage {cin}+{skip}->{cout} {side}x{side} {name}: " + "  ".join(f"{k} {v:8.1f} us" for k, v in t.items()), flush=True)
        print(f"    stage fwd+bwd {ours:8.1f} us  |  torch stage fwd {s_f:8.1f} us (x {s_f / t['stage fwd']:4.2f})  fwd+bwd {s_fb:8.1f} us (x {s_fb / ours:4.2f})",
              flush=True)


if __name__ == "__main__":
    main()
