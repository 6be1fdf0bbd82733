#!/usr/bin/env python3
"""One LoRA transformer block in training at SD-2.1's four block shapes (batch 2, context 77 x 1024): LoRATransformerBlock forward and
backward, the AdamW step over the block's 16 adapter tensors and over 256 (a whole UNet's count: the block's 16 tensors, 16 times),
next to torch's own block on the same device in the same dtype (F.layer_norm, F.linear with unmerged adapters, SDPA, F.gelu; forward
under no_grad, and forward + backward to the input and the 16 adapters) and torch.optim.AdamW(foreach) + clip_grad_norm_.  Then the
three new kernels alone: bytes moved / time against the achievable HBM figure (6.3 TB/s); at these sizes the tensors also fit the
Infinity Cache, so a figure above it is cache bandwidth.  HIP-event timed back to back after a warm-up, each figure a CALL time (all of
the call's launches), the median of 5 windows.  IDB_DTYPE selects the operand type (default f16, the reference's mixed precision).
Writes nothing; profiles/lorablock/README.md holds a recorded run."""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from faceposegenerator_amd import _lib as L  # noqa: E402
from faceposegenerator_amd.lorablock import LoRAAdamW, LoRATransformerBlock  # noqa: E402

BATCH, HBM, CTX = 2, 6.3e12, (77, 1024)
SHAPES = ((320, 4096), (640, 1024), (1280, 256), (1280, 64))      # channels, tokens


def timed(run, reps):
    for _ in range(3):
        run()
    torch.cuda.synchronize()
    out = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            run()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / reps * 1e3)
    return statistics.median(out)


def torch_block(block, tdt, dev):
    """The same block from torch ops, adapters unmerged and trainable, everything in the operand dtype."""
    sd = {k: v.to(dev).to(tdt) for k, v in block.frozen_state_dict().items()}
    par = {k: v.to(dev).to(tdt).requires_grad_(True) for k, v in block.state_dict().items()}
    p, c, s = block.prefix, block.channels, block.attn1.scaling

    def lin(mod, name, t, bias=None):
        a, b = par[f"{p}.{mod}.{name}.lora_A.weight"], par[f"{p}.{mod}.{name}.lora_B.weight"]
        return F.linear(t, sd[f"{p}.{mod}.{name}.weight"], bias) + F.linear(F.linear(t, a), b) * s

    def heads(t):
        return t.reshape(t.shape[0], t.shape[1], c // 64, 64).transpose(1, 2)

    def attn(mod, t, src):
        o = F.scaled_dot_product_attention(heads(lin(mod, "to_q", t)), heads(lin(mod, "to_k", src)), heads(lin(mod, "to_v", src)), scale=0.125)
        return lin(mod, "to_out.0", o.transpose(1, 2).reshape(t.shape), sd[f"{p}.{mod}.to_out.0.bias"])

    def norm(i, t):
        return F.layer_norm(t, (c,), sd[f"{p}.norm{i}.weight"], sd[f"{p}.norm{i}.bias"], 1e-5)

    def forward(x, ctx):
        n1 = norm(1, x)
        h1 = x + attn("attn1", n1, n1)
        h2 = h1 + attn("attn2", norm(2, h1), ctx)
        value, gate = F.linear(norm(3, h2), sd[f"{p}.ff.net.0.proj.weight"], sd[f"{p}.ff.net.0.proj.bias"]).chunk(2, -1)
        return h2 + F.linear(value * F.gelu(gate), sd[f"{p}.ff.net.2.weight"], sd[f"{p}.ff.net.2.bias"])

    return forward, par


def main():
    if not torch.cuda.is_available():
        raise SystemExit("bench_lorablock needs a HIP device (no CPU fallback: a CPU time says nothing)")
    lib, dev = L.load(), "cuda:0"
    name = os.environ.get("IDB_DTYPE", "f16")
    tdt, dt = (torch.float16, L.IDB_F16) if name == "f16" else (torch.bfloat16, L.IDB_BF16)
    st = torch.cuda.current_stream().cuda_stream
    for c, tokens in SHAPES:
        block = LoRATransformerBlock.from_synthetic(1, c, CTX[1]).init_adapters(torch.Generator().manual_seed(2)).to(dev, tdt)
        x = torch.randn(BATCH, tokens, c, device=dev).to(tdt)
        ctx = torch.randn(BATCH, CTX[0], CTX[1], device=dev).to(tdt)
        go = torch.randn(BATCH, tokens, c, device=dev).to(tdt)
        reps = 10 if tokens >= 1024 else 30
        fwd = block(x, ctx)
        t_f = timed(lambda: block(x, ctx), reps)
        t_b = timed(lambda: block.backward(fwd, go), reps)
        grads = block.backward(fwd, go).adapters
        # torch's own block
        tf, par = torch_block(block, tdt, dev)
        xg = x.clone().requires_grad_(True)

        def t_fwd():
            with torch.no_grad():
                tf(x, ctx)

        def t_both():
            xg.grad = None
            for v in par.values():
                v.grad = None
            tf(xg, ctx).backward(go)

        s_f, s_fb = timed(t_fwd, reps), timed(t_both, reps)
        print(f"c={c} tokens={tokens} {name}: block fwd {t_f:8.1f} us  bwd {t_b:8.1f} us  fwd+bwd {t_f + t_b:8.1f} us  |  torch block fwd {s_f:8.1f} us "
              f"(x {s_f / t_f:4.2f})  fwd+bwd {s_fb:8.1f} us (x {s_fb / (t_f + t_b):4.2f})", flush=True)
        # the optimiser: the whole step() of the block's 16 tensors (three launches, the norm's read-back, refresh: 16 merges and their
        # transposes), then the library call alone on 16 and on 256 tensors
        opt = LoRAAdamW(block)
        t_step = timed(lambda: opt.step(grads), 10)
        for count in (16, 256):
            shapes = [tuple(v.shape) for v in grads.values()] * (count // 16)
            w, g, m, v = ([torch.randn(s, device=dev) * k for s in shapes] for k in (0.1, 0.01, 0.01, 0.0))
            v = [t.abs() + 1e-6 for t in v]
            tab = torch.tensor([[t.data_ptr() for t in lst] for lst in (w, g, m, v)] + [[t.numel() for t in w]], dtype=torch.int64, device=dev)
            need = lib.idb_adamw_clip_table_workspace_bytes(count)
            ws = torch.empty(need, dtype=torch.uint8, device=dev)
            norm, skipped = torch.zeros(1, dtype=torch.float64, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)

            def call():
                L.check(lib.idb_adamw_clip_step_table(count, *[tab[i].data_ptr() for i in range(5)], 1e-4, 0.9, 0.999, 1e-8, 1e-2, 1.0, 1.0, 10,
                                                      norm.data_ptr(), skipped.data_ptr(), ws.data_ptr(), need, st), "adamw")

            t_lib = timed(call, 30)
            tp = [torch.nn.Parameter(t.clone()) for t in w]
            for p_, g_ in zip(tp, g):
                p_.grad = g_.clone()
            topt = torch.optim.AdamW(tp, lr=1e-4, weight_decay=1e-2, foreach=True)

            def t_call():
                torch.nn.utils.clip_grad_norm_(tp, 1.0, foreach=True)
                topt.step()

            t_t = timed(t_call, 30)
            elems = sum(t.numel() for t in w)
            print(f"    adamw {count:3d} tensors ({elems} elements): idb_adamw_clip_step_table {t_lib:7.1f} us  |  torch clip_grad_norm_ + AdamW(foreach) "
                  f"{t_t:7.1f} us (x {t_t / t_lib:4.2f})" + (f"  |  LoRAAdamW.step with refresh and read-back {t_step:7.1f} us" if count == 16 else ""),
                  flush=True)
        # the three kernels alone
        rows, inner = BATCH * tokens, 4 * c
        gamma = block.norm[0][0]
        dx = torch.empty_like(x)
        hg, dact = fwd.hg, torch.randn(rows, inner, device=dev).to(tdt)
        act, dhg = torch.empty(rows, inner, device=dev, dtype=tdt), torch.empty(rows, 2 * inner, device=dev, dtype=tdt)
        kern = {
            "idb_layernorm_bwd": (4 * rows * c * 2, lambda: L.check(lib.idb_layernorm_bwd(x.data_ptr(), go.data_ptr(), fwd.h1.data_ptr(), gamma.data_ptr(),
                                                                                            dx.data_ptr(), rows, c, 1e-5, dt, st))),
            "idb_geglu_fwd": (3 * rows * inner * 2, lambda: L.check(lib.idb_geglu_fwd(hg.data_ptr(), 2 * inner, act.data_ptr(), rows, inner, dt, st))),
            "idb_geglu_bwd": (5 * rows * inner * 2, lambda: L.check(lib.idb_geglu_bwd(hg.data_ptr(), 2 * inner, dact.data_ptr(), dhg.data_ptr(), rows, inner,
                                                                                       dt, st))),
        }
        for kname, (nbytes, run) in kern.items():
            t = timed(run, 50)
            print(f"    {kname:18s} {t:7.1f} us, {nbytes / 2 ** 20:6.1f} MiB moved: {nbytes / t / 1e6:6.2f} TB/s = {100 * nbytes / t / 1e-6 / HBM:5.1f} % of 6.3 TB/s",
                  flush=True)


if __name__ == "__main__":
    main()
