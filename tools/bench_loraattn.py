#!/usr/bin/env python3
"""Training attention at the five SD-2.1 attention shapes (batch 2): idb_attention_fwd_train, idb_attention_bwd and the four
idb_lora_grad calls of one module, next to torch's own SDPA forward + backward on the same device as the yardstick.  HIP-event timed
back to back after a warm-up of every shape; each figure is a CALL time (all of the call's launches), the median of 5 windows.
FLOP/s count 4 b h n_q n_kv 64 (forward) and 10 b h n_q n_kv 64 (backward: the five products of the algorithm; the kernels issue
seven).  The lora_grad line gives the time of reading x and dy once at 8 TB/s as the floor and the share of it reached.
IDB_DTYPE selects the operand type (default f16, the reference's mixed precision).  Writes nothing; profiles/loraattn/README.md holds a
recorded run."""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from faceposegenerator_amd import _lib as L  # noqa: E402

BATCH, HBM = 2, 8.0e12
SHAPES = ((5, 4096, 4096), (10, 1024, 1024), (20, 256, 256), (20, 64, 64), (5, 4096, 77))      # heads, n_q, n_kv


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


def main():
    if not torch.cuda.is_available():
        raise SystemExit("bench_loraattn needs a HIP device (no CPU fallback: a CPU time says nothing)")
    lib, dev = L.load(), "cuda:0"
    name = os.environ.get("IDB_DTYPE", "f16")
    tdt, dt = (torch.float16, L.IDB_F16) if name == "f16" else (torch.bfloat16, L.IDB_BF16)
    st = torch.cuda.current_stream().cuda_stream
    for heads, nq, nk in SHAPES:
        c, b = heads * 64, BATCH
        self_attn = nq == nk
        rn = lambda *s: torch.randn(*s, device=dev).to(tdt)       # noqa: E731
        if self_attn:
            qkv, g = rn(b * nq, 3 * c), torch.empty(b * nq, 3 * c, device=dev, dtype=tdt)
            ptrs = (qkv.data_ptr(), 3 * c, qkv.data_ptr() + 2 * c, qkv.data_ptr() + 4 * c, 3 * c)
            gp = (g.data_ptr(), 3 * c, g.data_ptr() + 2 * c, g.data_ptr() + 4 * c, 3 * c)
        else:
            q, kv = rn(b * nq, c), rn(b * nk, 2 * c)
            gq, gkv = torch.empty_like(q), torch.empty_like(kv)
            ptrs = (q.data_ptr(), c, kv.data_ptr(), kv.data_ptr() + 2 * c, 2 * c)
            gp = (gq.data_ptr(), c, gkv.data_ptr(), gkv.data_ptr() + 2 * c, 2 * c)
        out, dout = torch.empty(b * nq, c, device=dev, dtype=tdt), rn(b * nq, c)
        lse = torch.empty(b, heads, nq, device=dev, dtype=torch.float32)
        need = lib.idb_attention_bwd_workspace_bytes(b, heads, nq, nk)
        ws = torch.empty(need, device=dev, dtype=torch.uint8)
        form = [L.C.c_int32() for _ in range(4)]
        L.check(lib.idb_attention_bwd_plan(b, heads, nq, nk, *[L.C.byref(v) for v in form]), "plan")

        def fwd():
            L.check(lib.idb_attention_fwd_train(ptrs[0], ptrs[1], ptrs[2], ptrs[3], ptrs[4], out.data_ptr(), c, lse.data_ptr(), b, heads, nq, nk, nk,
                                                0.125, dt, st), "fwd")

        def bwd():
            L.check(lib.idb_attention_bwd(ptrs[0], ptrs[1], ptrs[2], ptrs[3], ptrs[4], out.data_ptr(), c, dout.data_ptr(), c, lse.data_ptr(), gp[0],
                                          gp[1], gp[2], gp[3], gp[4], ws.data_ptr(), need, b, heads, nq, nk, nk, 0.125, dt, st), "bwd")

        reps = 5 if nq * nk > 1 << 22 else 50
        t_f, t_b = timed(fwd, reps), timed(bwd, reps)
        # torch's SDPA on the same shapes: forward alone, and forward + backward (autograd needs the forward's graph), so the
        # backward's share is the difference
        tq = torch.randn(b, heads, nq, 64, device=dev).to(tdt).requires_grad_(True)
        tk = torch.randn(b, heads, nk, 64, device=dev).to(tdt).requires_grad_(True)
        tv = torch.randn(b, heads, nk, 64, device=dev).to(tdt).requires_grad_(True)
        tg = torch.randn(b, heads, nq, 64, device=dev).to(tdt)

        def t_fwd():
            with torch.no_grad():
                F.scaled_dot_product_attention(tq, tk, tv, scale=0.125)

        def t_both():
            tq.grad = tk.grad = tv.grad = None
            F.scaled_dot_product_attention(tq, tk, tv, scale=0.125).backward(tg)

        s_f, s_fb = timed(t_fwd, reps), timed(t_both, reps)
        fl = b * heads * nq * nk * 64
        print(f"heads={heads} n_q={nq} n_kv={nk} {name} form {form[0].value}, workspace {need / 2 ** 20:.1f} MiB: fwd_train {t_f:8.1f} us "
              f"({4 * fl / t_f / 1e6:6.1f} TFLOP/s)  bwd {t_b:8.1f} us ({10 * fl / t_b / 1e6:6.1f} TFLOP/s)  |  torch SDPA fwd {s_f:8.1f} us, "
              f"fwd+bwd {s_fb:8.1f} us, bwd alone {s_fb - s_f:8.1f} us", flush=True)
        # the four adapter-gradient calls of the module (rank 4): to_q / to_k / to_v on x or the context, to_out.0 on the attention output
        x = rn(b * nq, c)
        m_kv, kdim = (b * nq, c) if self_attn else (b * nk, 1024)
        ctx = x if self_attn else rn(m_kv, kdim)
        la = {i: torch.randn(4, i, device=dev) for i in {c, kdim}}
        lb = torch.randn(c, 4, device=dev)
        da, db = {i: torch.empty(4, i, device=dev) for i in {c, kdim}}, torch.empty(c, 4, device=dev)
        calls = [(x, c, gp[0], gp[1], b * nq), (ctx, kdim, gp[2], gp[4], m_kv), (ctx, kdim, gp[3], gp[4], m_kv), (out, c, dout.data_ptr(), c, b * nq)]
        lneed = max(lib.idb_lora_grad_workspace_bytes(m, i, c, 4) for _, i, _, _, m in calls)
        lws = torch.empty(lneed, device=dev, dtype=torch.uint8)

        def lora():
            for xin, i, dyp, dyld, m in calls:
                L.check(lib.idb_lora_grad(xin.data_ptr(), i, dyp, dyld, la[i].data_ptr(), lb.data_ptr(), da[i].data_ptr(), db.data_ptr(), m, i, c, 4,
                                          1.0, lws.data_ptr(), lneed, dt, st), "lora_grad")

        t_l = timed(lora, 20)
        floor = sum(2.0 * m * (i + c) for _, i, _, _, m in calls) / HBM * 1e6
        print(f"    lora_grad x 4 (rank 4): {t_l:8.1f} us; reading x and dy once at 8 TB/s: {floor:6.1f} us = {100 * floor / t_l:4.1f} % of the time",
              flush=True)


if __name__ == "__main__":
    main()
