#!/usr/bin/env python3
"""GroupNorm+SiLU fused into the patch-resident 3x3 conv (idb_conv_patch_kernel<.., GN = true>) at B_eff 2, cold weights rotated inside a
HIP graph.  Per shape that fuses, three timings on the tile and split the fused plan takes (tile = 100 + shape, so the launches differ by
the fusion alone): the unfused conv on a normalised input, idb_groupnorm(partials from the producer) + that conv, and ONE idb_gemm with
gn_in_*.  us per layer incl. the split-K reduce.  `fused - conv` is what the fusion costs inside the kernel; a least-squares line through
it over the channel chunks a workgroup walks gives the prologue (intercept) and the steady-state cost per chunk (slope).
Usage: python tools/bench_gnfuse.py [B_eff]; IDB_LIB selects the library."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from faceposegenerator_amd import spec as S, _lib as L
from faceposegenerator_amd.engine import HipEngine
beff = int(sys.argv[1]) if len(sys.argv) > 1 else 2
eng = HipEngine(S.TINY_UNET, S.TINY_VAE, None, None, "cuda:0", os.environ.get("IDB_DTYPE", "f16"))
dev = eng.device
# (h, [channels of the normalised K segments], cout): ResnetBlock2D norm1+conv1 / norm2+conv2 of the SD 2.1 UNet, single and skip-concat
shapes = [(64, [320], 320), (32, [640], 640), (16, [1280], 1280), (8, [1280], 1280), (8, [1280, 1280], 1280),
          (32, [640, 640], 640), (32, [640, 320], 640), (16, [1280, 1280], 1280), (16, [1280, 640], 1280)]
G = 32
print(f"library {L.LIB_PATH}  B_eff {beff}  {eng.tdt}", flush=True)
fit = []
for (h, cs, cout) in shapes:
    cin, hw = sum(cs), h * h
    nbuf = max(2, min(16, int(400e6 // (cout * cin * 9 * 2))))
    ws, wrefs = [], []
    for _ in range(nbuf):
        wc = torch.randn(cout, cin, 3, 3, device=dev) * (9 * cin) ** -0.5
        wrefs.append(eng.tile_weight(eng._pack_conv(wc)))
        # K order of several normalised segments: [src0 taps][src1 taps]
        ws.append(wrefs[-1] if len(cs) == 1 else
                  eng.tile_weight(torch.cat([eng._pack_conv(wc[:, :cs[0]].contiguous()), eng._pack_conv(wc[:, cs[0]:].contiguous())], dim=1).contiguous()))
        del wc
    xs = [torch.randn(beff * hw, c, device=dev).to(eng.tdt) for c in cs]
    gamma, beta, bias = torch.rand(cin, device=dev) + 0.5, torch.randn(cin, device=dev) * 0.1, torch.randn(cout, device=dev)
    if len(cs) == 1:        # the producer's layout: per 64-row chunk and group {sum, sum of squares}
        xf = xs[0].float().view(beff, max(1, hw // 64), min(64, hw), G, cin // G)
        part = torch.stack([xf.sum(dim=(2, 4)), (xf * xf).sum(dim=(2, 4))], dim=-1).contiguous()
        chunks = max(1, hw // 64)
    else:
        part, chunks = eng.gn_statistics(xs[0], cs[0], xs[1], cs[1], beff, hw, G)
        part = part.clone()
    if not eng.fuses_groupnorm([(c, 9) for c in cs], ws[0], cout, beff, h, h, G, len(cs)):
        print(f"{h:2d}x{h:<2d} {'+'.join(map(str, cs)):>9s}->{cout:4d}: the plan does not fuse", flush=True)
        continue
    gn_in = (part, chunks, G, 1e-5, gamma, beta, True, len(cs))
    fsrcs = [(x, c, 9, h, h, 0) for x, c in zip(xs, cs)]
    eng.launch_log = []
    eng.gemm(fsrcs, ws[0], cout, beff, h, h, bias=bias, gn_in=gn_in)
    torch.cuda.synchronize()
    tile, sk = eng.launch_log[-1]["tile"] - 1000, eng.launch_log[-1]["split_k"]
    eng.launch_log = None
    if tile // 10 != 10:
        print(f"{h:2d}x{h:<2d} {'+'.join(map(str, cs)):>9s}->{cout:4d}: fuses on tile {tile}, not the patch-resident conv", flush=True)
        continue
    xn0 = torch.empty(beff * hw, cin, device=dev, dtype=eng.tdt)

    def gn(out):
        L.check(eng.lib.idb_groupnorm(xs[0].data_ptr(), cs[0], None if len(cs) == 1 else xs[1].data_ptr(), 0 if len(cs) == 1 else cs[1], beff, hw, G,
                                      1e-5, gamma.data_ptr(), beta.data_ptr(), 1, out.data_ptr(), eng.dt, eng._gn_ws.data_ptr(), eng._gn_ws.numel(),
                                      None, 0, part.data_ptr() if len(cs) == 1 else None, chunks if len(cs) == 1 else 0,
                                      torch.cuda.current_stream().cuda_stream), "gn")
    gn(xn0)

    def run(name, i):
        eng.arena.reset()
        if name == "fused":
            return eng.gemm(fsrcs, ws[i % nbuf], cout, beff, h, h, bias=bias, tile=tile, split_k=sk, gn_in=gn_in)
        xn = xn0
        if name == "gn+conv":
            xn = eng.arena.alloc((beff * hw, cin), eng.tdt)
            gn(xn)
        return eng.gemm([(xn, cin, 9, h, h, 0)], wrefs[i % nbuf], cout, beff, h, h, bias=bias, tile=tile, split_k=sk)
    res, outs = {}, {}
    for name in ("conv", "gn+conv", "fused"):
        for i in range(nbuf): o = run(name, i)
        torch.cuda.synchronize()
        outs[name] = o.clone()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for i in range(nbuf): run(name, i)
        g.replay(); torch.cuda.synchronize()
        best = 1e9
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); g.replay(); g.replay(); e1.record(); torch.cuda.synchronize()
            best = min(best, e0.elapsed_time(e1) / (2 * nbuf) * 1e3)
        res[name] = best
        del g
    same = torch.equal(outs["fused"], outs["gn+conv"])
    nch = cin // 64 / sk
    fit.append((nch, res["fused"] - res["conv"]))
    print(f"{h:2d}x{h:<2d} {'+'.join(map(str, cs)):>9s}->{cout:4d} tile {tile} split {sk:2d} chunks/wg {nch:5.2f}: conv {res['conv']:6.2f}  gn+conv {res['gn+conv']:6.2f}  "
          f"fused {res['fused']:6.2f} us   fused-(gn+conv) {res['fused'] - res['gn+conv']:+6.2f}  fused-conv {res['fused'] - res['conv']:+6.2f}  "
          f"bit-identical {same}", flush=True)
    del ws, wrefs
if len(fit) >= 2:
    n = len(fit)
    mx, my = sum(a for a, _ in fit) / n, sum(b for _, b in fit) / n
    sxx = sum((a - mx) ** 2 for a, _ in fit)
    slope = sum((a - mx) * (b - my) for a, b in fit) / sxx if sxx else 0.0
    icpt = my - slope * mx
    rms = (sum((b - icpt - slope * a) ** 2 for a, b in fit) / n) ** 0.5
    print(f"fused - conv = {icpt:+.2f} us (prologue) {slope:+.3f} us x chunks per workgroup; rms residual {rms:.2f} us over {n} shapes", flush=True)
