"""The prologue of the patch-resident 3x3 conv with GroupNorm(+SiLU) fused into its patch loaders (idb_conv_patch_kernel<.., GN = true>):
the group statistics are finalised by MFMA waves and the first halo patch is normalised by all twelve non-weight waves.  Every case
compares the fused launch (gn_in, forced tile 100 + shape) with idb_groupnorm + the unfused patch-resident conv on the same tile and
split, both from the same producer-layout partial sums: the operands and the accumulation order are the same, so the outputs must be
equal bit for bit.  Each fused launch runs twice into the same buffers and the two results must be equal too (a race on the patch
buffers or on the statistics shows as a difference between runs)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
G = 32


@pytest.fixture(scope="module", params=["bf16", "f16"])
def eng(request, lib):
    from faceposegenerator_amd import spec as S
    from faceposegenerator_amd.engine import HipEngine
    return HipEngine(S.TINY_UNET, S.TINY_VAE, None, None, DEV, request.param)


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(DEV)


def _groupnorm(eng, xs, cs, b, hw, gamma, beta, silu, part, chunks):
    from faceposegenerator_amd import _lib as L
    xn = torch.empty((b * hw, sum(cs)), dtype=eng.tdt, device=DEV)
    two = len(xs) == 2
    L.check(eng.lib.idb_groupnorm(xs[0].data_ptr(), cs[0], xs[1].data_ptr() if two else None, cs[1] if two else 0, b, hw, G, 1e-5,
                                  gamma.data_ptr(), beta.data_ptr(), int(silu), xn.data_ptr(), eng.dt, eng._gn_ws.data_ptr(), eng._gn_ws.numel(),
                                  None, 0, None if part is None else part.data_ptr(), chunks, 0), "idb_groupnorm")
    return xn


def _fused_twice(eng, srcs, w, cout, b, h, tile, split_k, gn_in, **kw):
    out = torch.empty((b * h * h, cout), dtype=eng.tdt, device=DEV)
    runs = []
    for _ in range(2):
        out.fill_(float("nan"))
        r = eng.gemm(srcs, w, cout, b, h, h, tile=tile, split_k=split_k, out=out, gn_in=gn_in, **kw)
        torch.cuda.synchronize()
        assert r is not None, "the library declined the fused GroupNorm for this plan"
        runs.append(out.clone())
    return runs


# b, h, cin, cout, shape, split_k:
#   one chunk whose nine K-steps split 4 / 5 (a split starts inside the chunk, nk < 9, one partial per group, the tile is a whole image
#   with all four borders padded); a split that crosses a chunk boundary inside both chunks; 36 patch units over the twelve waves with 64
#   partials per group, padded top / bottom tiles and interior ones; an odd batch with three chunks and groups of 6 channels (one lane's
#   8 channels straddle groups)
@pytest.mark.parametrize("silu", [True, False])
@pytest.mark.parametrize("b,h,cin,cout,shape,split_k", [(2, 8, 64, 160, 6, 2), (2, 8, 128, 160, 6, 3), (1, 64, 64, 160, 8, 1), (3, 32, 192, 128, 7, 1)])
def test_fused_prologue_bit_identical_and_repeatable(eng, b, h, cin, cout, shape, split_k, silu):
    hw, tile = h * h, 100 + shape
    x = _rand((b, h, h, cin), 301, 1.5).to(eng.tdt)
    w = eng.tile_weight(eng._pack_conv(_rand((cout, cin, 3, 3), 302, (9 * cin) ** -0.5)))
    bias = _rand((cout,), 303)
    gamma, beta = 1.0 + 0.3 * _rand((cin,), 304), 0.2 * _rand((cin,), 305)
    # partials in the producer's layout (one per 64-row chunk and group), fed to both paths
    xf = x.float().reshape(b, hw // 64, 64, G, cin // G)
    part = torch.stack([xf.sum(dim=(2, 4)), (xf * xf).sum(dim=(2, 4))], dim=-1).contiguous()
    chunks = hw // 64
    xn = _groupnorm(eng, [x], [cin], b, hw, gamma, beta, silu, part, chunks)
    ref = eng.gemm([(xn, cin, 9, h, h, 0)], w, cout, b, h, h, tile=tile, split_k=split_k, bias=bias)
    torch.cuda.synchronize()
    ref = ref.clone()
    first, second = _fused_twice(eng, [(x, cin, 9, h, h, 0)], w, cout, b, h, tile, split_k, (part, chunks, G, 1e-5, gamma, beta, silu, 1), bias=bias)
    assert torch.isfinite(first.float()).all()
    assert torch.equal(first, second)
    assert torch.equal(first, ref)


@pytest.mark.parametrize("silu", [True, False])
def test_fused_prologue_two_normalised_segments(eng, silu):
    """cat[x, skip] as two normalised 3x3 K segments (the segment switch in the first patch's addressing).  The fused kernel takes
    idb_groupnorm_stats' partials, the reference idb_groupnorm's own first pass — the same sums in a different order — so the comparison
    with the reference has the tolerance of the existing concatenation test; the two fused runs must still be equal."""
    b, h, ca, cb, cout, tile = 2, 16, 128, 64, 192, 106
    xa, xb = _rand((b, h, h, ca), 311).to(eng.tdt), _rand((b, h, h, cb), 312, 2.0).to(eng.tdt)
    wc = _rand((cout, ca + cb, 3, 3), 313, (9 * (ca + cb)) ** -0.5)
    w_ref = eng.tile_weight(eng._pack_conv(wc))
    w_split = eng.tile_weight(torch.cat([eng._pack_conv(wc[:, :ca].contiguous()), eng._pack_conv(wc[:, ca:].contiguous())], dim=1).contiguous())
    bias = _rand((cout,), 314)
    gamma, beta = 1.0 + 0.3 * _rand((ca + cb,), 315), 0.2 * _rand((ca + cb,), 316)
    part, chunks = eng.gn_statistics(xa, ca, xb, cb, b, h * h, G)
    xn = _groupnorm(eng, [xa, xb], [ca, cb], b, h * h, gamma, beta, silu, None, 0)
    ref = eng.gemm([(xn, ca + cb, 9, h, h, 0)], w_ref, cout, b, h, h, tile=tile, bias=bias)
    torch.cuda.synchronize()
    ref = ref.clone()
    first, second = _fused_twice(eng, [(xa, ca, 9, h, h, 0), (xb, cb, 9, h, h, 0)], w_split, cout, b, h, tile, 0,
                                 (part, chunks, G, 1e-5, gamma, beta, silu, 2), bias=bias)
    assert torch.equal(first, second)
    tol = 2.0 ** -7 if eng.dtype_name == "bf16" else 2.0 ** -9
    assert (first.float() - ref.float()).abs().max().item() <= tol * max(1.0, ref.float().abs().max().item())
    assert (first != ref).float().mean().item() < 0.02
