"""ArcFace IResNet on the MI355X: the idb_gemm pieces (PReLU epilogue on every plan, the strided 1x1 second K segment, the affine second
output), one IBasicBlock at 7x7 with large bn1 shifts (border vs interior), the full r100 / r50 against the fp32 restatement of
tests/arcface_oracle.py with per-stage teacher forcing, the uint8 entry, determinism, and the detect -> align -> embed path.

Tolerances were set on CPU from the emulated-autocast restatement before any GPU run (r100, synthetic weights, 2 faces): f16 cosine
0.999999 / relative L2 1.3e-3, bf16 cosine 0.99995 / relative L2 1.0e-2.  Bounds are about 3-4x those: f16 cosine >= 0.9995, relative
L2 <= 5e-3; bf16 cosine >= 0.995, relative L2 <= 4e-2."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import arcface_oracle as O  # noqa: E402

from faceposegenerator_amd import _lib as L  # noqa: E402
from faceposegenerator_amd import arcface as A  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BOUNDS = {torch.float16: (0.9995, 5e-3, 1e-2), torch.bfloat16: (0.995, 4e-2, 6e-2)}      # cosine, relative L2, per-stage relative L2


def _rel(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm()).item()


# ---- idb_gemm pieces --------------------------------------------------------------------------------------------------------------
def _conv_case(dtype, B=2, H=14, cin=128, n=128, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, H, H, cin, generator=g).to(dtype)
    w = (torch.randn(n, cin, 3, 3, generator=g) / (9 * cin) ** 0.5)
    b = 0.1 * torch.randn(n, generator=g)
    slope = 0.05 + 0.35 * torch.rand(n, generator=g)
    return x, w, b, slope


def _run(m, srcs, w, n, B, oh, ow, b, **kw):
    return m.gemm([(s.to(DEV).contiguous(), *rest) for s, *rest in srcs], w.to(DEV, m.tdt).contiguous(), n, B, oh, ow, b.to(DEV), **kw)


@pytest.fixture(scope="module", params=[torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def eng(request, lib):
    return A.ArcFace.from_synthetic("r18", 0, request.param).to(DEV)


def _plans(lib, dt):
    """One forced tile id per kernel family that plans the PReLU case (every family but the persistent / 256-row patch ones)."""
    d = L.GemmDesc()
    d.dtype, d.batch, d.out_h, d.out_w, d.stride, d.n, d.nsrc = dt, 2, 14, 14, 1, 128, 1
    d.src[0].ptr, d.src[0].channels, d.src[0].taps, d.src[0].in_h, d.src[0].in_w = 0x1000, 128, 9, 14, 14
    d.w, d.out, d.out_dtype, d.out_ld, d.act, d.act_slope = 0x2000, 0x3000, dt, 128, 2, 0x4000
    fams = {}
    for t in range(1, 110):
        d.tile = t
        if lib.idb_gemm_plan(C.byref(d), None, None, None) == 0:
            fams.setdefault(t // 10, t)
    return sorted(fams.values())


def test_prelu_epilogue_on_every_plan(eng, lib):
    x, w, b, slope = _conv_case(eng.tdt)
    ref = F.prelu(F.conv2d(x.float().permute(0, 3, 1, 2), w.to(eng.tdt).float(), b, 1, 1), slope).permute(0, 2, 3, 1)
    tiles = _plans(lib, eng.dt)
    assert len(tiles) >= 5, tiles
    cases = [dict(), dict(split_k=4)] + [dict(tile=t) for t in tiles]
    for kw in cases:
        out, _ = _run(eng, [(x, 128, 9, 14, 14)], A._pack(w), 128, 2, 14, 14, b,
                      slope=slope.to(DEV), **kw)
        err = (out.float().cpu() - ref).abs().max().item()
        assert err <= 2e-2 * ref.abs().max().item(), (kw, err)


def test_two_segment_stride2_gemm(eng):
    """conv3x3 stride 2 (+ its bias) and a 1x1 stride-2 shortcut as ONE GEMM with two K segments: the sum of the two F.conv2d."""
    g = torch.Generator().manual_seed(3)
    B, H, c1, c0, n = 2, 14, 128, 64, 128
    h = torch.randn(B, H, H, c1, generator=g).to(eng.tdt)
    x = torch.randn(B, H, H, c0, generator=g).to(eng.tdt)
    w3 = torch.randn(n, c1, 3, 3, generator=g) / (9 * c1) ** 0.5
    w1 = torch.randn(n, c0, 1, 1, generator=g) / c0 ** 0.5
    b = 0.1 * torch.randn(n, generator=g)
    wk = torch.cat([A._pack(w3), A._pack(w1)], dim=1)
    out, _ = _run(eng, [(h, c1, 9, H, H), (x, c0, 1, H, H)], wk, n, B, 7, 7, b, stride=2)
    ref = (F.conv2d(h.float().permute(0, 3, 1, 2), w3.to(eng.tdt).float(), b, 2, 1) +
           F.conv2d(x.float().permute(0, 3, 1, 2), w1.to(eng.tdt).float(), None, 2, 0)).permute(0, 2, 3, 1)
    assert (out.float().cpu() - ref).abs().max().item() <= 2e-2 * ref.abs().max().item()


@pytest.mark.parametrize("kw", [dict(), dict(split_k=3)])
def test_out2_is_bit_equal_to_the_affine_of_the_rounded_output(eng, kw):
    x, w, b, _ = _conv_case(eng.tdt, seed=5)
    g = torch.Generator().manual_seed(6)
    sc, sh = (0.5 + torch.rand(128, generator=g)), torch.randn(128, generator=g)
    res = torch.randn(2, 14, 14, 128, generator=g).to(eng.tdt).to(DEV)
    out, out2 = _run(eng, [(x, 128, 9, 14, 14)], A._pack(w), 128, 2, 14, 14, b, residual=res, out2=(sc.to(DEV), sh.to(DEV)), **kw)
    o = out.cpu().double()
    want = (o * sc.double() + sh.double()).float().to(eng.tdt)          # fma(x, s, b) in fp32, one rounding to the operand dtype
    assert torch.equal(out2.cpu().view(torch.int16), want.view(torch.int16))


def test_basic_block_border_meets_the_interior_bound(eng):
    """layer4.1 of r18 (7x7, 24 of 49 positions on the border) with the fixture's large bn1 shifts, input from the previous block."""
    sd = eng._sd
    g = torch.Generator().manual_seed(8)
    x = (torch.randn(4, 512, 7, 7, generator=g)).to(eng.tdt)
    k = "layer4.1"
    a, s = A._affine(sd, f"{k}.bn1")
    xn = x.permute(0, 2, 3, 1).contiguous()
    xb = (xn.double() * a + s).float().to(eng.tdt)
    out, _ = eng.block(3, 1, xn.to(DEV), xb.to(DEV))
    ref = O.block(sd, k, x.float(), 1)
    got = out.float().cpu().permute(0, 3, 1, 2)
    ring = torch.ones(7, 7, dtype=torch.bool)
    ring[1:-1, 1:-1] = False
    e_ring, e_in = _rel(got[..., ring], ref[..., ring]), _rel(got[..., ~ring], ref[..., ~ring])
    bound = BOUNDS[eng.tdt][2]
    assert e_ring <= bound and e_in <= bound, (e_ring, e_in)


# ---- the whole network ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def r100_sd():
    return A.synth_weights("r100", 0)


def _faces(B, seed=1):
    return torch.rand(B, 3, 112, 112, generator=torch.Generator().manual_seed(seed)) * 2 - 1


def _check_embeddings(got, ref, dt):
    cmin, rel_max, _ = BOUNDS[dt]
    cos = F.cosine_similarity(got.float(), ref, dim=1)
    rel = (got.float() - ref).norm(dim=1) / ref.norm(dim=1)
    assert torch.isfinite(got).all()
    assert cos.min().item() >= cmin and rel.max().item() <= rel_max, (cos.min().item(), rel.max().item())
    return cos.min().item(), rel.max().item()


@pytest.mark.parametrize("B,dt", [(1, torch.float16), (5, torch.float16), (64, torch.float16), (5, torch.bfloat16)])
def test_r100_matches_the_restatement(r100_sd, B, dt):
    m = A.ArcFace.from_state_dict(r100_sd, "r100", dt).to(DEV)
    x = _faces(B)
    got = m(x).cpu()
    assert got.shape == (B, 512) and got.dtype == torch.float32
    idx = torch.arange(B) if B <= 8 else torch.randperm(B, generator=torch.Generator().manual_seed(0))[:8].sort().values
    ref = O.forward(r100_sd, "r100", x[idx])
    c, r = _check_embeddings(got[idx], ref, dt)
    print(f"r100 B={B} {dt}: min cosine {c:.7f}, max relative L2 {r:.3e}")


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
def test_r100_per_stage_teacher_forced(r100_sd, dt):
    """Each stage run by the restatement from the HIP input of that stage, compared with the HIP output of the stage."""
    m = A.ArcFace.from_state_dict(r100_sd, "r100", dt).to(DEV)
    x = _faces(2, seed=4)
    h, hb = m.stem(x.to(DEV).contiguous(), False)
    ref0 = O.stem(r100_sd, x)
    errs = [_rel(h.cpu().permute(0, 3, 1, 2), ref0)]
    for i in range(4):
        inp = h.float().cpu().permute(0, 3, 1, 2)
        h, hb = m.stage(i, h, hb)
        errs.append(_rel(h.cpu().permute(0, 3, 1, 2), O.stage(r100_sd, "r100", i, inp)))
    hin = h.float().cpu().permute(0, 3, 1, 2)
    errs.append(_rel(m.head(h).cpu(), O.head(r100_sd, hin)))
    print(f"r100 {dt} per-stage relative L2 (stem, layer1-4, head): {['%.2e' % e for e in errs]}")
    assert max(errs) <= BOUNDS[dt][2], errs


def test_embed_u8_equals_call_on_host_preprocessed_input(r100_sd):
    m = A.ArcFace.from_state_dict(r100_sd, "r100", torch.float16).to(DEV)
    crops = torch.randint(0, 256, (3, 112, 112, 3), generator=torch.Generator().manual_seed(2), dtype=torch.uint8)
    x = ((crops.float() / 255 - 0.5) / 0.5).permute(0, 3, 1, 2).contiguous()
    assert torch.equal(m.embed_u8(crops), m(x))
    with pytest.raises(ValueError):
        m(torch.zeros(1, 3, 96, 96))
    with pytest.raises(ValueError):
        m.embed_u8(torch.zeros(1, 112, 112, 3))


def test_two_calls_are_bit_identical(r100_sd):
    m = A.ArcFace.from_state_dict(r100_sd, "r100", torch.float16).to(DEV)
    x = _faces(7, seed=9)
    assert torch.equal(m(x), m(x))


def test_chunked_batch_matches_unchunked(r100_sd):
    m = A.ArcFace.from_state_dict(r100_sd, "r100", torch.float16).to(DEV)
    x = _faces(5, seed=10)
    full = m(x)
    m.chunk = 2
    # chunks of 2 / 1 faces plan other tiles and split-K factors than 5 faces (M differs): same values, not the same summation order
    part = m(x)
    assert part.shape == full.shape
    assert ((part - full).norm(dim=1) / full.norm(dim=1)).max().item() < 2e-3


def test_r50_runs_one_batch():
    sd = A.synth_weights("r50", 1)
    m = A.ArcFace.from_state_dict(sd, "r50", torch.float16).to(DEV)
    x = _faces(4, seed=11)
    _check_embeddings(m(x).cpu(), O.forward(sd, "r50", x), torch.float16)


def test_detect_align_embed_end_to_end(lib):
    """Tiny-config sampler images -> synthetic MTCNN -> norm_crop -> embed_faces: finite [B,512], has_face as detect() says."""
    from faceposegenerator_amd import face_align as FA
    from faceposegenerator_amd import mtcnn as M
    from faceposegenerator_amd import spec as S
    from faceposegenerator_amd.pipeline import StableDiffusionPipeline
    from oracle import sd21_oracle as SO
    pipe = StableDiffusionPipeline.from_synthetic(S.TINY_UNET, S.TINY_VAE, seed=7, torch_dtype=torch.float16).to(DEV)
    g = torch.Generator().manual_seed(11)
    pe = torch.randn(2, 77, S.TINY_UNET.cross_attention_dim, generator=g)
    ne = torch.randn(2, 77, S.TINY_UNET.cross_attention_dim, generator=g)
    noise = SO.draw_noise(torch.Generator().manual_seed(5), 2, 2, (16, 16))
    lat = pipe(prompt_embeds=pe, negative_prompt_embeds=ne, num_inference_steps=2, guidance_scale=5.0, height=128, width=128,
               output_type="latent", noise=noise).images
    _, u8 = pipe._engine().decode_images(lat.to(DEV))
    imgs = torch.cat([u8.cpu(), torch.zeros(1, *u8.shape[1:], dtype=torch.uint8)])     # + a blank image
    det = M.MTCNN(select_largest=True, post_process=False, device=DEV, weights=M.synth_weights(5))
    arc = A.ArcFace.from_synthetic("r18", 0).to(DEV)
    emb, has = A.embed_faces(imgs, det, arc)
    _, _, lms = det.detect(imgs, landmarks=True)
    assert emb.shape == (imgs.shape[0], 512) and torch.isfinite(emb).all()
    assert has.tolist() == [lm is not None for lm in lms]
    assert (emb[~has.to(DEV)] == 0).all()
    for b in np.nonzero(has.numpy())[0]:
        crop = FA.norm_crop(imgs[b:b + 1].to(DEV), lms[b][0][None])
        assert torch.equal(emb[b:b + 1], arc.embed_u8(crop))
