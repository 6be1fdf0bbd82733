"""idb_cfg_plms_step per element against float64, and the whole PLMS sampler (PNDMScheduler through StableDiffusionPipeline and
HipEngine, eager and HIP-graph) against tests/pndm_oracle.py over the fp32 oracle UNet; class-image generation end to end."""
import dataclasses
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pndm_oracle as P  # noqa: E402

from faceposegenerator_amd import _lib as L  # noqa: E402
from faceposegenerator_amd import spec as S  # noqa: E402
from faceposegenerator_amd import weights as W  # noqa: E402
from faceposegenerator_amd.engine import plms_slots  # noqa: E402
from faceposegenerator_amd.scheduler import PNDMScheduler  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24                                        # fp32 unit roundoff
LOOP_INDICES = (0, 1, 2, 3, 5)                        # 1 term + save, the restore form, 2, 3 and 4 terms (ring wrapped: write slot 0)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ---- the step kernel ------------------------------------------------------------------------------------------------------------
def _step_case(lib, B, rep, h, w, vpred, i, aligned, seed):
    """One call at loop index i (structure from plms_slots, scalars from PNDMScheduler at 8 steps), every history slot that holds
    no prediction yet and the saved-sample buffer (unless it is read) poisoned with NaN.  Returns the largest error / bound ratio."""
    C, hw = 4, h * w
    g = torch.Generator().manual_seed(seed)
    sch = PNDMScheduler(S.SchedulerConfig(prediction_type="v_prediction" if vpred else "epsilon"))
    sch.set_timesteps(8)
    coef = torch.tensor(list(sch.step_coefficients(i)) + [7.5], dtype=torch.float32)
    write, terms, slots, mode = plms_slots(i)
    eps = torch.randn(rep * B, hw, C, generator=g)
    lat = 3.0 * torch.randn(B, C, h, w, generator=g)
    hist = torch.randn(L.IDB_PLMS_SLOTS, B, C, h, w, generator=g)
    saved = torch.randn(B, C, h, w, generator=g)
    valid = {0: (), 1: (0,), 2: (0,), 3: (0, 1), 5: (0, 1, 2, 3)}[i]
    for s in range(L.IDB_PLMS_SLOTS):
        if s not in valid:
            hist[s] = float("nan")
    if mode != L.IDB_PLMS_RESTORE:
        saved[:] = float("nan")
    # float64 reference on the very fp32 inputs and coefficients
    w4, (sa, sb, c_sample, c_eps, gs) = coef[:4].double(), coef[4:].double()
    e_u = eps[:B].double().reshape(B, h, w, C).permute(0, 3, 1, 2)
    if rep == 2:
        e_c = eps[B:].double().reshape(B, h, w, C).permute(0, 3, 1, 2)
        e, e_mag = e_u + gs * (e_c - e_u), e_u.abs() + gs.abs() * (e_c.abs() + e_u.abs())
    else:
        e, e_mag = e_u, e_u.abs()
    x = (saved if mode == L.IDB_PLMS_RESTORE else lat).double()
    m, M = w4[0] * e, w4[0].abs() * e_mag
    for j in range(terms - 1):
        m = m + w4[j + 1] * hist[slots[j]].double()
        M = M + w4[j + 1].abs() * hist[slots[j]].double().abs()
    if vpred:
        m, M = sa * m + sb * x, sa * M + sb * x.abs()
    want = c_sample * x - c_eps * m
    bound = 16 * U * (c_sample.abs() * x.abs() + c_eps.abs() * M)
    assert torch.isfinite(want).all()
    # device buffers; a misaligned eps (one float into its allocation) takes the per-element kernel instead of the float4 one
    eps_buf = torch.empty(eps.numel() + 4, dtype=torch.float32, device=DEV)
    eps_d = eps_buf[(0 if aligned else 1):][:eps.numel()].view(eps.shape)
    eps_d.copy_(eps)
    assert (eps_d.data_ptr() % 16 == 0) == aligned
    lat_d, hist_d, saved_d, coef_d = lat.to(DEV), hist.to(DEV), saved.to(DEV), coef.to(DEV)
    L.check(lib.idb_cfg_plms_step(eps_d.data_ptr(), lat_d.data_ptr(), hist_d.data_ptr(), saved_d.data_ptr(), coef_d.data_ptr(), B, C, hw,
                                  rep, int(vpred), write, terms, *slots, mode, _stream()), "idb_cfg_plms_step")
    torch.cuda.synchronize()
    got, hist_o, saved_o = lat_d.cpu(), hist_d.cpu(), saved_d.cpu()
    assert torch.isfinite(got).all(), "a poisoned buffer was read"
    ratio = ((got.double() - want).abs() / bound).max().item()
    assert ratio <= 1.0, (i, ratio)
    for s in range(L.IDB_PLMS_SLOTS):
        if s == write:
            assert ((hist_o[s].double() - e).abs() <= 4 * U * e_mag).all()
        else:
            assert torch.equal(_bits(hist_o[s]), _bits(hist[s])), f"slot {s} was written at loop index {i}"
    if mode == L.IDB_PLMS_SAVE:
        assert torch.equal(_bits(saved_o), _bits(lat))
    else:
        assert torch.equal(_bits(saved_o), _bits(saved))
    assert torch.equal(_bits(eps_d.cpu()), _bits(eps)) and torch.equal(_bits(coef_d.cpu()), _bits(coef))
    return ratio


@pytest.mark.parametrize("vpred", [False, True], ids=["epsilon", "v_prediction"])
@pytest.mark.parametrize("h,w", [(5, 7), (16, 16)])
@pytest.mark.parametrize("rep", [1, 2])
@pytest.mark.parametrize("B", [1, 3])
def test_step_kernel_per_element(lib, B, rep, h, w, vpred):
    """Bound per element: 16 * 2^-24 * (|c_sample| |x| + |c_eps| M), M = sum_j |w_j| |term_j| with |e_u| + |g| (|e_c| + |e_u|) for
    the current term, sqrt(abar) M + sqrt(1-abar) |x| in its place for v-prediction: at most 12 fp32 roundings on quantities bounded
    by that sum (derived, not measured).  B = 3 at 16x16 is 768 pixels = more than one block; 5x7 is an odd pixel count."""
    worst = 0.0
    for i in LOOP_INDICES:
        for aligned in (True, False):
            worst = max(worst, _step_case(lib, B, rep, h, w, vpred, i, aligned, seed=100 * i + B))
    print(f"idb_cfg_plms_step B={B} rep={rep} {h}x{w} vpred={vpred}: worst error / bound {worst:.3f}")


def test_step_kernel_rejects_bad_arguments(lib):
    B, C, hw = 1, 4, 16
    eps, lat = torch.zeros(2 * B, hw, C, device=DEV), torch.ones(B, C, 4, 4, device=DEV)
    hist, saved, coef = torch.zeros(4, B, C, 4, 4, device=DEV), torch.zeros(B, C, 4, 4, device=DEV), torch.ones(9, device=DEV)

    def call(rep=2, write=0, terms=1, s1=1, s2=2, s3=3, mode=0):
        return lib.idb_cfg_plms_step(eps.data_ptr(), lat.data_ptr(), hist.data_ptr(), saved.data_ptr(), coef.data_ptr(), B, C, hw, rep, 0,
                                     write, terms, s1, s2, s3, mode, _stream())

    for kw in ({"rep": 0}, {"rep": 3}, {"terms": 0}, {"terms": 5}, {"write": 4}, {"write": -2}, {"terms": 2, "s1": 4},
               {"terms": 4, "s3": -1}, {"terms": 3, "s2": 0}, {"mode": 3}):
        assert call(**kw) < 0 and lib.idb_last_error(), kw
    torch.cuda.synchronize()
    assert torch.equal(lat.cpu(), torch.ones(B, C, 4, 4)) and not hist.any() and not saved.any()      # nothing was launched
    assert call(terms=1, s1=9, s2=9, s3=9) == 0                                                      # slots past n_terms are not looked at
    torch.cuda.synchronize()


# ---- the whole sampler ------------------------------------------------------------------------------------------------------------
STEPS, GS = 6, 5.0                                    # 7 UNet calls: every branch of the step
# max-abs / rel-RMS of the final latents (std 7.0) against the float64 PLMS over the fp32 oracle UNet (B = 2, 16x16 latents, 6 steps,
# CFG 5.0); bounds = 1.5 x the largest value measured on an MI355X over the eager run, the capturing run and the replay with other
# inputs (eager, capture and replay of the same inputs agree to every printed digit):
#   f16   measured max-abs 6.28e-2 (other inputs 6.29e-2), rel-RMS 2.25e-3 (2.22e-3)
#   bf16  measured max-abs 5.62e-1 (other inputs 4.40e-1), rel-RMS 1.85e-2 (1.75e-2)
# free-running error: amplified by CFG and by c_sample up to 1.95 per step, so far above one UNet forward's error
TOL = {"f16": (9.4e-2, 3.4e-3), "bf16": (8.4e-1, 2.8e-2)}
TOL_NO_CFG = (2.0e-2, 7.5e-4)                         # guidance_scale = 1.0 (rep = 1), f16: measured 1.36e-2 / 4.98e-4 (latents std 6.4)


@pytest.fixture(scope="module")
def tiny():
    return S.TINY_UNET, W.synth_unet(S.TINY_UNET, 7), W.synth_vae(S.TINY_VAE, 8)


def _inputs(seed):
    g = torch.Generator().manual_seed(seed)                                  # a 1-D fp32 draw in the order pe, ne, init
    cd = S.TINY_UNET.cross_attention_dim
    return torch.randn(2, 77, cd, generator=g), torch.randn(2, 77, cd, generator=g), torch.randn(2, 4, 16, 16, generator=g)


@pytest.fixture(scope="module")
def refs(tiny):
    """Computed once, shared, never modified: the float64 PLMS trajectory ends for two input sets, the order-1 control and the
    run without guidance."""
    ucfg, usd, _ = tiny
    a, b = _inputs(13), _inputs(17)
    return {"a": P.plms_unet_sample(usd, ucfg, a[0], a[1], a[2], STEPS, GS),
            "b": P.plms_unet_sample(usd, ucfg, b[0], b[1], b[2], STEPS, GS),
            "a_order1": P.plms_unet_sample(usd, ucfg, a[0], a[1], a[2], STEPS, GS, order=1),
            "a_no_cfg": P.plms_unet_sample(usd, ucfg, a[0], None, a[2], STEPS, 1.0)}


def _stats(got, ref):
    d = (got.double().cpu() - ref).abs()
    return d.max().item(), (d.pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()).item()


def _pipe(tiny, dtype, ucfg=None):
    from faceposegenerator_amd.pipeline import StableDiffusionPipeline
    base, usd, vsd = tiny
    pipe = StableDiffusionPipeline(ucfg or base, S.TINY_VAE, usd, vsd, torch_dtype=dtype).to(DEV)
    pipe.scheduler = PNDMScheduler.from_config(pipe.scheduler.config)
    return pipe


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_plms_sampler_matches_oracle(lib, tiny, refs, dtype):
    """One eager run, then the capturing run and one replay of the HIP graph, the replay with other initial latents and embeddings
    (the history and the saved sample live in the graph entry and are rebuilt by every replay)."""
    pipe = _pipe(tiny, dtype)
    a, b = _inputs(13), _inputs(17)
    mx_tol, rel_tol = TOL[dtype]
    order1 = (refs["a"] - refs["a_order1"]).abs().max().item()
    print(f"PLMS vs its order-1 control: max-abs {order1:.3f}; ratio to the {dtype} max-abs bound {order1 / mx_tol:.1f}")
    assert order1 > 2 * mx_tol                       # 3.16 on these inputs: 34 x the f16 bound, 3.8 x the bf16 one
    for name, use_graph, (pe, ne, init), ref in (("eager", False, a, refs["a"]), ("capture", True, a, refs["a"]),
                                                 ("replay", True, b, refs["b"])):
        pipe.use_graph = use_graph
        out = pipe(prompt_embeds=pe, negative_prompt_embeds=ne, num_inference_steps=STEPS, guidance_scale=GS, height=128, width=128,
                   output_type="latent", latents=init).images
        mx, rel = _stats(out, ref)
        print(f"[{dtype}] PLMS sampler {name}: latents max-abs {mx:.3e} rel-rms {rel:.3e}")
        assert mx < mx_tol and rel < rel_tol, (name, mx, rel)
    ent = [v for k, v in pipe._engine()._graphs.items() if k[-2] == "plms"]
    assert len(ent) == 1 and ent[0]["hist"].shape == (L.IDB_PLMS_SLOTS + 1, 2, 4, 16, 16)


def test_plms_without_guidance_and_output_types(lib, tiny, refs):
    pipe = _pipe(tiny, "f16")
    pe, ne, init = _inputs(13)
    out = pipe(prompt_embeds=pe, num_inference_steps=STEPS, guidance_scale=1.0, height=128, width=128, output_type="latent",
               latents=init).images
    mx, rel = _stats(out, refs["a_no_cfg"])
    print(f"[f16] PLMS sampler without guidance (rep 1): latents max-abs {mx:.3e} rel-rms {rel:.3e}")
    assert mx < TOL_NO_CFG[0] and rel < TOL_NO_CFG[1]
    gen = lambda: torch.Generator().manual_seed(3)
    kw = dict(prompt_embeds=pe, negative_prompt_embeds=ne, num_inference_steps=STEPS, guidance_scale=GS, height=128, width=64)
    pil = pipe(generator=gen(), output_type="pil", **kw).images
    assert len(pil) == 2 and all(im.size == (64, 128) and im.mode == "RGB" for im in pil)
    lat = pipe(generator=gen(), output_type="latent", **kw).images
    assert lat.shape == (2, 4, 16, 8) and torch.isfinite(lat).all()
    assert torch.equal(lat, pipe(generator=gen(), output_type="latent", **kw).images)               # deterministic: no per-step noise
    init2 = pipe.prepare_noise(2, 0, 128, 64, gen())[0]                                              # the generator's only draw
    assert torch.equal(lat, pipe(latents=init2, output_type="latent", **kw).images)
    npy = pipe(generator=gen(), output_type="np", **kw).images
    assert npy.shape == (2, 128, 64, 3) and 0.0 <= npy.min() and npy.max() <= 1.0
    assert pipe(generator=gen(), output_type="pt", **kw).images.shape == (2, 3, 128, 64)
    assert pipe(generator=gen(), output_type="uint8", **kw).images.dtype == torch.uint8


def test_generate_class_images_end_to_end(lib, tiny, tmp_path):
    """The default call (PLMS, 50 steps = 51 UNet calls, guidance 7.5, empty negative prompt) on the reduced-width graph with a
    16x16 sample size and synthetic prompt embeddings: 3 JPEGs of 128x128 in batches of 2 + 1; a second call writes nothing."""
    from PIL import Image
    from faceposegenerator_amd.driver import generate_class_images, synthetic_embed_fn
    pipe = _pipe(tiny, "f16", dataclasses.replace(S.TINY_UNET, sample_size=16))
    embed = synthetic_embed_fn(S.TINY_UNET.cross_attention_dim)
    seen = []

    def encode(prompt, negative_prompt, do_cfg):
        prompts = [prompt] if isinstance(prompt, str) else list(prompt)
        seen.append((prompts, negative_prompt, do_cfg))
        return embed(prompts), embed([negative_prompt or ""] * len(prompts)) if do_cfg else None

    pipe.encode_prompt_fn = encode
    pipe.use_graph = False                           # two batch sizes would capture two 51-step graphs; the graph path is tested above
    d = str(tmp_path / "class_images")
    paths = generate_class_images(pipe, "photo of a person", d, 3, sample_batch_size=2, generator=torch.Generator().manual_seed(0))
    assert len(paths) == 3 and sorted(os.listdir(d)) == sorted(os.path.basename(p) for p in paths)
    assert [os.path.basename(p).split("-")[0] for p in paths] == ["0", "1", "2"]
    assert seen == [(["photo of a person"] * 2, None, True), (["photo of a person"], None, True)]
    assert len(pipe.scheduler.timesteps) == 51
    for p in paths:
        with Image.open(p) as im:
            assert im.format == "JPEG" and im.size == (128, 128)
    assert generate_class_images(pipe, "photo of a person", d, 3, sample_batch_size=2) == [] and len(seen) == 2
    assert len(os.listdir(d)) == 3
