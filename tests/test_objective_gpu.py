"""GPU tests of the training objective's forward pass: the kernels of csrc/idb_objective.hip and idb_crop_resize_area_f32 against
the float64 oracle (tests/objective_oracle.py, itself checked against torch in test_objective_cpu.py), MTCNN.detect on a float
image against oracle/mtcnn_oracle.py, and TrainingObjective.step_losses / validation_losses end to end on the tiny UNet / VAE with
a synthetic ArcFace r18 — teacher-forced (the GPU's own network outputs fed into the oracle's arithmetic) and free-running against
the whole CPU fp32 composition.

The end-to-end images are 128 x 128 (16 x 16 latents), the resolution the tiny configuration is run at everywhere else (smoke(),
tests/test_golden_gpu.py): its UNet reaches 2 x 2 at the lowest level and the CPU oracle of a batch of four takes about a second."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import arcface_oracle as AO  # noqa: E402
import detect_matrix as D  # noqa: E402
import objective_oracle as R  # noqa: E402

from faceposegenerator_amd import _lib as L  # noqa: E402
from faceposegenerator_amd import objective as OB  # noqa: E402
from faceposegenerator_amd import spec as S  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TS = (0, 500, 999)


def _ac():
    from faceposegenerator_amd.scheduler import DDPMScheduler
    return DDPMScheduler().alphas_cumprod.float()


# ---- idb_diffuse_targets, idb_objective_mse_x0 ----------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[(3, 4, 8, 10), (2, 4, 64, 64)], ids=["3x4x8x10", "2x4x64x64"])
def latents(request, lib):
    shape = request.param
    g = torch.Generator().manual_seed(sum(shape))
    x0, noise, pred = (torch.randn(shape, generator=g) for _ in range(3))
    ts = torch.tensor([TS[(b + shape[0]) % 3] for b in range(shape[0])], dtype=torch.int32)     # 3 samples: all of TS; 2: 999 and 0
    return dict(shape=shape, x0=x0, noise=noise, pred=pred, ts=ts, ac=_ac())


@pytest.mark.parametrize("vp", [False, True], ids=["epsilon", "v_prediction"])
def test_diffuse_targets_and_x0_pred(latents, vp):
    """rtol 2e-6, atol 1e-6 against float64: the bound test_vae_sample_kernel uses for fp32 elementwise arithmetic."""
    d = latents
    B, C, h, w = d["shape"]
    ac, ts = d["ac"].to(DEV), d["ts"].to(DEV)
    noisy, target = OB.diffuse_targets(d["x0"].to(DEV), d["noise"].to(DEV), ts, ac, vp)
    n_ref, t_ref = R.diffuse_targets(d["x0"], d["noise"], d["ts"], d["ac"], vp)
    assert torch.allclose(noisy.cpu().double(), n_ref, rtol=2e-6, atol=1e-6) and torch.allclose(target.cpu().double(), t_ref, rtol=2e-6, atol=1e-6)
    if not vp:
        assert torch.equal(target.cpu(), d["noise"])
    ref = R.pred_original_sample(d["pred"], noisy.cpu(), d["ts"], d["ac"], vp)
    for nhwc in (False, True):
        pred = d["pred"].permute(0, 2, 3, 1).reshape(B * h * w, C).contiguous() if nhwc else d["pred"]
        _, x0p = OB.mse_x0(pred.to(DEV), target, noisy, ts, ac, vp, pred_nhwc=nhwc)
        err = (x0p.cpu().double() - ref).abs()
        print(f"x0_pred {d['shape']} vp={vp} nhwc={nhwc}: max |err| {err.max():.3e} at |ref| max {ref.abs().max():.2f}")
        assert torch.allclose(x0p.cpu().double(), ref, rtol=2e-6, atol=1e-6)
    # a timestep outside [0, T) is clamped into the table
    bad = torch.tensor([-5, 2000, 1000][:B] + [0] * max(0, B - 3), dtype=torch.int32)
    got = OB.diffuse_targets(d["x0"].to(DEV), d["noise"].to(DEV), bad.to(DEV), ac, vp)[0]
    assert torch.allclose(got.cpu().double(), R.diffuse_targets(d["x0"], d["noise"], bad.clamp(0, 999), d["ac"], vp)[0], rtol=2e-6, atol=1e-6)


def test_sse_is_the_float64_sum_and_deterministic(latents):
    d = latents
    B, C, h, w = d["shape"]
    ac, ts = d["ac"].to(DEV), d["ts"].to(DEV)
    target = d["noise"].to(DEV)
    ref = R.sse(d["pred"], d["noise"])
    got = {}
    for nhwc in (False, True):
        pred = (d["pred"].permute(0, 2, 3, 1).reshape(B * h * w, C).contiguous() if nhwc else d["pred"]).to(DEV)
        a = OB.mse_x0(pred, target, None, ts, ac, False, pred_nhwc=nhwc, want_x0=False)[0].cpu()
        b = OB.mse_x0(pred, target, None, ts, ac, False, pred_nhwc=nhwc, want_x0=False)[0].cpu()
        rel = ((a - ref).abs() / ref).max().item()
        print(f"sse {d['shape']} nhwc={nhwc}: max relative error {rel:.3e}")
        assert a.dtype == torch.float64 and rel <= 1e-9
        assert torch.equal(a.view(torch.int64), b.view(torch.int64))                 # two calls agree bitwise
        got[nhwc] = a
    assert torch.equal(got[False].view(torch.int64), got[True].view(torch.int64))    # the order of the sum does not depend on the layout
    # with x0_pred requested the sums are the same
    c = OB.mse_x0(d["pred"].to(DEV), target, d["x0"].to(DEV), ts, ac, True)[0].cpu()
    assert torch.equal(c.view(torch.int64), got[False].view(torch.int64))


# ---- idb_crop_resize_bilinear_f32 -------------------------------------------------------------------------------------------------
BILINEAR_BOXES = {
    (37, 53): [(0, 5, 25, 10, 23),          # 20 x 13 -> 112: upscale
               (0, 0, 12, 0, 9), (1, 30, 37, 40, 53), (1, 0, 37, 0, 53),       # top-left, bottom-right corners, the whole image
               (0, 3, 30, 17, 18),          # one pixel wide
               (1, 20, 21, 4, 50),          # one pixel high
               (1, 36, 37, 52, 53)],        # a single pixel in the last row and column
    (300, 280): [(0, 0, 300, 0, 280),       # downscale of the whole image
                 (1, 150, 300, 0, 140), (0, 0, 113, 167, 280)],                # bottom-left, top-right
}


@pytest.mark.parametrize("hw", list(BILINEAR_BOXES), ids=lambda v: f"{v[0]}x{v[1]}")
def test_crop_resize_bilinear(lib, hw):
    """atol 2e-6 against float64 F.interpolate on the crop, then the normalisation: the weights are exact in double, four fp32
    roundings on values <= 255 (4 * 255 * 2^-24 = 6.1e-5) before the division by 127.5 (4.8e-7), and the normalisation's own
    roundings of values <= 1."""
    img = torch.rand(2, *hw, 3, generator=torch.Generator().manual_seed(hw[0])) * 255
    boxes = np.array(BILINEAR_BOXES[hw], dtype=np.int32)
    got = OB.crop_resize_bilinear(img.to(DEV), boxes).cpu().double()
    ref = R.crop_resize_bilinear(img, boxes)
    err = (got - ref).abs().flatten(1).max(1).values
    print(f"bilinear {hw}: max |err| per box {[f'{e:.2e}' for e in err.tolist()]}")
    assert got.shape == (len(boxes), 3, 112, 112) and err.max().item() <= 2e-6
    other = OB.crop_resize_bilinear(img.to(DEV), boxes[:2], 7, 200).cpu().double()       # oh != ow, no multiple of the block
    assert (other - R.crop_resize_bilinear(img, boxes[:2], 7, 200)).abs().max().item() <= 2e-6


# ---- idb_crop_resize_area_f32 -----------------------------------------------------------------------------------------------------
def _area(lib, img_d, boxes, oh, ow):
    b, h, w, c = img_d.shape
    n = boxes.shape[0]
    out = torch.full((max(n, 1), c, oh, ow), float("nan"), dtype=torch.float32, device=DEV)
    bx = torch.from_numpy(np.ascontiguousarray(boxes, dtype=np.int32).reshape(-1, 5)).to(DEV) if n else torch.zeros(5, dtype=torch.int32, device=DEV)
    fn = lib.idb_crop_resize_area_u8 if img_d.dtype == torch.uint8 else lib.idb_crop_resize_area_f32
    L.check(fn(img_d.data_ptr(), b, h, w, c, bx.data_ptr(), n, out.data_ptr(), oh, ow, D.SUB, D.MUL, torch.cuda.current_stream().cuda_stream))
    return out[:n].cpu()


def test_area_f32_equals_the_u8_kernel_bit_for_bit(lib):
    """Integer-valued floats in [0, 255], over every case (boxes, sizes, channel counts) of the detect-matrix test."""
    imgs = {k: torch.from_numpy(v) for k, v in D.area_images().items()}
    for case in D.area_cases():
        u8 = imgs[case.image]
        a = _area(lib, u8.to(DEV), case.boxes_np, case.oh, case.ow)
        b = _area(lib, u8.float().to(DEV), case.boxes_np, case.oh, case.ow)
        ok, where = D.bit_equal(b.numpy(), a.numpy())
        assert ok, (case.name, where)


@pytest.mark.parametrize("quarters", [True, False], ids=["quarter_values", "random_fractions"])
def test_area_f32_on_fractional_images(lib, quarters):
    """Against float64 F.interpolate(mode="area") at the detect-matrix criterion (u |q| + u |q - sub|) |mul| + u |out|.  That criterion
    presumes the window sum is exact in fp32 (area_sum_exact): true for multiples of 1/4 in [0, 255] (1020 * window pixels < 2^24), so
    those are held to it as it stands; for arbitrary fractions the fp32 sum of a k-pixel window adds gamma_k |q| |mul|."""
    rng = np.random.default_rng(11)
    for case in [c for c in D.area_cases() if c.image == "noise3" and c.boxes]:
        shape = D.area_images()[case.image].shape
        img = torch.from_numpy(rng.integers(0, 1021, size=shape) / 4.0 if quarters else rng.uniform(0, 255, size=shape)).float()
        assert (img != img.round()).any()
        got = _area(lib, img.to(DEV), case.boxes_np, case.oh, case.ow).double()
        ref, bound = R.crop_resize_area(img, case.boxes_np, case.oh, case.ow, exact_sums=quarters)
        assert D.area_window_pixels(case) * 1020 < 2 ** 24
        res = D.check(got.numpy(), ref.numpy(), bound.numpy())
        assert res[0], D.describe(case.name, res)


# ---- idb_identity_losses ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 512, 8192])
@pytest.mark.parametrize("n", [1, 5])
def test_identity_losses(lib, n, d):
    """Rows: random | zero anchor (the eps clamp) | positive identical to the anchor (cos = 1) | a triplet inside the margin (negative
    = positive: the loss is exactly the margin) | a triplet outside it (positive = anchor, negative = -anchor: hinge at 0).  Bound:
    2 fp32 ulp of the float64 value (objective_oracle.loss_bound)."""
    g = torch.Generator().manual_seed(100 * n + d)
    a, p, q = (torch.randn(n, d, generator=g) for _ in range(3))
    if n == 5:
        a[1] = 0.0
        p[2] = a[2]
        q[3] = p[3]
        p[4], q[4] = a[4], -a[4]
    cos, ident, trip = (t.cpu().double().numpy() for t in OB.identity_losses(a.to(DEV), p.to(DEV), q.to(DEV)))
    c_ref, i_ref, t_ref = (t.numpy() for t in R.identity_losses(a, p, q))
    for name, got, ref in (("cos", cos, c_ref), ("identity", ident, i_ref), ("triplet", trip, t_ref)):
        res = D.check(got, ref, R.loss_bound(ref))
        assert res[0], D.describe(f"{name} n={n} d={d}", res)
    if n == 5:
        assert cos[1] == 0.0 and ident[1] == 1.0
        assert abs(ident[2]) <= 2.0 ** -24 and abs(cos[2] - 1.0) <= 2.0 ** -24          # 0 to one rounding
        assert trip[3] == 1.0 and trip[4] == 0.0 and (d == 1 or t_ref[0] > 0)          # d = 1: every cosine is +-1
    only = OB.identity_losses(a.to(DEV), p.to(DEV))                                       # without a negative: no triplet
    assert only[2] is None and np.array_equal(only[0].cpu().double().numpy(), cos) and np.array_equal(only[1].cpu().double().numpy(), ident)


# ---- MTCNN.detect on a float image ------------------------------------------------------------------------------------------------
class _Spy:
    """Records which library entries are called."""

    def __init__(self, lib):
        self._lib, self.calls = lib, set()

    def __getattr__(self, name):
        self.calls.add(name)
        return getattr(self._lib, name)


def test_mtcnn_detect_on_a_float_image(lib):
    """The boxes and probabilities of the oracle on the same float image, at test_cascade_matches_the_oracle's tolerances; the image is
    the one test_objective_cpu.py shows to decide > 1e-4 away from every threshold."""
    from faceposegenerator_amd import mtcnn as M
    from oracle import mtcnn_oracle as O
    w = M.synth_weights(5)
    m = M.MTCNN(select_largest=True, post_process=False, device=DEV, weights=w)
    m.lib = spy = _Spy(m.lib)
    img = R.mtcnn_float_image()
    boxes, inds, pts = m.detect_faces(img.to(DEV))
    assert "idb_crop_resize_area_f32" in spy.calls and "idb_crop_resize_area_u8" not in spy.calls
    b_ref, i_ref, p_ref = O.detect_face(img, w)
    print(f"MTCNN on a float image: {boxes.shape[0]} faces (oracle {b_ref.shape[0]}) on a 2 x 80x96 batch")
    assert boxes.shape[0] == b_ref.shape[0] > 0 and (inds == i_ref.numpy()).all()
    assert np.abs(boxes[:, :4] - b_ref[:, :4].numpy()).max() < 1e-2 and np.abs(boxes[:, 4] - b_ref[:, 4].numpy()).max() < 1e-5
    assert np.abs(pts - p_ref.numpy()).max() < 1e-2
    bb, pp = m.detect(img, landmarks=False)                                               # the reference's call (:1085)
    assert bb.shape == (2,) and bb[0].shape[1:] == (4,) and pp[0].shape == (bb[0].shape[0],)
    # the same image rounded to uint8 still goes through the u8 kernel, and gives what its integer-valued float twin gives
    spy.calls.clear()
    u8 = img.round().to(torch.uint8)
    b8, i8, p8 = m.detect_faces(u8.to(DEV))
    assert "idb_crop_resize_area_u8" in spy.calls and "idb_crop_resize_area_f32" not in spy.calls
    bf, jf, pf = m.detect_faces(u8.float().to(DEV))
    assert np.array_equal(b8, bf) and np.array_equal(i8, jf) and np.array_equal(p8, pf)
    with pytest.raises(ValueError):
        m.detect(img.double())


# ---- end to end on TINY_UNET / TINY_VAE -------------------------------------------------------------------------------------------
SIDE = 128
BOX = np.array([[20.7, 10.2, 100.9, 117.5]])          # x0, y0, x1, y1 -> rows 10..117, columns 20..100
DTYPES = {"f16": torch.float16, "bf16": torch.bfloat16}
ARC_BOUNDS = {"f16": (0.9995, 5e-3), "bf16": (0.995, 4e-2)}        # tests/test_arcface_gpu.py BOUNDS: cosine, relative L2 of r18 embeddings

# Free-running |gpu - oracle| / oracle of `instance` and `prior` over seeds 0, 1, 2 and the batches [1;1], [2;2] (12 values per dtype),
# measured on an MI355X: the largest value seen, and the bound = 3 x that.
FREE_RUN_MEASURED = {"f16": 1.467e-4, "bf16": 1.062e-3}


@pytest.fixture(scope="module")
def weights():
    from faceposegenerator_amd import arcface as A, weights as W
    return dict(unet=W.synth_unet(S.TINY_UNET, 7), vae=W.synth_vae(S.TINY_VAE, 8), enc=W.synth_vae_encoder(S.TINY_VAE, 21),
                arc=A.synth_weights("r18", 0))


def _pipe(weights, dt, prediction_type="epsilon"):
    from faceposegenerator_amd.pipeline import StableDiffusionPipeline
    ucfg = S.UNetConfig(**{**S.TINY_UNET.__dict__, "prediction_type": prediction_type})
    pipe = StableDiffusionPipeline(ucfg, S.TINY_VAE, weights["unet"], weights["vae"], torch_dtype=DTYPES[dt]).to(DEV)
    pipe.set_vae_encoder_weights(weights["enc"])
    return pipe


def _batch(seed, n):
    g = torch.Generator().manual_seed(1000 + seed)
    B = 2 * n
    return dict(x=torch.rand(B, 3, SIDE, SIDE, generator=g) * 2 - 1, emb=torch.randn(B, 512, generator=g),
                ehs=torch.randn(B, 77, S.TINY_UNET.cross_attention_dim, generator=g),
                ts=torch.tensor([[137, 802], [137, 455, 802, 999]][n - 1]), noise=torch.randn(B, 4, SIDE // 8, SIDE // 8, generator=g),
                ln=torch.randn(B, 4, SIDE // 8, SIDE // 8, generator=g))


@pytest.fixture(scope="module", params=["f16", "bf16"])
def rig(request, lib, weights):
    from faceposegenerator_amd import arcface as A
    dt = request.param
    return dict(dt=dt, pipe=_pipe(weights, dt), arc=A.ArcFace.from_state_dict(weights["arc"], "r18", DTYPES[dt]).to(DEV), w=weights)


@pytest.mark.parametrize("which", ["identity", "triplet_prior"])
@pytest.mark.parametrize("n", [1, 2], ids=["1+1", "2+2"])
def test_step_losses_teacher_forced(rig, n, which):
    """The GPU's own model_pred, x0_pred, 112 x 112 crops and features fed into the oracle's arithmetic: instance, prior, weight and
    combined to 1e-6 relative; the ArcFace features of the GPU's crops against tests/arcface_oracle.py within test_arcface_gpu.py's
    r18 bounds (cosine, relative L2 r), and the loss's cosine within 2 r / (1 - r) of the oracle's (unit vectors whose originals differ
    by r |a| differ by at most 2 r / (1 - r))."""
    b = _batch(5, n)
    obj = OB.TrainingObjective(rig["pipe"], arcface=rig["arc"], prior_loss_weight=0.7, which_loss=which)
    r = obj.step_losses(b["x"], b["emb"], b["ehs"], timesteps=b["ts"], noise=b["noise"], latent_noise=b["ln"],
                        detector=lambda im: [BOX] * n, keep=True)
    ac = rig["pipe"].scheduler.alphas_cumprod
    pred, target, noisy = (r[k].cpu() for k in ("model_pred", "target", "noisy"))
    assert all(r["detected"]) and r["bbox"] == [(10, 117, 20, 100)] * n and r["timesteps"] == b["ts"].tolist()
    # the pieces between the networks
    n_ref, t_ref = R.diffuse_targets(r["latents"].cpu(), b["noise"], b["ts"], ac, False)
    assert torch.allclose(noisy.double(), n_ref, rtol=2e-6, atol=1e-6) and torch.equal(target, b["noise"])
    x0_ref = R.pred_original_sample(pred, noisy, b["ts"], ac, False)[:n]
    assert torch.allclose(r["pred_original_sample"].cpu().double(), x0_ref, rtol=2e-6, atol=1e-6)
    inst, prior = R.mse_halves(pred, target, n)
    assert r["instance"] == pytest.approx(inst, rel=1e-6) and r["prior"] == pytest.approx(prior, rel=1e-6)
    weights = [R.timestep_weight(int(t), 1000) for t in b["ts"][:n]]
    assert r["weights"] == pytest.approx(weights, rel=1e-6)
    boxes = [[i, 10, 117, 20, 100] for i in range(n)]
    assert (r["faces"].cpu().double() - R.crop_resize_bilinear(r["images"].cpu(), boxes)).abs().max().item() <= 2e-6
    assert 0.0 <= r["images"].min().item() and r["images"].max().item() <= 255.0 and (r["images"] != r["images"].round()).any()
    # ArcFace on the GPU's crops
    feat = r["features"].cpu()
    f_ref = AO.forward(rig["w"]["arc"], "r18", r["faces"].cpu())
    cmin, rel_max = ARC_BOUNDS[rig["dt"]]
    cos_e = torch.nn.functional.cosine_similarity(feat, f_ref, dim=1).min().item()
    rel = ((feat - f_ref).norm(dim=1) / f_ref.norm(dim=1)).max().item()
    c_ref = R.identity_losses(f_ref, b["emb"][:n])[0]
    dcos = (torch.tensor(r["cos"], dtype=torch.float64) - c_ref).abs().max().item()
    print(f"[{rig['dt']}] {which} {n}+{n}: embedding cosine {cos_e:.6f}, relative L2 {rel:.3e}, |cos - oracle cos| {dcos:.3e}")
    assert cos_e >= cmin and rel <= rel_max and dcos <= 2 * rel_max / (1 - rel_max)
    # the losses from the GPU's features
    _, i_ref, t_ref = R.identity_losses(feat, b["emb"][:n], b["emb"][n:])
    l_ref = (t_ref if which == "triplet_prior" else i_ref).numpy()
    res = D.check(np.array(r["id_losses"]), l_ref, R.loss_bound(l_ref))
    assert res[0], D.describe("id_losses", res)
    comb = R.combined(inst, prior, l_ref.tolist(), weights, [True] * n, 0.7, which)
    assert r["combined"] == pytest.approx(comb, rel=1e-6) and r["id"] == pytest.approx(float(l_ref.mean()), rel=1e-6)
    assert r["weight"] == pytest.approx(float(np.mean(weights)), rel=1e-6)
    if n == 1:                                       # the reference's formula
        assert r["combined"] == pytest.approx(r["instance"] + 0.7 * r["prior"] + r["weight"] * r["id"], rel=1e-12)


def test_step_losses_v_prediction_and_weight_switch(lib, weights):
    b = _batch(6, 1)
    obj = OB.TrainingObjective(_pipe(weights, "f16", "v_prediction"), timestep_loss_weighting=False)
    r = obj.step_losses(b["x"], b["emb"], b["ehs"], timesteps=b["ts"], noise=b["noise"], latent_noise=b["ln"], keep=True)
    ac = obj.pipe.scheduler.alphas_cumprod
    lat = r["latents"].cpu()
    t_ref = R.diffuse_targets(lat, b["noise"], b["ts"], ac, True)[1]
    assert torch.allclose(r["target"].cpu().double(), t_ref, rtol=2e-6, atol=1e-6) and not torch.equal(r["target"].cpu(), b["noise"])
    x0_ref = R.pred_original_sample(r["model_pred"].cpu(), r["noisy"].cpu(), b["ts"], ac, True)[:1]
    assert torch.allclose(r["pred_original_sample"].cpu().double(), x0_ref, rtol=2e-6, atol=1e-6)
    inst, prior = R.mse_halves(r["model_pred"].cpu(), r["target"].cpu(), 1)
    assert r["instance"] == pytest.approx(inst, rel=1e-6) and r["prior"] == pytest.approx(prior, rel=1e-6) and r["weights"] == [1.0]


def _oracle_step(weights, b, n):
    """The whole CPU fp32 composition: oracle VAE encode + sample, the float64 targets rounded to fp32, the oracle UNet, the MSEs."""
    from faceposegenerator_amd.scheduler import DDPMScheduler
    from oracle import sd21_oracle as O
    with torch.no_grad():
        mean, logvar = O.vae_encode(weights["enc"], S.TINY_VAE, b["x"])
        lat = O.vae_latent_sample(mean, logvar, b["ln"], S.TINY_VAE.scaling_factor)
        noisy, target = (t.float() for t in R.diffuse_targets(lat, b["noise"], b["ts"], DDPMScheduler().alphas_cumprod, False))
        pred = O.unet_forward(weights["unet"], S.TINY_UNET, noisy, b["ts"], b["ehs"])
    return R.mse_halves(pred, target, n)


@pytest.fixture(scope="module")
def free_refs(weights):
    """Computed once, shared by both dtypes."""
    return {(seed, n): _oracle_step(weights, _batch(seed, n), n) for seed in (0, 1, 2) for n in (1, 2)}


def test_step_losses_free_running(rig, free_refs):
    """instance and prior against the whole CPU fp32 composition.  The deviation of f16 / bf16 operands through the VAE encoder and
    the UNet is not known in advance: it was measured over three seeds and two batch sizes (FREE_RUN_MEASURED, the largest value),
    and the bound is three times that.  Seeds move it by a small factor; a wrong coefficient, target or half moves it by orders of
    magnitude."""
    obj = OB.TrainingObjective(rig["pipe"])
    worst = 0.0
    for (seed, n), (inst, prior) in free_refs.items():
        b = _batch(seed, n)
        r = obj.step_losses(b["x"], b["emb"], b["ehs"], timesteps=b["ts"], noise=b["noise"], latent_noise=b["ln"])
        di, dp = abs(r["instance"] - inst) / inst, abs(r["prior"] - prior) / prior
        print(f"[{rig['dt']}] free-running seed {seed} {n}+{n}: instance {r['instance']:.6f} (oracle {inst:.6f}, rel {di:.3e}), "
              f"prior {r['prior']:.6f} (oracle {prior:.6f}, rel {dp:.3e})")
        worst = max(worst, di, dp)
    print(f"[{rig['dt']}] free-running: largest relative deviation {worst:.3e}")
    assert worst <= 3 * FREE_RUN_MEASURED[rig["dt"]]


# ---- remaining API checks ---------------------------------------------------------------------------------------------------------
def test_plain_loss_needs_no_face_models_and_undetected_faces_drop_the_term(rig):
    b = _batch(7, 1)
    kw = dict(timesteps=b["ts"], noise=b["noise"], latent_noise=b["ln"])
    plain = OB.TrainingObjective(rig["pipe"]).step_losses(b["x"], b["emb"], b["ehs"], **kw)
    assert plain["combined"] == plain["instance"] + plain["prior"] and plain["id"] == 0.0 and plain["detected"] == [False]
    assert plain["pred_original_sample"] is None
    obj = OB.TrainingObjective(rig["pipe"], arcface=rig["arc"], which_loss="identity")
    for found in (lambda im: None, lambda im: [None], lambda im: [np.array([[130.0, 10.0, 150.0, 40.0]])]):      # the last: empty after clipping
        r = obj.step_losses(b["x"], b["emb"], b["ehs"], detector=found, **kw)
        assert r["detected"] == [False] and r["id"] == 0.0 and r["bbox"] == [None]
        assert r["combined"] == r["instance"] + r["prior"] and r["instance"] == plain["instance"] and r["prior"] == plain["prior"]
        assert tuple(r["pred_original_sample"].shape) == (1, 4, SIDE // 8, SIDE // 8)
    with pytest.raises(ValueError):
        obj.step_losses(b["x"], b["emb"], b["ehs"], **kw)                                 # no MTCNN and no detector
    with pytest.raises(ValueError):
        obj.step_losses(b["x"], b["emb"], b["ehs"], timesteps=torch.tensor([5, 1000]), noise=b["noise"], latent_noise=b["ln"])
    solo = OB.TrainingObjective(rig["pipe"], with_prior_preservation=False).step_losses(b["x"][:1], b["emb"][:1], b["ehs"][:1], timesteps=b["ts"][:1],
                                                                                        noise=b["noise"][:1], latent_noise=b["ln"][:1])
    assert solo["prior"] == 0.0 and solo["combined"] == solo["instance"] > 0


def test_validation_losses_record_and_seed(rig):
    b = _batch(8, 2)
    obj = OB.TrainingObjective(rig["pipe"], arcface=rig["arc"], which_loss="identity")
    args = (obj, b["x"][:2], b["x"][2:], b["emb"][:2], b["emb"][2:], b["ehs"][:2])
    a = OB.validation_losses(*args, n_draws=3, seed=4, detector=lambda im: [BOX])
    assert set(OB.LOG_KEYS) <= set(a) and a["detection_rate"] == 1.0 and len(a["draws"]["combined"]) == 3
    assert a["Step Loss/Combined"] == pytest.approx(float(np.mean(a["draws"]["combined"])), rel=1e-12)
    assert a["Step Loss/Reconstruction"] > 0 and a["Step Loss/Prior"] > 0 and a["Step Loss/ID"] > 0
    assert OB.validation_losses(*args, n_draws=3, seed=4, detector=lambda im: [BOX]) == a      # identical on a second run
    assert OB.validation_losses(*args, n_draws=3, seed=5, detector=lambda im: [BOX])["draws"]["timesteps"] != a["draws"]["timesteps"]
