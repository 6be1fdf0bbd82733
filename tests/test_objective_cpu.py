"""CPU checks of the training objective's forward pass (faceposegenerator_amd/objective.py): the float64 oracle
(tests/objective_oracle.py) against torch itself and against this project's DDPMScheduler, the host policy of step_losses (box
truncation and clipping, timestep weight, the combined loss, the undetected rule, the draw order), the argument checks of the new
entry points (they run before any HIP call), and the condition the detector's float test image must meet."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import objective_oracle as R  # noqa: E402

from faceposegenerator_amd import objective as OB  # noqa: E402
from faceposegenerator_amd import spec as S  # noqa: E402
from faceposegenerator_amd.scheduler import DDPMScheduler  # noqa: E402

P = 0x1000          # a non-null, 16-byte aligned address for argument checks that never reach a launch
EINVAL, EUNSUPPORTED = -1, -2


def _sched(pt):
    return DDPMScheduler(S.SchedulerConfig(prediction_type=pt))


# ---- the oracle against torch ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pt", ["epsilon", "v_prediction"])
def test_oracle_matches_the_scheduler(pt):
    """add_noise, get_velocity and step(...).pred_original_sample at t in {0, 500, 999}.  The scheduler works in fp32 (coefficients
    rounded to fp32, then two products and a sum): per element at most ~4 roundings of terms of magnitude |sa x| + |sb n|, and the
    epsilon form of x0 divides that by sa (0.068 at t = 999)."""
    s = _sched(pt)
    g = torch.Generator().manual_seed(0)
    x0, noise, pred = (torch.randn(3, 4, 8, 10, generator=g) for _ in range(3))
    ts = torch.tensor([0, 500, 999])
    vp = pt == "v_prediction"
    noisy, target = R.diffuse_targets(x0, noise, ts, s.alphas_cumprod, vp)
    sa, sb = R.coefs(s.alphas_cumprod, ts)
    mag = sa * x0.abs().double() + sb * noise.abs().double()
    assert ((s.add_noise(x0, noise, ts).double() - noisy).abs() <= 4 * R.U32 * mag + 1e-30).all()
    want = s.get_velocity(x0, noise, ts) if vp else noise
    assert ((want.double() - target).abs() <= 4 * R.U32 * (sa * noise.abs() + sb * x0.abs()).double()).all()
    nz = noisy.float()
    ref = R.pred_original_sample(pred, nz, ts, s.alphas_cumprod, vp)
    for b, t in enumerate(ts.tolist()):
        got = s.step(pred[b:b + 1], t, nz[b:b + 1], variance_noise=torch.zeros(1, 4, 8, 10)).pred_original_sample
        m = (nz[b].abs().double() + sb[b] * pred[b].abs().double()) / (1.0 if vp else sa[b])
        assert ((got[0].double() - ref[b]).abs() <= 6 * R.U32 * m).all(), t


def test_oracle_mse_is_f_mse_loss():
    g = torch.Generator().manual_seed(1)
    a, b = torch.randn(4, 4, 8, 10, generator=g).double(), torch.randn(4, 4, 8, 10, generator=g).double()
    inst, prior = R.mse_halves(a, b, 2)
    assert inst == pytest.approx(F.mse_loss(a[:2], b[:2]).item(), rel=1e-14) and prior == pytest.approx(F.mse_loss(a[2:], b[2:]).item(), rel=1e-14)
    assert R.mse_halves(a, b, 4)[1] == 0.0


@pytest.mark.parametrize("d", [1, 512])
def test_oracle_losses_are_torchs(d):
    g = torch.Generator().manual_seed(2)
    a, p, n = (torch.randn(5, d, generator=g).double() for _ in range(3))
    a[1] = 0.0                                   # the eps clamp
    p[2] = a[2]                                  # cos = 1
    n[3] = a[3]                                  # hinge: d(a, n) = 0
    cos, ident, trip = R.identity_losses(a, p, n)
    want = torch.nn.CosineSimilarity(dim=1, eps=1e-6)(a, p)
    assert torch.allclose(cos, want, rtol=1e-13, atol=1e-15) and torch.allclose(ident, 1 - want, rtol=1e-13, atol=1e-15)
    assert cos[1] == 0.0 and abs(cos[2].item() - 1.0) < 1e-15

    def cosine_distance(x, y):                   # train_ID-Booth.py:974-977
        return 1 - F.cosine_similarity(x, y)

    loss = torch.nn.TripletMarginWithDistanceLoss(distance_function=cosine_distance, reduction="none")(a, p, n)
    assert torch.allclose(trip, loss, rtol=1e-13, atol=1e-15)
    assert (trip > 0).any() and (trip >= 0).all()


@pytest.mark.parametrize("hw,out", [((13, 20), (112, 112)), ((300, 280), (112, 112)), ((1, 17), (5, 9)), ((9, 1), (4, 3)), ((112, 112), (112, 112))])
def test_oracle_bilinear_is_f_interpolate(hw, out):
    img = torch.rand(3, *hw, generator=torch.Generator().manual_seed(3)).double() * 255
    want = F.interpolate(img[None], size=out, mode="bilinear", align_corners=False, antialias=False)[0]
    got = torch.from_numpy(R.bilinear_restated(img.numpy(), *out))
    # the two computations round the source coordinate (<= the input size) differently: a weight may differ by a few ulps of it
    assert (got - want).abs().max().item() <= 255 * 4 * max(hw) * 2.0 ** -52
    nhwc = img.permute(1, 2, 0)[None].contiguous()
    box = [[0, 0, hw[0], 0, hw[1]]]
    assert torch.allclose(R.crop_resize_bilinear(nhwc, box, *out), R.crop_resize_bilinear(nhwc, box, *out, restated=True), rtol=0, atol=1e-13)


# ---- host policy ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("box,want", [((10.9, 20.2, 50.99, 60.5), (20, 60, 10, 50)),             # truncation, not rounding
                                      ((-3.7, -0.5, 40.2, 30.9), (0, 30, 0, 40)),                # a negative corner: astype(int) gives -3 and 0
                                      ((100.5, 90.1, 140.8, 131.9), (90, 128, 100, 128)),        # a corner beyond S = 128
                                      ((130.0, 10.0, 150.0, 40.0), None),                        # empty: wholly right of the image
                                      ((10.2, 10.9, 10.8, 40.0), None),                          # empty: x0 == x1 after truncation
                                      ((5.0, -9.0, 50.0, -2.0), None)])                          # the end itself negative
def test_box_truncation_and_clipping(box, want):
    assert OB.clip_box(np.array(box, dtype=np.float32), 128) == want == R.clip_box(box, 128)
    if want is not None:                         # the reference's expression on a real image
        img = np.zeros((128, 128, 3))
        b = np.array(box, dtype=np.float32).astype(int)
        crop = img[max(0, b[1]):min(b[3], 128), max(0, b[0]):min(b[2], 128)]
        assert crop.shape[:2] == (want[1] - want[0], want[3] - want[2])


def test_timestep_weight_and_its_switch():
    for t in (0, 1, 500, 999):
        assert OB.timestep_weight(t, 1000) == pytest.approx((1 - t / 1000) ** 2, rel=1e-15) == R.timestep_weight(t, 1000)
        assert OB.timestep_weight(t, 1000, False) == 1.0
    assert OB.timestep_weight(0, 1000) == 1.0 and OB.timestep_weight(999, 1000) == pytest.approx(1e-6, rel=1e-9)


@pytest.mark.parametrize("which", ["", "identity", "triplet_prior"])
def test_combined_formula_and_the_undetected_rule(which):
    inst, prior, plw = 0.25, 0.5, 0.7
    r = OB.combine(inst, prior, [0.8], [0.36], [True], plw, which)
    want = inst + plw * prior + (0.36 * 0.8 if which else 0.0)
    assert r["combined"] == pytest.approx(want, rel=1e-15) == R.combined(inst, prior, [0.8], [0.36], [True], plw, which)
    assert r["id"] == (0.8 if which else 0.0)
    # undetected: the term is left out, id is 0
    r = OB.combine(inst, prior, [0.0], [0.36], [False], plw, which)
    assert r["combined"] == pytest.approx(inst + plw * prior, rel=1e-15) and r["id"] == 0.0
    # several instances: the mean over the detected ones
    r = OB.combine(inst, prior, [0.8, 0.0, 0.4], [0.36, 1.0, 0.04], [True, False, True], plw, which)
    want = inst + plw * prior + ((0.36 * 0.8 + 0.04 * 0.4) / 2 if which else 0.0)
    assert r["combined"] == pytest.approx(want, rel=1e-15) == R.combined(inst, prior, [0.8, 0.0, 0.4], [0.36, 1.0, 0.04], [True, False, True], plw, which)
    assert r["id"] == pytest.approx(0.6 if which else 0.0)
    with pytest.raises(ValueError):
        OB.combine(inst, prior, [0.8], [1.0], [True], plw, "triplet")


def test_draw_order_with_a_seeded_generator():
    """encoder sample noise, then randn_like, then randint (train_ID-Booth.py:1001, :1007, :1010)."""
    shape = (2, 4, 16, 16)
    ln, nz, ts = OB.draw_step_inputs(shape, 1000, torch.Generator().manual_seed(5))
    g = torch.Generator().manual_seed(5)
    a = torch.randn(shape, generator=g)
    b = torch.randn(shape, generator=g)
    c = torch.randint(0, 1000, (2,), generator=g)
    assert torch.equal(ln, a) and torch.equal(nz, b) and torch.equal(ts, c) and ts.dtype == torch.int64
    assert not torch.equal(ln, nz)


def test_constructor_policy():
    with pytest.raises(ValueError):
        OB.TrainingObjective(None, which_loss="arcface")
    with pytest.raises(ValueError):
        OB.TrainingObjective(None, which_loss="identity")                       # no ArcFace model
    with pytest.raises(ValueError):
        OB.TrainingObjective(None, arcface=object(), which_loss="identity", with_prior_preservation=False)
    o = OB.TrainingObjective(None)
    assert o.which_loss == "" and o.prior_loss_weight == 1.0 and o.timestep_loss_weighting and o.with_prior_preservation
    assert OB.LOG_KEYS == ("Step Loss/Reconstruction", "Step Loss/Prior", "Step Loss/ID", "Step Loss/Combined")


def test_load_images_is_the_datasets_transform():
    from PIL import Image
    rng = np.random.default_rng(0)
    sq = rng.integers(0, 256, size=(32, 32, 3), dtype=np.uint8)
    x = OB.load_images([sq], 32)
    assert x.shape == (1, 3, 32, 32) and torch.equal(x[0], (torch.from_numpy(sq).permute(2, 0, 1).float() / 255 - 0.5) / 0.5)
    wide = rng.integers(0, 256, size=(40, 60, 3), dtype=np.uint8)
    y = OB.load_images([Image.fromarray(wide)], 20)                             # short side 40 -> 20, long 60 -> 30, centre crop 20
    ref = np.asarray(Image.fromarray(wide).resize((30, 20), Image.BILINEAR))[:, 5:25]
    assert torch.equal(y[0], (torch.from_numpy(ref.copy()).permute(2, 0, 1).float() / 255 - 0.5) / 0.5)


# ---- argument checks (before any HIP call) ------------------------------------------------------------------------------------------
def _refused(lib, rc, status, text):
    assert rc == status and text.encode() in lib.idb_last_error(), (rc, lib.idb_last_error())


def test_argument_checks(lib):
    ok = lambda **kw: {**dict(x0=P, noise=P, ts=P, ac=P, T=1000, pt=0, b=2, c=4, hw=64, noisy=P, target=P), **kw}      # noqa: E731
    dt = lambda a: lib.idb_diffuse_targets(a["x0"], a["noise"], a["ts"], a["ac"], a["T"], a["pt"], a["b"], a["c"], a["hw"], a["noisy"], a["target"], None)      # noqa: E731
    _refused(lib, dt(ok(x0=None)), EINVAL, "idb_diffuse_targets: null pointer")
    _refused(lib, dt(ok(ts=None)), EINVAL, "idb_diffuse_targets: timesteps")
    _refused(lib, dt(ok(b=0)), EINVAL, "idb_diffuse_targets: batch")
    _refused(lib, dt(ok(c=1 << 16, hw=1 << 15)), EINVAL, "idb_diffuse_targets: batch")
    _refused(lib, dt(ok(pt=2)), EUNSUPPORTED, "prediction_type 2")
    _refused(lib, dt(ok(noisy=P + 2)), EINVAL, "unaligned")
    assert lib.idb_objective_workspace_bytes(2, 4 * 64 * 64) == 2 * 16 * 8 and lib.idb_objective_workspace_bytes(3, 320) == 3 * 8
    assert lib.idb_objective_workspace_bytes(0, 64) == 0 and lib.idb_objective_workspace_bytes(1, 1 << 31) == 0
    mse = lambda **kw: (lambda a: lib.idb_objective_mse_x0(a["pred"], 0, a["target"], a["noisy"], P, P, 1000, a["pt"], 2, 4, 4096, a["sse"], a["x0"],      # noqa: E731
                                                           a["ws"], a["wsb"], None))({**dict(pred=P, target=P, noisy=P, pt=1, sse=P, x0=P, ws=P, wsb=64), **kw})
    _refused(lib, mse(pred=None), EINVAL, "idb_objective_mse_x0: null pointer")
    _refused(lib, mse(noisy=None), EINVAL, "x0_pred needs noisy")
    _refused(lib, mse(wsb=63), EINVAL, "workspace of 63 bytes, 64 needed")
    _refused(lib, mse(pt=-1), EUNSUPPORTED, "prediction_type -1")
    _refused(lib, mse(sse=P + 4), EINVAL, "unaligned")
    bl = lib.idb_crop_resize_bilinear_f32
    _refused(lib, bl(None, 1, 8, 8, 3, P, 1, P, 112, 112, None), EINVAL, "idb_crop_resize_bilinear_f32: bad arguments")
    _refused(lib, bl(P, 1, 8, 8, 3, P, 1, P, 0, 112, None), EINVAL, "idb_crop_resize_bilinear_f32: bad arguments")
    _refused(lib, bl(P, 1, 1 << 16, 1 << 15, 3, P, 1, P, 112, 112, None), EINVAL, "image plane or box count too large")
    assert bl(P, 1, 8, 8, 3, P, 0, P, 112, 112, None) == 0                      # nothing to do: no launch
    ar = lib.idb_crop_resize_area_f32
    _refused(lib, ar(None, 1, 8, 8, 3, P, 1, P, 24, 24, 127.5, 0.0078125, None), EINVAL, "idb_crop_resize_area_f32: bad arguments")
    _refused(lib, ar(P + 2, 1, 8, 8, 3, P, 1, P, 24, 24, 127.5, 0.0078125, None), EINVAL, "idb_crop_resize_area_f32: unaligned image")
    assert ar(P, 1, 8, 8, 3, P, 0, P, 24, 24, 127.5, 0.0078125, None) == 0
    il = lib.idb_identity_losses
    _refused(lib, il(P, None, None, 1, 512, P, P, None, None), EINVAL, "idb_identity_losses: null pointer")
    _refused(lib, il(P, P, P, 1, 512, P, P, None, None), EINVAL, "neg and triplet go together")
    _refused(lib, il(P, P, None, 0, 512, P, P, None, None), EINVAL, "idb_identity_losses: n 1..2^30")
    _refused(lib, il(P, P, None, 1, 8193, P, P, None, None), EUNSUPPORTED, "d 8193")


# ---- the detector's float test image ------------------------------------------------------------------------------------------------
def test_float_detector_image_decides_away_from_the_thresholds():
    """The GPU test compares detect() on this float image with the oracle box for box: that is only meaningful when no face
    probability of the oracle's own run lies within 1e-4 of its stage threshold (the kernels agree with the oracle to 1e-5)."""
    from faceposegenerator_amd import mtcnn as M
    from oracle import mtcnn_oracle as O
    img = R.mtcnn_float_image()
    assert img.dtype == torch.float32 and 0 <= img.min() and img.max() <= 255 and (img != img.round()).any()
    w = M.synth_weights(5)
    margin = R.mtcnn_threshold_margin(img, w)
    assert margin is not None and margin > 1e-4, margin
    assert O.detect_face(img, w)[0].shape[0] > 0
