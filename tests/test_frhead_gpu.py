"""The FR loss head on the GPU: idb_head_logits per element and idb_head_loss per row against the float64 oracle (tests/frhead_oracle.py,
itself checked against recordings of the reference's classes in test_frhead_cpu.py).  Every bound below is derived, none is measured;
the measured maxima are printed by the last test of the file.

Logits, u = 2^-24, s = 64.  The kernel rounds each normalised embedding component once (the division is done in double) and each
normalised kernel component once: with unit rows and columns, sum |a_k b_k| <= 1, that moves the cosine by at most 2 u.  The f32 MFMA
is a k-ordered fma chain, D roundings of partial sums of magnitude <= 1: D u (first order; the factor 1.001 covers 1 / (1 - D u)).  The
clamp bound 1 - 1e-3 is rounded to fp32 (u) and the scale s c rounds once more (u): a logit is within s (D + 4) u 1.001 of the oracle,
1.97e-3 at D = 512.  AdaFace takes its rows as given; the test gives it fp32-rounded unit rows, whose norm is within u of 1.
Target logit, v = 2^-53.  The target cosine is a double dot product of exact products over the double norms: (2 D + 8) v on either
side, e = (4 D + 16) v between kernel and oracle.  CosFace: s (e + 8 v).  AdaFace clamps to |c| <= 1 - 1e-3 first, where acos has
slope <= 22.4: s (22.4 e + 16 v + 2 m ds) with ds the error of the margin scaler (below).  ArcFace: acos has slope 1 / sqrt(1 - c^2)
away from +-1 and is Hoelder-1/2 everywhere, |acos a - acos b| <= (pi / 2) sqrt(2 |a - b|) (equality of acos(1 - t) and
(pi / 2) sqrt(2 t) at t = 2, ratio increasing in t): per row s (min(e / sqrt(1 - (|c| + e)^2), (pi / 2) sqrt(2 e)) + 16 v), which at
a cosine within 1e-7 of 1 is 6.8e-5 at D = 512 -- thirty times below the fp32-sized bound, where an fp32 acos would be off by 0.8.
In `thetas` the target is stored as fp32: half an ulp of a value below 128, 2^-18, more.
Log-sum-exp: 1-Lipschitz in the maximum norm, so the logit bound carries over (the replaced target entry: its 2^-18).  Each term is
expf(z - max) in fp32: the difference of two logits, below 256 in magnitude, rounds by 2^-17, expf by an ulp, both relative errors of
the term and so absolute errors of the logarithm: 2^-17 + 4 u.  The sums over C, the rescaling exponentials (one per tile and one per
column block, in double) and the logarithm are double: (C + 300) v relative, taken on 4 s.  loss_i = lse - target: both bounds.
Margin scaler: mean and deviation sums over B doubles of at most 100, (B + 8) v relative each; through (safe - mean) / (std + 1e-3) h
that is at most h (2 B + 16) v (|safe - mean| + mean) / (std + 1e-3) on either side, twice that between the two.
Prediction: on a row whose float64 top-two gap exceeds twice the logit bound the order of the two cannot flip; other rows accept either
contender, and at most 5 % of a case's rows may be such rows (the seeds keep the oracle under that share: test_frhead_cpu.py).
"""
import ctypes as C
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import arcface_oracle as AO  # noqa: E402
import frhead_oracle as O  # noqa: E402

from faceposegenerator_amd import _lib  # noqa: E402
from faceposegenerator_amd import arcface as A  # noqa: E402
from faceposegenerator_amd import frhead as H  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ARC_BOUNDS = (0.9995, 5e-3)                                   # test_arcface_gpu.BOUNDS[torch.float16]: cosine, relative L2
MEASURED = {}                                                 # (what, loss, D) -> (largest error, its bound)


def _note(what, loss, D, err, bound):
    key = (what, loss, D)
    if key not in MEASURED or err / bound > MEASURED[key][0] / MEASURED[key][1]:
        MEASURED[key] = (float(err), float(bound))


def _kw(loss, norms, **more):
    return dict(norms=norms, **more) if loss == "AdaFace" else {}


@functools.lru_cache(maxsize=None)
def _reference(loss, B, Cn, D):
    emb, kernel, labels, norms = O.inputs(loss, B, Cn, D, O.gpu_seed(loss, B, Cn, D))
    th, extras = O.thetas(loss, emb, kernel, labels, **_kw(loss, norms))
    return emb, kernel, labels, norms, th, extras, O.cross_entropy(th, labels), O.target_cosine(loss, emb, kernel, labels)


def _scaler_err(B, norms, extras, h=0.333):
    safe = np.clip(norms.astype(np.float64), 0.001, 100)
    mean, std = extras["batch_mean"], extras["batch_std"]
    return 2 * h * (2 * B + 16) * O.U64 * (np.abs(safe - mean).max() + mean) / (std + O.EPS)


def _check(loss, D, header, emb, labels, norms, th, ce, cos_t, extras, tag=None):
    """Everything the loss and logits routes return for one batch, against the oracle's thetas `th`."""
    B, Cn = th.shape
    rows_i = np.arange(B)
    mean_want, per_want, lse_want = ce
    t_lab = torch.from_numpy(labels)
    t_emb = torch.from_numpy(emb)
    args = (t_emb, torch.from_numpy(norms), t_lab) if loss == "AdaFace" else (t_emb, t_lab)
    got_th = header(*args)
    assert got_th.dtype == torch.float32 and tuple(got_th.shape) == (B, Cn) and got_th.is_cuda
    got_th = got_th.cpu().numpy().astype(np.float64)
    out = header.loss(t_emb, t_lab, **_kw(loss, torch.from_numpy(norms)))
    again = header.loss(t_emb, t_lab, **_kw(loss, torch.from_numpy(norms)))
    for a, b in ((out.per_sample, again.per_sample), (out.lse, again.lse), (out.target_logit, again.target_logit), (out.pred, again.pred)):
        assert torch.equal(a, b)                              # bit-identical from run to run
    assert (out.loss, out.correct, out.acc) == (again.loss, again.correct, again.acc)
    lb, sb = O.logit_bound(D), O.lse_bound(D, Cn)
    tb = O.target_bound(loss, D, cos_t, scaler_err=_scaler_err(B, norms, extras) if loss == "AdaFace" else 0.0)
    # logits per element: the target column against its double-sized bound (+ its fp32 storage), every other entry against the fp32 one
    err = np.abs(got_th - th)
    t_err = err[rows_i, labels].copy()
    err[rows_i, labels] = 0
    tag = tag or loss
    _note("logit", tag, D, err.max(), lb)
    _note("target in thetas", tag, D, (t_err / (tb + 2.0 ** -18)).max(), 1.0)
    assert err.max() <= lb, (err.max(), lb)
    assert (t_err <= tb + 2.0 ** -18).all(), (t_err.max(), tb.max())
    # per-row values of the loss route
    lse, per, tgt = out.lse.cpu().numpy(), out.per_sample.cpu().numpy(), out.target_logit.cpu().numpy()
    tg_err = np.abs(tgt - th[rows_i, labels])
    _note("target logit", tag, D, (tg_err / tb).max(), 1.0)
    _note("target logit (abs)", tag, D, tg_err.max(), tb.max())
    _note("lse", tag, D, np.abs(lse - lse_want).max(), sb)
    _note("loss_i", tag, D, (np.abs(per - per_want) / (sb + tb)).max(), 1.0)
    assert (tg_err <= tb).all(), (tg_err.max(), tb.max())
    assert np.abs(lse - lse_want).max() <= sb, (np.abs(lse - lse_want).max(), sb)
    assert (np.abs(per - per_want) <= sb + tb).all()
    assert np.array_equal(per, lse - tgt)
    # the two routes run the same fma chains: the loss route's argmax and log-sum-exp are those of the logits route's matrix
    pred = out.pred.cpu().numpy()
    assert out.pred.dtype == torch.int32 and np.array_equal(pred, np.argmax(got_th, axis=1))
    lse_th = O.cross_entropy(got_th, labels)[2]
    assert np.abs(lse - lse_th).max() <= 2.0 ** -17 * 1.001 + 4 * O.U32 + (Cn + 300) * O.U64 * 4 * O.S
    # prediction against the oracle
    want_pred, unsure = O.argmax(th), O.ambiguous_rows(th, lb) if Cn > 1 else np.zeros(B, dtype=bool)
    assert unsure.mean() <= 0.05
    assert np.array_equal(pred[~unsure], want_pred[~unsure])
    for i in np.nonzero(unsure)[0]:
        assert th[i, pred[i]] >= th[i].max() - 2 * lb
    # the batch numbers from the per-row values
    assert out.correct == int((pred == labels).sum()) and out.acc == O.multi_class_acc(pred, labels)
    assert abs(out.loss - per.sum() / B) <= (B + 2) * O.U64 * np.abs(per).max()
    assert abs(out.loss - mean_want) <= (sb + tb.max()) + (B + 2) * O.U64 * 4 * O.S
    return out, got_th


def _header(loss, kernel, **kw):
    return H.MarginHeader(torch.from_numpy(np.ascontiguousarray(kernel)), loss, **kw).to(DEV)


# ---- every shape, every loss ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss,B,Cn,D", O.gpu_cases(), ids=lambda v: str(v))
def test_logits_and_loss_against_oracle(lib, loss, B, Cn, D):
    emb, kernel, labels, norms, th, extras, ce, cos_t = _reference(loss, B, Cn, D)
    header = _header(loss, kernel)
    rt, cb = header.plan(B)
    assert rt == (B + 127) // 128 and 1 <= cb <= (Cn + 31) // 32
    if (B, Cn) == (130, 4099):
        assert rt > 1 and cb > 1                              # more than one row tile, more than one column block
    out, _ = _check(loss, D, header, emb, labels, norms, th, ce, cos_t, extras)
    if loss == "AdaFace":
        serr = _scaler_err(B, norms, extras)
        got = out.margin_scaler.cpu().numpy()
        _note("margin scaler", loss, D, np.abs(got - extras["margin_scaler"]).max(), serr)
        assert np.abs(got - extras["margin_scaler"]).max() <= serr
        assert abs(header.batch_mean - extras["batch_mean"]) <= (B + 8) * O.U64 * 100
        assert abs(header.batch_std - extras["batch_std"]) <= (B + 8) * O.U64 * 100


# ---- the target near +-1 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss", ["ArcFace", "AdaFace"])
def test_target_cosine_within_1e7_of_one(lib, loss):
    """Target columns along (even rows) and against (odd rows) their embedding, 1e-7 off the direction: acos has no slope there, and the
    target logit is still within the double-sized bound (the Hoelder branch of target_bound)."""
    B, Cn, D = 20, 33, 512
    rng = np.random.default_rng(5)
    emb, kernel, _, norms = O.inputs(loss, B, Cn, D, 77)
    emb, kernel = emb.copy(), kernel.copy()
    labels = rng.permutation(Cn)[:B].astype(np.int64)
    unit = emb.astype(np.float64) / np.linalg.norm(emb.astype(np.float64), axis=1, keepdims=True)
    sign = np.where(np.arange(B) % 2 == 0, 1.0, -1.0)[:, None]
    kernel[:, labels] = (sign * (unit + 1e-7 * rng.standard_normal((B, D)) / math.sqrt(D)) * 0.3).T.astype(np.float32)
    th, extras = O.thetas(loss, emb, kernel, labels, **_kw(loss, norms))
    cos_t = O.target_cosine(loss, emb, kernel, labels)
    # ArcFace normalises the rows; AdaFace takes the fp32-rounded unit rows as they are, so its cosine is 1 only up to their norm
    assert (np.abs(1 - np.abs(cos_t)) <= (1e-13 if loss == "ArcFace" else 1e-8)).all()
    header = _header(loss, kernel)
    _check(loss, D, header, emb, labels, norms, th, O.cross_entropy(th, labels), cos_t, extras, tag=loss + " target at +-1")


# ---- argmax --------------------------------------------------------------------------------------------------------------------------
def test_duplicate_columns_give_the_lower_index(lib):
    """Bit-identical columns give bit-identical logits; the argmax is the lower index, within a tile (7, 9), across the two half-waves
    of a tile (3, 20: rows 3 and 20 of a 32-row MFMA tile belong to different half-waves) and across column blocks (5, C - 1)."""
    B, Cn, D = 130, 4099, 130
    emb, kernel, labels, norms = O.inputs("ArcFace", B, Cn, D, 9)
    kernel, emb = kernel.copy(), emb.copy()
    kernel[:, 9], kernel[:, 20], kernel[:, Cn - 1] = kernel[:, 7], kernel[:, 3], kernel[:, 5]
    for i, col in enumerate((7, 3, 5)):                      # rows 0..2 and 127..129 (both row tiles) point at the duplicated columns
        emb[i] = kernel[:, col] * 50
        emb[127 + i] = kernel[:, col] * 70
    labels = np.full(B, 100, dtype=np.int64)                  # the target is none of them
    header = _header("ArcFace", kernel)
    assert header.plan(B)[1] > 1
    out = header.loss(torch.from_numpy(emb), torch.from_numpy(labels))
    pred = out.pred.cpu().numpy()
    assert pred[[0, 1, 2, 127, 128, 129]].tolist() == [7, 3, 5, 7, 3, 5]
    th = header(torch.from_numpy(emb), torch.from_numpy(labels)).cpu().numpy()
    assert (th[:, 9] == th[:, 7]).all() and (th[:, 20] == th[:, 3]).all() and (th[:, Cn - 1] == th[:, 5]).all()
    assert np.array_equal(pred, np.argmax(th, axis=1))


# ---- target replacement --------------------------------------------------------------------------------------------------------------
def test_margin_takes_the_argmax_from_the_target(lib):
    """CosFace, m = 0.35: the target is the row's largest cosine and loses the argmax once its margin is subtracted."""
    B, Cn, D = 37, 33, 130
    emb, kernel, labels, norms = O.inputs("CosFace", B, Cn, D, 21)
    emb = emb.copy()
    wn = kernel.astype(np.float64) / np.linalg.norm(kernel.astype(np.float64), axis=0)
    other = (labels + 1) % Cn
    emb[:] = ((0.62 * wn[:, labels] + 0.45 * wn[:, other]).T * 17).astype(np.float32)
    th, _ = O.thetas("CosFace", emb, kernel, labels)
    plain, _ = O.thetas("CosFace", emb, kernel, labels, m=0.0)
    assert np.array_equal(O.argmax(plain), labels) and np.array_equal(O.argmax(th), other)
    header = _header("CosFace", kernel)
    out, _ = _check("CosFace", D, header, emb, labels, norms, th, O.cross_entropy(th, labels), O.target_cosine("CosFace", emb, kernel, labels), {})
    assert np.array_equal(out.pred.cpu().numpy(), other) and out.correct == 0 and out.acc == 0.0


@pytest.mark.parametrize("loss", ["CosFace", "ArcFace", "AdaFace"])
@pytest.mark.parametrize("Cn", [33, 301, 4099])
def test_label_in_the_last_column_of_the_last_partial_tile(lib, loss, Cn):
    B, D = 37, 130
    emb, kernel, labels, norms = O.inputs(loss, B, Cn, D, 31 + Cn)
    labels = np.full(B, Cn - 1, dtype=np.int64)
    th, extras = O.thetas(loss, emb, kernel, labels, **_kw(loss, norms))
    header = _header(loss, kernel)
    _check(loss, D, header, emb, labels, norms, th, O.cross_entropy(th, labels), O.target_cosine(loss, emb, kernel, labels), extras)


# ---- AdaFace -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t_alpha", [1.0, 0.3])
def test_adaface_statistics_and_buffers(lib, t_alpha):
    """Two consecutive calls: the buffers follow upstream's EMA from their defaults (20, 100), the margin scaler uses the UPDATED ones."""
    B, Cn, D = 37, 301, 130
    emb, kernel, labels, norms = O.inputs("AdaFace", B, Cn, D, 13)
    header = _header("AdaFace", kernel, t_alpha=t_alpha)
    assert (header.batch_mean, header.batch_std) == (20.0, 100.0)
    mean, std = 20.0, 100.0
    for step in range(2):
        nrm = norms * (1.0 + 0.5 * step)
        nrm[0], nrm[1] = 1e-4, 250.0                          # clipped to 0.001 and 100
        th, extras = O.thetas("AdaFace", emb, kernel, labels, norms=nrm, t_alpha=t_alpha, batch_mean=mean, batch_std=std)
        out = header.loss(torch.from_numpy(emb), torch.from_numpy(labels), norms=torch.from_numpy(nrm))
        mean, std = extras["batch_mean"], extras["batch_std"]
        assert abs(header.batch_mean - mean) <= (B + 8) * O.U64 * 100 and abs(header.batch_std - std) <= (B + 8) * O.U64 * 100
        serr = _scaler_err(B, nrm, extras)
        assert np.abs(out.margin_scaler.cpu().numpy() - extras["margin_scaler"]).max() <= serr
        tb = O.target_bound("AdaFace", D, 0.0, scaler_err=serr)
        rows_i = np.arange(B)
        assert (np.abs(out.target_logit.cpu().numpy() - th[rows_i, labels]) <= tb).all()
        assert np.abs(out.lse.cpu().numpy() - O.cross_entropy(th, labels)[2]).max() <= O.lse_bound(D, Cn)
        header.set_buffers(mean, std)                         # the oracle's doubles, so that the second step compares one update only


def test_adaface_clamps_every_entry(lib):
    """A non-target column along an embedding: cosine 1 reads s (1 - eps), cosine -1 reads -s (1 - eps); the bound is the rounding of
    0.999 to fp32 and of its product with s."""
    B, Cn, D = 4, 33, 130
    emb, kernel, labels, norms = O.inputs("AdaFace", B, Cn, D, 17)
    kernel = kernel.copy()
    labels = np.array([20, 21, 22, 23], dtype=np.int64)
    kernel[:, 2], kernel[:, 3] = emb[0] * 2, -emb[1] * 3
    th = _header("AdaFace", kernel)(torch.from_numpy(emb), torch.from_numpy(norms), torch.from_numpy(labels)).cpu().numpy().astype(np.float64)
    want = O.S * (1 - O.EPS)
    assert abs(th[0, 2] - want) <= 2 * O.S * O.U32 and abs(th[1, 3] + want) <= 2 * O.S * O.U32
    off_target = np.abs(th).copy()
    off_target[np.arange(B), labels] = 0
    assert off_target.max() <= want + 2 * O.S * O.U32


def test_adaface_literal_loop_norms(lib):
    """The loop's own call: norms of the already normalised features, all 1 up to fp32 rounding.  The oracle is fed the GPU's norms
    and rows; only the formula is compared."""
    B, Cn, D = 37, 301, 512
    emb, kernel, labels, _ = O.inputs("AdaFace", B, Cn, D, 19)
    feats = torch.nn.functional.normalize(torch.from_numpy(emb * 7).to(DEV))
    norm = torch.norm(feats, 2, 1, True)
    unit = torch.div(feats, norm)
    g_norm, g_unit = norm.cpu().numpy(), unit.cpu().numpy()
    assert np.abs(g_norm - 1).max() <= 4 * O.U32 * 2
    th, extras = O.thetas("AdaFace", g_unit, kernel, labels, norms=g_norm)
    header = _header("AdaFace", kernel)
    out, _ = _check("AdaFace", D, header, g_unit, labels, g_norm, th, O.cross_entropy(th, labels), O.target_cosine("AdaFace", g_unit, kernel, labels),
                    extras, tag="AdaFace literal loop")
    assert np.abs(out.margin_scaler.cpu().numpy()).max() <= 0.333 * 8 * O.U32 / O.EPS      # rounding noise: the adaptive margin is off


# ---- the loop body -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def backbone(lib):
    return A.ArcFace.from_synthetic("r18", 0).to(DEV)


def _images(seed, B=8):
    return torch.randn(B, 3, 112, 112, generator=torch.Generator().manual_seed(seed)).clamp(-1, 1)


@pytest.mark.parametrize("loss", ["CosFace", "ArcFace", "AdaFace"])
def test_step_metrics_and_validate(lib, backbone, loss):
    Cn = 33
    header = H.MarginHeader.from_synthetic(512, Cn, 3, loss).to(DEV)
    kernel = header.kernel.numpy()
    batches = [(_images(1), torch.arange(8) % Cn), (_images(2), (torch.arange(8) * 5 + 1) % Cn)]
    steps = []
    for images, labels in batches:
        got = H.step_metrics(backbone, header, images, labels)
        feats = got["features"]
        assert feats.dtype == torch.float32 and tuple(feats.shape) == (8, 512)
        f = feats.cpu()
        if loss == "AdaFace":                                 # the oracle takes the loop's own rows and norms, computed as the loop does
            norm = torch.norm(feats, 2, 1, True)
            rows, kw = torch.div(feats, norm).cpu().numpy(), dict(norms=norm.cpu().numpy())
        else:
            rows, kw = f.numpy(), {}
        th, _ = O.thetas(loss, rows, kernel, labels.numpy(), **kw)
        mean_want, per_want, _ = O.cross_entropy(th, labels.numpy())
        tb = O.target_bound(loss, 512, O.target_cosine(loss, rows, kernel, labels.numpy()), scaler_err=1e-9).max()
        assert abs(got["loss"] - mean_want) <= O.lse_bound(512, Cn) + tb
        unsure = O.ambiguous_rows(th, O.logit_bound(512))
        if not unsure.any():
            assert got["correct"] == int((O.argmax(th) == labels.numpy()).sum())
        assert got["acc"] == O.multi_class_acc([1] * got["correct"] + [0] * (8 - got["correct"]), [1] * 8)
        steps.append(got)
    val = H.validate(backbone, header, batches)
    if loss != "AdaFace" or header.t_alpha == 1.0:            # t_alpha = 1: the buffers do not carry over, so the steps repeat exactly
        assert val == {"loss": O.average_meter([s["loss"] for s in steps]), "top1": O.average_meter([s["acc"] for s in steps]), "steps": 2}


def test_step_metrics_end_to_end_against_the_fp32_backbone(lib, backbone):
    """The looser check through the backbone: its f16-operand embeddings against the fp32 restatement, with test_arcface_gpu.py's bounds."""
    images = _images(3, 4)
    got = backbone(images).cpu()
    ref = AO.forward(backbone._sd, "r18", images)
    cos = torch.nn.functional.cosine_similarity(got, ref, dim=1).min().item()
    rel = ((got - ref).norm(dim=1) / ref.norm(dim=1)).max().item()
    print(f"backbone embeddings against the fp32 restatement: min cosine {cos:.7f}, max relative L2 {rel:.3e}")
    assert cos >= ARC_BOUNDS[0] and rel <= ARC_BOUNDS[1]
    header = H.MarginHeader.from_synthetic(512, 33, 3, "CosFace").to(DEV)
    labels = torch.arange(4)
    step = H.step_metrics(backbone, header, images, labels)
    th, _ = O.thetas("CosFace", torch.nn.functional.normalize(ref).numpy(), header.kernel.numpy(), labels.numpy())
    # a relative L2 error r of an embedding moves each of its cosines by at most r, a logit by s r, the loss by twice that
    assert abs(step["loss"] - O.cross_entropy(th, labels.numpy())[0]) <= 2 * O.S * ARC_BOUNDS[1] + O.lse_bound(512, 33)


# ---- the wider class tiles, and column blocks of several tiles -----------------------------------------------------------------------
# The loss kernel has three class-tile widths (32, 64, 128: the widest that still gives 256 workgroups) and lets a column block take
# several tiles once there would be more than 2048 workgroups.  The shape matrix above reaches only the 32-wide tile with one tile per
# block; these cases reach the rest, and assert through the workspace query that they do.  (loss, B, C, D, tile width, tiles per block)
WIDE_CASES = [(loss, B, 4099, 130, width, 1) for B, width in ((512, 64), (1024, 128)) for loss in O.GPU_LOSSES]
WIDE_CASES += [("ArcFace", 1024, 32801, 7, 128, 2), ("CosFace", 1024, 32801, 130, 128, 2)]


@pytest.mark.parametrize("loss,B,Cn,D,width,per", WIDE_CASES, ids=lambda v: str(v))
def test_wide_tiles_and_multi_tile_blocks(lib, loss, B, Cn, D, width, per):
    """A duplicate of column `lo` sits at `hi`: in another 32-class sub-tile of the same tile (per = 1), or in the second tile of the same
    column block (per = 2), so the lower index has to survive the tile's own argmax or the carry across tiles.  Rows 0 and B - 1 point at
    that column; with per = 2 every row's running maximum, sum and argmax are carried from the first tile into the second."""
    lo, hi = (5, 40) if per == 1 else (5, 200)
    tiles, rt = -(-Cn // width), B // 128
    assert tiles * rt >= 256 and (width == 128 or -(-Cn // (2 * width)) * rt < 256)     # this width fills 256 CUs, the next wider would not
    assert (tiles * rt > 2048) == (per > 1)
    assert lo // width == hi // width if per == 1 else (lo // width != hi // width and lo // (width * per) == hi // (width * per))
    emb, kernel, labels, norms = O.inputs(loss, B, Cn, D, O.gpu_seed(loss, B, Cn, D))
    emb, kernel, labels = emb.copy(), kernel.copy(), labels.copy()
    kernel[:, hi] = kernel[:, lo]
    v = kernel[:, lo].astype(np.float64)
    v /= np.linalg.norm(v)
    for i in (0, B - 1):
        emb[i] = (v * (1.0 if loss == "AdaFace" else 30.0)).astype(np.float32)
        labels[i] = lo + 1
    th, extras = O.thetas(loss, emb, kernel, labels, **_kw(loss, norms))
    header = _header(loss, kernel)
    assert header.plan(B) == (rt, -(-tiles // per))           # the column blocks the library reports are those of this width and depth
    out, got_th = _check(loss, D, header, emb, labels, norms, th, O.cross_entropy(th, labels), O.target_cosine(loss, emb, kernel, labels), extras,
                         tag=f"{loss} {width}-wide x{per}")
    assert out.pred.cpu().numpy()[[0, B - 1]].tolist() == [lo, lo]
    plain = (labels != lo) & (labels != hi)                   # rows whose target is neither copy: the two columns are bit-equal
    assert (got_th[plain, lo] == got_th[plain, hi]).all()


# ---- bad rows ------------------------------------------------------------------------------------------------------------------------
def test_zero_and_non_finite_rows_are_refused(lib):
    """Upstream returns NaN for them.  The per-row launch marks such a row's target, the call raises, and a NaN norm leaves AdaFace's
    buffers as they were."""
    emb, kernel, labels, norms = O.inputs("AdaFace", 8, 33, 130, 3)
    for loss in ("CosFace", "AdaFace"):
        header = _header(loss, kernel)
        for bad in (0.0, float("inf"), float("nan")):
            if loss == "AdaFace" and bad == 0.0:
                continue                                      # AdaFace takes its rows as they are: a zero row is cosine 0, as upstream
            e = torch.from_numpy(emb.copy())
            e[3] = bad
            args = (e, torch.from_numpy(labels)) + ((torch.from_numpy(norms),) if loss == "AdaFace" else ())
            with pytest.raises(ValueError, match="zero or non-finite row"):
                header.loss(*args)
            with pytest.raises(ValueError, match="zero or non-finite row"):
                header(*((args[0], args[2], args[1]) if loss == "AdaFace" else args))
    header = _header("AdaFace", kernel)
    header.loss(torch.from_numpy(emb), torch.from_numpy(labels), norms=torch.from_numpy(norms))
    before = (header.batch_mean, header.batch_std)
    nrm = torch.from_numpy(norms.copy())
    nrm[2] = float("nan")
    with pytest.raises(ValueError, match="non-finite AdaFace norm"):
        header.loss(torch.from_numpy(emb), torch.from_numpy(labels), norms=nrm)
    assert (header.batch_mean, header.batch_std) == before


# ---- the unpacked route --------------------------------------------------------------------------------------------------------------
def test_an_unpacked_header_is_refused(lib):
    """idb_head_logits and idb_head_loss on a descriptor without the packed matrix are refused (there is no second, slower route);
    the Python header packs in .to() and refuses to run before it."""
    emb, kernel, labels, norms = O.inputs("CosFace", 4, 33, 130, 3)
    header = _header("CosFace", kernel)
    lib_, d, keep, need = header._desc(torch.from_numpy(emb), torch.from_numpy(labels), None)
    th = torch.empty((4, 33), dtype=torch.float32, device=DEV)
    rows = torch.empty((5, 4), dtype=torch.float64, device=DEV)
    d.wn = None
    stream = torch.cuda.current_stream().cuda_stream
    assert lib.idb_head_logits(C.byref(d), th.data_ptr(), rows.data_ptr(), keep[3].data_ptr(), need, stream) == -1
    assert b"not packed" in lib.idb_last_error()
    unpacked = H.MarginHeader(torch.from_numpy(kernel), "CosFace")
    with pytest.raises(_lib.IdbError, match="not on a device"):
        unpacked(torch.from_numpy(emb), torch.from_numpy(labels))
    got = unpacked.to(DEV)(torch.from_numpy(emb), torch.from_numpy(labels))
    assert torch.equal(got, header(torch.from_numpy(emb), torch.from_numpy(labels)))


def test_zz_report_measured_maxima():
    """Prints the largest error of every checked quantity over the tests above, with its derived bound (DESIGN.md 4.12 records them)."""
    for (what, loss, D), (err, bound) in sorted(MEASURED.items()):
        print(f"measured {what:22s} {loss:24s} D={D:4d}: {err:.3e} (bound {bound:.3e})")
    assert all(err <= bound for err, bound in MEASURED.values())
