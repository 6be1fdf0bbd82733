"""CR-FIQA on the MI355X: the OpenCV-linear resize bit for bit against the integer restatement of tests/fiqa_oracle.py, the
double-accumulated tail against float64, the network (ArcFace body + quality head) against the restatement, and the reference's
``get_batch_feature`` / score-file path end to end.

Bounds.  Features: the ArcFace bounds of tests/test_arcface_gpu.py (set there on CPU from the emulated-autocast restatement before any
GPU run): f16 cosine >= 0.9995 and relative L2 <= 5e-3; bf16 cosine >= 0.995 and relative L2 <= 4e-2.  Tail: emb_norm lies in [-1, 1]
and is rounded once, so |got - ref| <= 2^-23 per element; qs is a sum of products that are exact in double, a 512-term double sum that
errs by far less than 2^-40 sum |e_i w_i|, and one rounding to fp32: |qs - ref| <= 2^-24 |ref| + 2^-40 sum |e_i w_i|.  Network qs: by
Cauchy-Schwarz on the embedding error, |qs - ref| <= rel ||qs.weight|| ||features_ref|| with rel the relative-L2 bound above, plus the
tail bound.  The observed deviations are printed; DESIGN.md records them."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fiqa_oracle as Q  # noqa: E402

from faceposegenerator_amd import fiqa as F  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BOUNDS = {torch.float16: (0.9995, 5e-3), torch.bfloat16: (0.995, 4e-2)}      # cosine, relative L2 (tests/test_arcface_gpu.py BOUNDS)
SHAPES = [(7, 7, 7, 7), (5, 9, 3, 4), (8, 8, 4, 4), (1, 1, 3, 3), (13, 11, 112, 112), (200, 300, 112, 112), (512, 512, 112, 112)]


def _images(H, W, B=2, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (B, H, W, 3), dtype=np.uint8)


# ---- resize -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,dh,dw", SHAPES)
def test_resize_is_bit_equal_to_the_oracle(lib, H, W, dh, dw):
    x = _images(H, W)
    ref = Q.resize(x, dh, dw)
    got = F.resize_linear_u8(x, dh, dw, device=DEV)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (2, dh, dw, 3) and got.is_cuda
    assert np.array_equal(got.cpu().numpy(), ref)
    swapped = F.resize_linear_u8(torch.from_numpy(x).to(DEV), dh, dw, swap_rb=True).cpu().numpy()
    assert np.array_equal(swapped, ref[..., ::-1])
    assert np.array_equal(swapped, got.cpu().numpy()[..., ::-1])


def test_resize_batch_equals_single_images(lib):
    x = _images(13, 11, B=3, seed=1)
    full = F.resize_linear_u8(x, 112, 112, swap_rb=True, device=DEV)
    for b in range(3):
        assert torch.equal(F.resize_linear_u8(x[b:b + 1], 112, 112, swap_rb=True, device=DEV)[0], full[b])
    x = _images(8, 8, B=3, seed=2)                                            # the box kernel
    full = F.resize_linear_u8(x, 4, 4, device=DEV)
    for b in range(3):
        assert torch.equal(F.resize_linear_u8(x[b:b + 1], 4, 4, device=DEV)[0], full[b])
    with pytest.raises(ValueError):
        F.resize_linear_u8(np.zeros((1, 4, 4, 4), np.uint8), 2, 2, device=DEV)
    with pytest.raises(ValueError):
        F.resize_linear_u8(np.zeros((1, 4, 4, 3), np.float32), 2, 2, device=DEV)


# ---- tail -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def r18():
    return F.FaceQuality.from_synthetic("r18", 0, torch.float16).to(DEV)


def _tail_bound(qs_ref, sum_abs):
    return 2.0 ** -24 * np.abs(qs_ref) + 2.0 ** -40 * sum_abs


def test_tail_against_float64(r18):
    g = torch.Generator().manual_seed(3)
    emb = torch.cat([3.0 * torch.randn(5, 512, generator=g), torch.zeros(1, 512)])
    w, b = r18._sd["qs.weight"].numpy().reshape(-1), r18._sd["qs.bias"].item()
    nrm_t, qs_t = r18.tail(emb)
    assert tuple(nrm_t.shape) == (6, 512) and tuple(qs_t.shape) == (6, 1) and nrm_t.dtype == qs_t.dtype == torch.float32
    qs_ref, nrm_ref, sum_abs = Q.tail(emb.numpy(), w, b)
    nrm, qs = nrm_t.cpu().numpy().astype(np.float64), qs_t.cpu().numpy().astype(np.float64).reshape(-1)
    assert not nrm[5].any() and qs[5] == np.float64(np.float32(b))                  # the zero row stays zero; its score is the bias
    e_n = np.abs(nrm - nrm_ref).max()
    e_q = np.abs(qs - qs_ref)
    bound = _tail_bound(qs_ref, sum_abs)
    print(f"tail: max |emb_norm - ref| = {e_n:.3e} (bound {2.0 ** -23:.3e}); max |qs - ref| / bound = {(e_q / bound).max():.3f}, "
          f"max |qs - ref| = {e_q.max():.3e}")
    assert e_n <= 2.0 ** -23
    assert (e_q <= bound).all(), (e_q, bound)
    nrm2, qs2 = r18.tail(emb)
    assert torch.equal(nrm2, nrm_t) and torch.equal(qs2, qs_t)


# ---- network ----------------------------------------------------------------------------------------------------------------------
def _faces(B, seed=1):
    return torch.rand(B, 3, 112, 112, generator=torch.Generator().manual_seed(seed)) * 2 - 1


_SD = {}


def _weights(arch):
    if arch not in _SD:
        _SD[arch] = F.synth_weights(arch, 0)
    return _SD[arch]


@pytest.mark.parametrize("arch,dt,B", [("r18", torch.float16, 1), ("r18", torch.float16, 3), ("r18", torch.bfloat16, 1),
                                       ("r18", torch.bfloat16, 3), ("r50", torch.float16, 4)])
def test_network_matches_the_restatement(arch, dt, B):
    sd = _weights(arch)
    m = F.FaceQuality.from_state_dict(sd, arch, dt).to(DEV)
    x = _faces(B)
    feat, qs = m(x)
    assert tuple(feat.shape) == (B, 512) and tuple(qs.shape) == (B, 1) and feat.dtype == qs.dtype == torch.float32
    feat, qs = feat.cpu().double(), qs.cpu().double().reshape(-1)
    assert torch.isfinite(feat).all() and torch.isfinite(qs).all()
    feat_ref, qs_ref = Q.forward(sd, arch, x)
    qs_ref = qs_ref.reshape(-1)
    cmin, rel_max = BOUNDS[dt]
    cos = torch.nn.functional.cosine_similarity(feat, feat_ref, dim=1).min().item()
    rel = ((feat - feat_ref).norm(dim=1) / feat_ref.norm(dim=1)).max().item()
    w = sd["qs.weight"].double().reshape(-1)
    # the tail's own error, at the embeddings the tail was given
    qs_exact, _, sum_abs = Q.tail(feat.numpy(), w.numpy(), sd["qs.bias"].item())
    bound = rel_max * w.norm().item() * feat_ref.norm(dim=1).numpy() + _tail_bound(qs_exact, sum_abs)
    dq = (qs - qs_ref).abs().numpy()
    print(f"{arch} {dt} B={B}: min cosine {cos:.7f}, max relative L2 {rel:.3e}; qs ref {qs_ref.numpy().round(4).tolist()}, "
          f"max |qs - ref| {dq.max():.3e} (bound {bound.min():.3e})")
    assert cos >= cmin and rel <= rel_max, (cos, rel)
    assert (dq <= bound).all(), (dq, bound)


# ---- end to end -------------------------------------------------------------------------------------------------------------------
def test_get_batch_feature_is_resize_embed_tail(r18):
    imgs = _images(40, 56, B=3, seed=5)                                              # RGB
    feat, qs = r18.get_batch_feature(imgs)
    assert tuple(feat.shape) == (3, 512) and tuple(qs.shape) == (3, 1) and feat.is_cuda
    crops = np.ascontiguousarray(Q.resize(imgs, 112, 112)[..., ::-1])                # BGR, as cv2.imread + cv2.resize deliver
    nrm, q = r18.tail(r18.embed_u8(crops))
    assert torch.equal(feat, nrm) and torch.equal(qs, q)
    assert ((feat.double().norm(dim=1) - 1).abs() <= 2.0 ** -22).all()
    x = ((torch.from_numpy(crops).float() / 255 - 0.5) / 0.5).permute(0, 3, 1, 2).contiguous()
    raw, q2 = r18(x)
    assert torch.equal(q2, qs)
    assert torch.equal(r18.tail(raw)[0], feat)
    assert torch.equal(r18.get_batch_feature(torch.from_numpy(imgs).to(DEV))[1], qs)          # a device batch
    chunked = F.FaceQuality.from_state_dict(r18._sd, "r18", torch.float16).to(DEV)
    chunked.chunk = 2
    f2, q3 = chunked.get_batch_feature(imgs)                 # chunks of 2 + 1 plan other tiles than 3 images: same values, another order
    assert tuple(f2.shape) == (3, 512) and tuple(q3.shape) == (3, 1)
    assert ((f2 - feat).norm(dim=1) / feat.norm(dim=1)).max().item() < 2e-3
    with pytest.raises(ValueError):
        r18.get_batch_feature(np.zeros((1, 8, 8, 3), np.float32))


def test_score_folder(r18, tmp_path):
    from PIL import Image
    folder = tmp_path / "set"
    folder.mkdir()
    imgs = _images(24, 20, B=12, seed=6)
    for i in range(12):
        Image.fromarray(imgs[i]).save(str(folder / f"{i}.png"))
    out = str(tmp_path / "scores.txt")
    summary = F.score_folder(r18, str(folder), out, n=5, seed=7, batch=4)
    want_paths = F.sample_paths(F.list_images(str(folder)), 5, 7)
    assert len(want_paths) == 5
    idx = [int(os.path.basename(p).split(".")[0]) for p in want_paths]
    lines = open(out).read().split("\n")
    assert lines[-1] == "" and len(lines) == 6
    # score_folder ran batches of 4 + 1 images; a batch of another size may plan other tiles, so the scores are recomputed in the same batches
    q = np.concatenate([r18.get_batch_feature(imgs[idx[:4]])[1].cpu().numpy(), r18.get_batch_feature(imgs[idx[4:]])[1].cpu().numpy()])
    assert q.dtype == np.float32
    assert lines[:5] == [want_paths[k] + " " + str(q[k, 0]) for k in range(5)]
    assert summary == F.quality_summary(F.read_scores(out))
    assert set(summary) == {"mean", "std"} and np.isfinite(summary["mean"]) and np.isfinite(summary["std"])
