"""The pair benchmark on the GPU: idb_frb_pair_dist and idb_frb_fold_counts against the float64 oracle (tests/frbench_oracle.py, itself
checked against recordings of the reference in test_frbench_cpu.py), evaluate from the fixture embeddings, and test / benchmark with a
synthetic r18 backbone.

Distance bound, u = 2^-53.  s = e0 + e1 and the squares of fp32 operands are exact in double.  A row's sum of squares takes d - 1
additions in any order, (d - 1) u relative; the square root halves that and adds u: the norm is within (d / 2 + 1) u relative, a
normalised component (one more division) within (d / 2 + 2) u of its magnitude.  With xa, xb the unit rows and diff = xa - xb, the error
of dist = |diff|^2 from the perturbed rows is at most 2 |diff| (|dxa| + |dxb|) <= 2 sqrt(dist) 2 (d / 2 + 2) u = (2 d + 8) u sqrt(dist)
(Cauchy-Schwarz, |xa| = |xb| = 1); the subtraction, the square and the d - 1 additions add (d + 2) u dist.  With dist <= 4 that is
(4 d + 16) u + (4 d + 8) u <= (8 d + 24) u for either side, the kernel or the oracle: (16 d + 48) u between them, 9.1e-13 at d = 512.
Norms: (d / 2 + 1) u relative per side, (d + 2) u between the two.  xnorm sums the 4P positive norms one at a time on either side,
(4P - 1) u relative each, and divides once: (d + 2 + 8P) u relative between the two."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import arcface_oracle as AO  # noqa: E402
import frbench_oracle as O  # noqa: E402

from faceposegenerator_amd import arcface as A  # noqa: E402
from faceposegenerator_amd import frbench as F  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -53
THR = O.thresholds()
ARC_BOUNDS = (0.9995, 5e-3)                                   # test_arcface_gpu.BOUNDS[torch.float16]: cosine, relative L2


def _embeddings(P, d, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((2 * P, d)).astype(np.float32) * 3, rng.standard_normal((2 * P, d)).astype(np.float32) * 3)


# ---- distances -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [512, 130, 7, 1])
@pytest.mark.parametrize("P", [1, 257, 3000])
def test_pair_distances_against_oracle(d, P):
    e0, e1 = _embeddings(P, d, 11 * d + P)
    dist, norms = F.pair_dist_norms(e0, e1)
    assert dist.dtype == torch.float64 and dist.is_cuda and tuple(dist.shape) == (P,) and tuple(norms.shape) == (2, 2 * P)
    want, want_xnorm = O.pair_dist(e0, e1)
    err = np.abs(dist.cpu().numpy() - want).max()
    want_norms = O.row_norms(e0, e1)
    nerr = (np.abs(norms.cpu().numpy() - want_norms) / want_norms).max()
    print(f"d={d} P={P}: dist max abs err {err:.3e} (bound {(16 * d + 48) * U:.3e}), norms max rel err {nerr:.3e} (bound {(d + 2) * U:.3e})")
    assert err <= (16 * d + 48) * U
    assert nerr <= (d + 2) * U
    dist2, xnorm = F.pair_distances(torch.from_numpy(e0).to(DEV), torch.from_numpy(e1).to(DEV))
    assert torch.equal(dist2, dist)
    assert abs(xnorm - want_xnorm) <= (d + 2 + 8 * P) * U * want_xnorm


@pytest.mark.parametrize("d", [512, 130, 7, 1])
def test_identical_rows_give_zero_and_a_zero_row_follows_sklearn(d):
    e0, e1 = _embeddings(40, d, d + 5)
    e0[1::4], e1[1::4] = e0[0::4], e1[0::4]                   # every second pair: two identical rows
    e0[6], e1[6] = 0, 0                                       # pair 3: a zero row against an ordinary one
    e1[10] = -e0[10]                                          # pair 5: image and mirror cancel, a zero sum of non-zero rows
    e0[16:18], e1[16:18] = 0, 0                               # pair 8: two zero rows
    dist, norms = F.pair_dist_norms(e0, e1)
    dist, norms = dist.cpu().numpy(), norms.cpu().numpy()
    assert (dist[0::2] == 0).all() and (d == 1 or (dist[1::2] > 0).all())               # d = 1: unit rows are +-1, dist is 0 or 4
    want, _ = O.pair_dist(e0, e1)
    assert np.abs(dist - want).max() <= (16 * d + 48) * U
    assert abs(dist[3] - 1.0) <= (16 * d + 48) * U and abs(dist[5] - 1.0) <= (16 * d + 48) * U      # |0 - unit row|^2
    assert norms[0, 6] == 0 and norms[1, 6] == 0 and norms[0, 10] > 0 and norms[0, 10] == norms[1, 10]


# ---- counts --------------------------------------------------------------------------------------------------------------------------
def _count_case(name):
    rng = np.random.default_rng(len(name))
    if name in O.TIE_CASES:
        dist, issame = O.tie_case(name)
        return dist, issame, THR, 10
    if name == "ties_mixed":
        dist = O.tie_distances(500, 9)
        return dist, rng.random(500) < 0.5, THR, 10
    n, nfolds, thr = {"603_10": (603, 10, THR), "6000_10_fine": (6000, 10, O.thresholds(0.001)), "7_3": (7, 3, THR), "10_10": (10, 10, THR),
                      "50_1": (50, 1, THR), "one_threshold": (300, 10, np.array([1.3])),
                      "repeated_thresholds": (300, 7, np.repeat(np.arange(0, 4, 0.25), 3))}[name]
    dist = rng.uniform(0, 4.2, n)
    if name == "repeated_thresholds":
        dist[::5] = rng.integers(0, 17, len(dist[::5])) * 0.25                              # on the repeated values themselves
    return dist, rng.random(n) < 0.5, thr, nfolds


COUNT_CASES = ("603_10", "6000_10_fine", "7_3", "10_10", "50_1", "one_threshold", "repeated_thresholds", "ties_same", "ties_diff", "ties_mixed")


@pytest.mark.parametrize("name", COUNT_CASES)
def test_fold_counts_equal_the_oracle(name):
    dist, issame, thr, nfolds = _count_case(name)
    got = F.fold_counts(torch.from_numpy(dist).to(DEV), issame, thr, nfolds)
    want = O.fold_counts(dist, issame, thr, nfolds)
    assert got[0].shape == (nfolds, len(thr), 2) and all(g.dtype == np.int64 for g in got)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    host = F.fold_counts(dist, issame.tolist(), thr, nfolds)                                # host inputs are uploaded
    assert np.array_equal(host[0], want[0])
    if len(thr) > 400:                                        # the oracle's search over 4000 thresholds takes seconds
        return
    stats, ref = F.stats_from_counts(*got, thr), O.roc(dist, issame, thr, nfolds)
    for key in ("tpr", "fpr", "accuracy", "best_threshold"):
        assert np.array_equal(stats[key], ref[key]), key


def test_two_runs_are_bit_identical():
    e0, e1 = _embeddings(3000, 512, 77)
    a, b = F.pair_dist_norms(e0, e1), F.pair_dist_norms(e0, e1)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    issame = np.random.default_rng(3).random(3000) < 0.5
    c, d = F.fold_counts(a[0], issame, THR), F.fold_counts(a[0], issame, THR)
    assert c[0].tobytes() == d[0].tobytes()


# ---- evaluate ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,d,nfolds", O.CASES)
def test_evaluate_from_fixture_embeddings(P, d, nfolds):
    e0, e1, issame = O.pair_embeddings(P, d, seed=P + d)
    want_dist, want_xnorm = O.pair_dist(e0, e1)
    # a condition, not a tolerance: every oracle distance is further from every threshold than the kernel can be from the oracle, so
    # the GPU's distances fall on the same side of every threshold and the statistics must be the oracle's to the bit
    gap = O.threshold_gap(want_dist, THR)
    assert gap > 1e-9 > (16 * d + 48) * U
    out = F.evaluate(e0, e1, issame, nfolds)
    got_dist = out["dist"].cpu().numpy()
    assert np.abs(got_dist - want_dist).max() <= (16 * d + 48) * U
    assert abs(out["xnorm"] - want_xnorm) <= (d + 2 + 8 * P) * U * want_xnorm
    want = O.roc(want_dist, issame, THR, nfolds)
    for key in ("tpr", "fpr", "accuracy", "best_threshold"):
        assert np.array_equal(out[key], want[key]), key
    assert (out["acc"], out["std"]) == (want["acc"], want["std"])
    assert np.array_equal(out["thresholds"], THR)
    assert np.array_equal(out["genuine"], got_dist[issame]) and np.array_equal(out["impostor"], got_dist[~issame])


# ---- the backbone --------------------------------------------------------------------------------------------------------------------
def _crops(P, seed):
    g = torch.Generator().manual_seed(seed)
    base = torch.randint(0, 256, (2 * P, 112, 112, 3), generator=g, dtype=torch.uint8)
    issame = (torch.rand(P, generator=g) < 0.5).numpy()
    noise = torch.randint(-40, 41, (P, 112, 112, 3), generator=g)
    same = torch.from_numpy(issame)
    base[1::2][same] = (base[0::2][same].int() + noise[same]).clamp(0, 255).to(torch.uint8)     # "same": a noisy copy
    return base, issame


@pytest.fixture(scope="module")
def backbone(lib):
    return A.ArcFace.from_synthetic("r18", 0).to(DEV)


def test_test_with_a_synthetic_backbone(backbone):
    crops, issame = _crops(24, 4)
    acc1, std1, acc2, std2, xnorm, embs = F.test(crops, issame, backbone, nfolds=10)
    assert (acc1, std1) == (0.0, 0.0) and len(embs) == 2
    # one chunk on both sides (48 crops, chunk 256): the same launches, so the same bits
    assert torch.equal(embs[0], backbone.embed_u8(crops)) and torch.equal(embs[1], backbone.embed_u8(crops.flip(2)))
    idx = torch.tensor([0, 1, 17, 47])
    x = ((crops.flip(2)[idx].float() / 255 - 0.5) / 0.5).permute(0, 3, 1, 2).contiguous()
    ref = AO.forward(backbone._sd, "r18", x)
    got = embs[1][idx.to(DEV)].cpu()
    cos = torch.nn.functional.cosine_similarity(got, ref, dim=1).min().item()
    rel = ((got - ref).norm(dim=1) / ref.norm(dim=1)).max().item()
    print(f"mirrored embeddings against the fp32 restatement: min cosine {cos:.7f}, max relative L2 {rel:.3e}")
    assert cos >= ARC_BOUNDS[0] and rel <= ARC_BOUNDS[1]
    # the statistics are the oracle's statistics of the GPU's own embeddings
    e0, e1 = embs[0].cpu().numpy(), embs[1].cpu().numpy()
    dist, want_xnorm = O.pair_dist(e0, e1)
    assert O.threshold_gap(dist, THR) > 1e-9
    want = O.roc(dist, issame, THR, 10)
    assert (acc2, std2) == (want["acc"], want["std"])
    assert abs(xnorm - want_xnorm) <= (512 + 2 + 8 * 24) * U * want_xnorm


def test_benchmark_record(backbone):
    sets = {"lfw": _crops(12, 5), "agedb_30": _crops(10, 6)}
    rec = F.benchmark(backbone, sets)
    assert list(rec) == ["lfw", "agedb_30", "Average"] and all(len(v) == 1 for v in rec.values())
    accs = [F.test(*sets[k], backbone)[2] for k in ("lfw", "agedb_30")]
    assert [rec["lfw"][0], rec["agedb_30"][0]] == accs
    assert rec["Average"][0] == sum([a / 2 for a in accs])
