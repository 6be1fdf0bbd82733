"""CPU checks for the feature metrics: tests/metrics_oracle.py (float64) against known answers and against sklearn / torch / scipy, the
conditions on the test fixture, the host metrics of faceposegenerator_amd/metrics.py (fd, vendi_per_class), every ValueError path and
the argument validation of the idb_pair_* entries (no GPU here)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import metrics_oracle as O  # noqa: E402

from faceposegenerator_amd import _lib  # noqa: E402
from faceposegenerator_amd import metrics as M  # noqa: E402

SHAPES = [(200, 168, 72), (333, 257, 96), (520, 400, 384)]


# ---- oracle against known answers ----------------------------------------------------------------------------------------------------
def test_oracle_on_hand_computed_points():
    # real on a line at 0, 1, 3, 7; nearest_k = 1 -> radii^2 = 1, 1, 4, 16.  gen at 0.5, 2.5, 20, 6.5.
    real = np.array([[0.0], [1.0], [3.0], [7.0]])
    gen = np.array([[0.5], [2.5], [20.0], [6.5]])
    assert O.knn_radii(real, 2).tolist() == [1.0, 1.0, 4.0, 16.0]
    assert O.knn_radii(gen, 2).tolist() == [4.0, 4.0, 13.5 ** 2, 16.0]
    # gen 0.5 lies in the spheres of 0 and 1 (0.25 < 1), not of 3 (6.25 > 4), not of 7; gen 2.5 in 3's only (d2 to 1 is 2.25 > 1);
    # gen 20 in none (169 > 16); gen 6.5 in 7's only (d2 to 3 is 12.25 > 4)
    p = O.Prdc(real, gen, 1)
    assert p.in_sphere.sum(axis=0).tolist() == [2, 1, 0, 1]
    s = p.scores()
    assert s["precision"] == 0.75 and s["density"] == 1.0
    # real 0: d2 to gen 0.5 = 0.25 < 4; real 1: 0.25 < 4; real 3: 0.25 < 4 (gen 2.5); real 7: 0.25 < 16 (gen 6.5)
    assert s["recall"] == 1.0
    # row minima 0.25 each against radii 1, 1, 4, 16
    assert s["coverage"] == 1.0
    # authenticity: nearest real of each gen = index 0 (tie with 1, lowest index), 2, 3, 3; that real's nearest other real at d2 = 1, 4, 16,
    # 16; authentic when that is below the gen's own distance 0.25, 0.25, 169, 0.25 -> only gen 20
    a = O.Auth(real, gen)
    assert a.rg.arg.tolist() == [0, 2, 3, 3] and a.rr.min.tolist() == [1.0, 1.0, 4.0, 16.0]
    assert a.authentic.tolist() == [False, False, True, False] and a.pct() == 25.0
    # the tie between real 0 and real 1 for gen 0.5 is exact: float64 reports it as not decided
    assert a.rg.decided.tolist() == [False, True, True, True]


def test_oracle_identical_and_disjoint_sets():
    real, _ = O.fixture(150, 10, 24)
    s = O.prdc(real, real.copy(), 5)
    assert s["precision"] == 1.0 and s["recall"] == 1.0 and s["coverage"] == 1.0
    rng = np.random.default_rng(0)
    idx = [(rng.choice(150, 60, replace=False), rng.choice(150, 60, replace=False)) for _ in range(40)]
    vals = O.kd(real, real, [i for i, _ in idx], [j for _, j in idx])
    assert vals.min() < 0 < vals.max()                # the unbiased estimate scatters around 0 and is not exactly 0
    assert abs(vals.mean()) < 3 * vals.std()
    far = real + 1000.0
    s = O.prdc(real, far, 5)
    assert s["precision"] == 0.0 and s["recall"] == 0.0 and s["coverage"] == 0.0 and s["density"] == 0.0
    assert O.authpct(real, far) == 100.0


def test_oracle_against_sklearn_torch_scipy():
    from scipy.spatial.distance import cdist
    from sklearn.metrics import pairwise_distances
    from sklearn.metrics.pairwise import polynomial_kernel
    real, gen = O.fixture(90, 70, 40)
    d = O.dist2(real, gen)
    r64, g64 = real.astype(np.float64), gen.astype(np.float64)
    # these form the distance by the norm expansion, so agreement is to its round-off in float64: 1e-9 of |a|^2 + |b|^2
    bound = 1e-9 * ((r64 ** 2).sum(1)[:, None] + (g64 ** 2).sum(1)[None, :])
    assert (np.abs(pairwise_distances(r64, g64) ** 2 - d) <= bound).all()
    assert (np.abs(torch.cdist(torch.from_numpy(r64), torch.from_numpy(g64)).numpy() ** 2 - d) <= bound).all()
    assert (np.abs(cdist(r64, g64, "sqeuclidean") - d) <= bound).all()
    kth = np.sort(pairwise_distances(r64, r64) ** 2, axis=1)[:, 5]
    assert np.allclose(O.knn_radii(real, 6), kth, rtol=0, atol=bound.max())
    gamma = 1.0 / 40
    kxx, kyy, kxy = polynomial_kernel(r64[:70], degree=3, gamma=gamma, coef0=1), polynomial_kernel(g64, degree=3, gamma=gamma, coef0=1), \
        polynomial_kernel(r64[:70], g64, degree=3, gamma=gamma, coef0=1)
    sums, abs_sums = O.poly_sums(r64[:70], g64, gamma)
    want = np.array([kxx.sum() - np.trace(kxx), kyy.sum() - np.trace(kyy), kxy.sum()])
    assert np.allclose(sums, want, rtol=1e-12)
    assert np.allclose(abs_sums, want, rtol=1e-12)    # every kernel value of these features is positive
    m = 70
    want_mmd = (want[0] + want[1]) / (m * (m - 1)) - 2 * want[2] / (m * m)
    assert np.isclose(O.mmd2(sums, m), want_mmd, rtol=1e-12)
    assert np.isclose(M.mmd2_from_sums(sums, m), want_mmd, rtol=1e-12)


# ---- the fixture ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_fixture_is_decided_and_not_degenerate(shape):
    real, gen = O.fixture(*shape)
    assert abs(float(real.mean()) - 2.0) < 0.5        # the mean is far from 0, as in real features
    p = O.Prdc(real, gen, 5)
    a = O.Auth(real, gen)
    assert p.undecided_share() <= O.UNDECIDED_CAP and a.und.mean() <= O.UNDECIDED_CAP
    assert p.undecided_share() == 0 and a.und.sum() == 0 and a.rr.decided.all() and a.rg.decided.all()
    values = dict(p.scores(), authentic=a.pct() / 100.0)
    for name, v in values.items():
        assert 0.05 < v < 0.98, (name, v)
    for k in (1, 7):                                  # the other neighbour counts of the GPU tests stay under the cap
        assert O.Prdc(real, gen, k).undecided_share() <= O.UNDECIDED_CAP


# ---- host metrics ------------------------------------------------------------------------------------------------------------------
def test_fd_matches_eigenvalue_form():
    rng = np.random.default_rng(2)
    a = rng.normal(size=(400, 24)) @ rng.normal(size=(24, 24)) + 1.0
    b = rng.normal(size=(300, 24)) @ rng.normal(size=(24, 24)) - 0.5
    c1, c2 = np.cov(a, rowvar=False), np.cov(b, rowvar=False)
    eig = np.linalg.eigvals(c1 @ c2)
    want = ((a.mean(0) - b.mean(0)) ** 2).sum() + np.trace(c1) + np.trace(c2) - 2 * np.sqrt(eig.real.clip(min=0)).sum()
    assert np.isclose(M.fd(a.astype(np.float32).astype(np.float64), b), want, rtol=1e-4)
    assert np.isclose(M.fd(a, b), want, rtol=1e-8)
    assert abs(M.fd(a, a.copy())) < 1e-6 * np.trace(c1)
    assert np.isclose(M.fd(torch.from_numpy(a), torch.from_numpy(b)), want, rtol=1e-8)


def test_vendi_per_class_on_orthonormal_rows():
    q, _ = np.linalg.qr(np.random.default_rng(3).normal(size=(16, 16)))
    rows = np.concatenate([3.0 * q[:5], np.repeat(q[5:6], 4, axis=0), q[6:9] * np.array([[1.0], [2.0], [0.5]])])
    labels = np.array([0] * 5 + [1] * 4 + [2] * 3)
    v = M.vendi_per_class(rows, labels)
    assert np.allclose(v, [5.0, 1.0, 3.0], rtol=1e-9)   # n orthogonal rows (any length: rows are normalised) -> n; identical rows -> 1
    with pytest.raises(ValueError):
        M.vendi_per_class(rows, labels[:-1])
    with pytest.raises(ValueError):
        M.vendi_per_class(rows, labels * 2)              # classes 0, 2, 4: class 1 of 3 is empty


def test_compute_scores_keys_and_host_only_path():
    real, gen = O.fixture(60, 50, 12)
    labels = np.arange(50) % 4
    s = M.compute_scores(real, gen, labels, metrics=("fd", "vendi"))     # the host metrics alone never touch the GPU
    assert set(s) == {"fd", "mean vendi per class", "std vendi per class"}
    assert s["fd"] == M.fd(real, gen)
    per_class = M.vendi_per_class(gen, labels)
    assert s["mean vendi per class"] == per_class.mean() and s["std vendi per class"] == per_class.std()
    assert set(M.SCORE_KEYS) == {"fd", "kd_value", "kd_variance", "precision", "recall", "density", "coverage", "mean vendi per class",
                                 "std vendi per class", "authpct"}


def test_value_errors_before_any_gpu_work():
    real, gen = O.fixture(20, 18, 12)
    bad = real.copy()
    bad[3, 4] = np.nan
    inf = gen.copy()
    inf[0, 0] = np.inf
    for fn in (M.prdc, M.authpct, M.kd, M.fd, M.compute_scores):
        with pytest.raises(ValueError, match="D ="):
            fn(real, gen[:, :11])
        with pytest.raises(ValueError, match="non-finite"):
            fn(bad, gen)
        with pytest.raises(ValueError, match="non-finite"):
            fn(real, inf)
        with pytest.raises(ValueError, match=r"\[N, D\]"):
            fn(real[0], gen)
    with pytest.raises(ValueError, match="nearest_k"):
        M.prdc(real[:5], gen, nearest_k=5)               # N <= nearest_k
    with pytest.raises(ValueError, match="nearest_k"):
        M.prdc(real, gen[:3], nearest_k=3)
    with pytest.raises(ValueError, match="> 8"):
        M.prdc(real, gen, nearest_k=8)                   # nearest_k + 1 > 8
    with pytest.raises(ValueError, match="nearest_k"):
        M.prdc(real, gen, nearest_k=0)
    with pytest.raises(ValueError, match="> 8"):
        M.compute_scores(real, gen, metrics=("prdc",), nearest_k=8)
    with pytest.raises(ValueError, match="nearest_k"):
        M.compute_scores(real, gen, metrics=("prdc",), nearest_k=5, reduced_n=4)
    with pytest.raises(ValueError, match="labels"):
        M.compute_scores(real, gen)                      # vendi requested without labels
    with pytest.raises(ValueError, match="unknown metric"):
        M.compute_scores(real, gen, metrics=("fls",))
    with pytest.raises(ValueError):
        M.authpct(real[:1], gen)
    with pytest.raises(ValueError):
        M.kd(real, gen, n_subsets=0)
    with pytest.raises(ValueError, match="out of range"):
        M.kd(real, gen, subsets=(np.array([[0, 20]]), np.array([[0, 1]])))
    with pytest.raises(ValueError):
        M.prdc(real.astype(np.int32), gen)


# ---- the C ABI without a GPU: every entry validates before any HIP call ------------------------------------------------------------
def test_pair_entries_reject_bad_arguments_without_gpu(lib):
    p = 0x1000                                           # never dereferenced: validation comes first
    big = 1 << 20

    def refused(rc, word):
        assert rc == -1 and word in lib.idb_last_error(), lib.idb_last_error()

    refused(lib.idb_pair_dist2(p, 0, p, 4, 8, p, p, p, big, None), b"na, nb")
    refused(lib.idb_pair_dist2(p, 4, p, 4, 0, p, p, p, big, None), b"d in")
    refused(lib.idb_pair_dist2(None, 4, p, 4, 8, p, p, p, big, None), b"null")
    refused(lib.idb_pair_dist2(p, 4, p, 4, 8, None, p, None, big, None), b"null")
    refused(lib.idb_pair_dist2(p, 4, p, 4, 8, p, p, p, 16, None), b"workspace")
    refused(lib.idb_pair_dist2(p, 4, p, 4, 8, p, p, p + 4, big, None), b"workspace")
    refused(lib.idb_pair_knn_radii(p, 100, 8, p, 9, p, p, 1 << 24, None), b"kth")
    refused(lib.idb_pair_knn_radii(p, 100, 8, p, 0, p, p, 1 << 24, None), b"kth")
    refused(lib.idb_pair_knn_radii(p, 3, 8, p, 4, p, p, 1 << 24, None), b"kth")
    refused(lib.idb_pair_knn_radii(p, 100, 8, p, 6, None, p, 1 << 24, None), b"null")
    refused(lib.idb_pair_knn_radii(p, 100, 8, p, 6, p, p, 64, None), b"workspace")
    refused(lib.idb_pair_prdc_counts(p, 10, p, 0, 8, p, p, p, p, p, p, p, big, None), b"nr, ng")
    refused(lib.idb_pair_prdc_counts(p, 10, p, 10, 8, p, None, p, p, p, p, p, big, None), b"null")
    refused(lib.idb_pair_prdc_counts(p, 10, p, 10, 8, p, p, p, p, p, p, p, 0, None), b"workspace")
    refused(lib.idb_pair_nearest(p, 1, p, 1, 8, p, 1, p, p, p, big, None), b"exclude_diag")
    refused(lib.idb_pair_nearest(p, 4, p, 4, 1 << 17, p, 0, p, p, p, big, None), b"d in")
    refused(lib.idb_pair_nearest(p, 4, p, 4, 8, p, 0, p, None, p, big, None), b"null")
    refused(lib.idb_pair_nearest(p, 4, p, 4, 8, p, 0, p, p, p, 8, None), b"workspace")
    refused(lib.idb_pair_poly_sums(p, 10, p, 10, 8, p, p, 0, 5, 0.1, 1.0, p, p, big, None), b"subsets")
    refused(lib.idb_pair_poly_sums(p, 10, p, 10, 8, p, p, 2, 11, 0.1, 1.0, p, p, big, None), b"subset size")
    refused(lib.idb_pair_poly_sums(p, 10, p, 10, 8, p, p, 2, 1, 0.1, 1.0, p, p, big, None), b"subset size")
    refused(lib.idb_pair_poly_sums(p, 10, p, 10, 8, p, None, 2, 5, 0.1, 1.0, p, p, big, None), b"null")
    refused(lib.idb_pair_poly_sums(p, 10, p, 10, 8, p, p, 2, 5, 0.1, 1.0, p, p, 4, None), b"workspace")


def test_pair_workspace_query(lib):
    q = lib.idb_pair_workspace_bytes
    assert q(_lib.IDB_PAIR_DIST2, 200, 168, 0) >= 4 * (200 + 168)
    # k nearest: norms and 8 candidates from each half-wave of up to 8 workgroups per query
    assert 4 * 200 + 2 * 2 * 200 * 8 * 4 <= q(_lib.IDB_PAIR_KNN, 200, 0, 0) <= 4 * 200 + 2 * 2 * 200 * 8 * 4 + 512
    assert q(_lib.IDB_PAIR_KNN, 10000, 0, 0) < 6 << 20                  # a few megabytes at the evaluation's size, not N x N
    assert q(_lib.IDB_PAIR_NEAREST, 10000, 10000, 0) < 2 << 20
    assert q(_lib.IDB_PAIR_POLY, 1000, 0, 100) == 3 * 100 * 8 * 8 * 4
    for args in ((9, 10, 10, 0), (-1, 10, 10, 0), (_lib.IDB_PAIR_DIST2, 0, 10, 0), (_lib.IDB_PAIR_PRDC, 10, 0, 0),
                 (_lib.IDB_PAIR_POLY, 100, 0, 0), (_lib.IDB_PAIR_KNN, (1 << 22) + 1, 0, 0)):
        assert q(*args) == 0, args
