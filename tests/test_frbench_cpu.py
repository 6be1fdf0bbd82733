"""The pair benchmark without a GPU: the float64 oracle (tests/frbench_oracle.py) against outputs recorded from the reference's own
embedding_preprocessing, calculate_roc, calculate_accuracy and LFold / KFold (tests/golden/frbench_*), the module's host arithmetic
(stats_from_counts, kfold_bounds) against the same recordings, load_bin, every refusal, and the preconditions of the fixtures.

Distance bound against the recording: both sides are double computations of the same expression in different summation orders, so
the bound of test_frbench_gpu.py applies, (16 d + 48) 2^-53, and for xnorm its (d + 2 + 8P) 2^-53 relative (the 4P norms, each within
(d + 2) 2^-53 relative between the two sides, summed one at a time on either side)."""
import io
import json
import os
import pickle

import numpy as np
import pytest
import torch

import frbench_oracle as O
from faceposegenerator_amd import frbench as F

HERE = os.path.dirname(os.path.abspath(__file__))
REF = np.load(os.path.join(HERE, "golden", "frbench_reference.npz"))
KFOLD = json.load(open(os.path.join(HERE, "golden", "frbench_kfold.json")))["fold_sizes"]
U = 2.0 ** -53
THR = O.thresholds()
IDS = [O.case_name(*c) for c in O.CASES]


@pytest.fixture(scope="module")
def cases():
    out = {}
    for (P, d, nfolds) in O.CASES:
        e0, e1, issame = O.pair_embeddings(P, d, seed=P + d)
        dist, xnorm = O.pair_dist(e0, e1)
        out[O.case_name(P, d, nfolds)] = dict(P=P, d=d, nfolds=nfolds, issame=issame, dist=dist, xnorm=xnorm, roc=O.roc(dist, issame, THR, nfolds))
    return out


@pytest.mark.parametrize("name", IDS)
def test_oracle_matches_the_recorded_reference(cases, name):
    c = cases[name]
    for key in ("tpr", "fpr", "accuracy"):
        assert np.array_equal(c["roc"][key], REF[f"{name}_{key}"]), key
    err = np.abs(c["dist"] - REF[name + "_dist"]).max()
    assert err <= (16 * c["d"] + 48) * U, err
    assert abs(c["xnorm"] - float(REF[name + "_xnorm"])) <= (c["d"] + 2 + 8 * c["P"]) * U * c["xnorm"]


@pytest.mark.parametrize("name", IDS)
def test_fixture_preconditions(cases, name):
    """An accuracy of 1.0 everywhere would test nothing about the threshold search, and a distance on a threshold would make the
    statistics depend on the last bits of the distance."""
    c = cases[name]
    assert 0.70 < c["roc"]["acc"] < 0.98
    if c["nfolds"] > 1:
        assert len(set(c["roc"]["accuracy"].tolist())) > 1
    assert 0 < c["issame"].sum() < len(c["issame"])
    assert O.threshold_gap(c["dist"], THR) > 1e-9
    assert O.threshold_gap(REF[name + "_dist"], THR) > 1e-9


@pytest.mark.parametrize("name", IDS)
def test_stats_from_counts_equal_the_recorded_reference(cases, name):
    """The module's host arithmetic, fed the oracle's counts: bit-equal to calculate_roc."""
    c = cases[name]
    got = F.stats_from_counts(*O.fold_counts(c["dist"], c["issame"], THR, c["nfolds"]), THR)
    for key in ("tpr", "fpr", "accuracy"):
        assert np.array_equal(got[key], REF[f"{name}_{key}"]), key
    want = c["roc"]
    assert np.array_equal(got["best_threshold"], want["best_threshold"])
    assert (got["acc"], got["std"]) == (want["acc"], want["std"]) == (float(np.mean(REF[name + "_accuracy"])), float(np.std(REF[name + "_accuracy"])))


@pytest.mark.parametrize("name", O.TIE_CASES)
def test_tie_fixtures_match_recorded_calculate_accuracy(name):
    dist, issame = O.tie_case(name)
    assert (dist == 0.0).any() and (dist >= 4.0).any() and np.isin(dist[dist < 4.0], THR).all()
    want = REF[name]                                              # [400][tpr, fpr, acc]
    got = np.array([O.accuracy_at(t, dist, issame) for t in THR], dtype=np.float64)
    assert np.array_equal(got, want)
    assert (want[:, 1] == 0).all() if issame.all() else (want[:, 0] == 0).all()          # the zero denominators
    stats = F.stats_from_counts(*O.fold_counts(dist, issame, THR, 1), THR)
    assert np.array_equal(stats["tpr"], want[:, 0]) and np.array_equal(stats["fpr"], want[:, 1])
    assert stats["accuracy"][0] == want[:, 2].max() and stats["best_threshold"][0] == THR[int(np.argmax(want[:, 2]))]


@pytest.mark.parametrize("n,k", O.KFOLD_CASES)
def test_kfold_bounds_match_recorded_sklearn(n, k):
    sizes = KFOLD[f"{n}_{k}"]
    for bounds in (F.kfold_bounds(n, k), O.kfold_bounds(n, k)):
        assert bounds.dtype == np.int64 and bounds[0] == 0 and np.diff(bounds).tolist() == sizes


def _jpeg(img: np.ndarray) -> bytes:
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, format="JPEG", quality=95)
    return buf.getvalue()


def test_load_bin_round_trip(tmp_path):
    from PIL import Image
    rng = np.random.default_rng(0)
    smooth = np.clip(np.add.outer(np.arange(112) * 1.0, np.arange(112) * 0.5)[..., None] + np.array([0.0, 30.0, 60.0]), 0, 255).astype(np.uint8)
    imgs = [rng.integers(0, 256, (112, 112, 3), dtype=np.uint8), smooth, smooth[::-1].copy(), rng.integers(0, 256, (112, 112, 3), dtype=np.uint8)]
    bins = [imgs[0], _jpeg(imgs[1]), np.frombuffer(_jpeg(imgs[2]), dtype=np.uint8), imgs[3]]
    path = tmp_path / "pairs.bin"
    pickle.dump((bins, [True, False]), open(path, "wb"))
    data, issame = F.load_bin(str(path))
    assert data.dtype == torch.uint8 and tuple(data.shape) == (4, 112, 112, 3)
    assert issame.dtype == bool and issame.tolist() == [True, False]
    assert np.array_equal(data[0].numpy(), imgs[0]) and np.array_equal(data[3].numpy(), imgs[3])          # arrays as they are
    for k in (1, 2):                                              # encoded entries: what Pillow decodes, in RGB order
        want = np.asarray(Image.open(io.BytesIO(_jpeg(imgs[k]))).convert("RGB"))
        assert np.array_equal(data[k].numpy(), want)
        assert np.abs(data[k].numpy().astype(int) - imgs[k].astype(int)).max() <= 8
        assert data[k].numpy()[..., 2].mean() > data[k].numpy()[..., 0].mean() + 30
    pickle.dump(([imgs[0], imgs[1][:100]], [True]), open(path, "wb"))
    with pytest.raises(ValueError):
        F.load_bin(str(path))
    pickle.dump(([imgs[0], _jpeg(imgs[1][:, :96].copy())], [True]), open(path, "wb"))
    with pytest.raises(ValueError):
        F.load_bin(str(path))
    pickle.dump(([imgs[0]], [True]), open(path, "wb"))
    with pytest.raises(ValueError):
        F.load_bin(str(path))


def test_refusals():
    e = np.ones((4, 8), dtype=np.float32)
    bad = e.copy()
    bad[1, 2] = np.inf
    for args in ((e, bad), (bad, e), (e[:3], e[:3]), (e, e[:2]), (e, np.ones((4, 7), dtype=np.float32)), (e.astype(np.int32), e),
                 (np.ones(4, dtype=np.float32), e), (torch.from_numpy(e), torch.from_numpy(bad))):
        with pytest.raises(ValueError):
            F.pair_distances(*args)
    d, s = np.array([0.5, 1.0, 1.5]), np.array([True, False, True])
    for args in ((d, s, [0.0, 0.2, 0.1]), (np.array([0.5, np.nan, 1.0]), s, THR), (np.array([0.5, np.inf, 1.0]), s, THR), (d, s[:2], THR),
                 (d, s, []), (d, s, [0.0, np.nan]), (d.reshape(1, 3), s, THR), (d, s, THR, 4), (d, s, THR, 0), (d, s.astype(float), THR),
                 (d, s, np.zeros(16385))):
        with pytest.raises(ValueError):
            F.fold_counts(*args)
    for n, k in ((3, 4), (5, 0)):
        with pytest.raises(ValueError):
            F.kfold_bounds(n, k)
    with pytest.raises(ValueError):
        F.stats_from_counts(np.zeros((2, 5, 2)), np.zeros(2), np.zeros(3), np.zeros(5))
    with pytest.raises(ValueError):
        F.embed_with_flip(torch.zeros(2, 112, 112, 3), None)
    with pytest.raises(ValueError):
        F.benchmark(None, {})


def test_library_refuses_bad_arguments_before_any_hip_call(lib):
    p = 0x1000
    assert lib.idb_frb_workspace_bytes(600, 10, 400) >= 4 * 10 * 2 * 401
    for n, f, t in ((0, 1, 400), ((1 << 30) + 1, 10, 400), (600, 0, 400), (600, 65, 400), (5, 6, 400), (600, 10, 0), (600, 10, 16385)):
        assert lib.idb_frb_workspace_bytes(n, f, t) == 0
        assert lib.idb_frb_fold_counts(p, p, n, p, f, p, t, p, p, 1 << 30, None) == -1
    assert b"n_thr" in lib.idb_last_error()
    assert lib.idb_frb_workspace_bytes(1, 1, 1) > 0 and lib.idb_frb_workspace_bytes(1 << 30, 64, 16384) > 0
    assert lib.idb_frb_fold_counts(p, p, 600, p, 10, p, 400, p, p, 8, None) == -1
    assert b"workspace" in lib.idb_last_error()
    assert lib.idb_frb_fold_counts(p, p, 600, p, 10, p, 400, p, p + 8, 1 << 30, None) == -1
    assert lib.idb_frb_fold_counts(p, None, 600, p, 10, p, 400, p, p, 1 << 30, None) == -1
    assert b"null" in lib.idb_last_error()
    for n, d in ((0, 512), ((1 << 30) + 1, 512), (600, 0), (600, 8193)):
        assert lib.idb_frb_pair_dist(p, p, n, d, p, p, None) == -1
    assert b"8192" in lib.idb_last_error()
    assert lib.idb_frb_pair_dist(p, None, 600, 512, p, p, None) == -1
    assert b"null" in lib.idb_last_error()
