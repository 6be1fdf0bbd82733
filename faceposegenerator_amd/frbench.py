"""The pair-verification benchmark of a face-recognition backbone, the reference's headline utility number (``FR_training/test_FR.py``
-> ``CallBackVerification.ver_test`` -> ``utils/verification.py``: LFW, CFP-FP, AgeDB-30, CALFW, CPLFW): the benchmark's ``.bin``
file, embeddings of every crop and of its horizontal mirror, the L2-normalised sum of the two, squared distances of the pairs, the
10-fold search of the best threshold over ``np.arange(0, 4, 0.01)``, and the accuracy record.  No sklearn, scipy or mxnet.

The backbones of ``FR_training/backbones/iresnet.py`` (``iresnet18``, ``iresnet50``) are ``arcface.ArcFace`` with ``arch="r18"`` /
``"r50"``; ``embed_u8`` fuses the benchmark's ``((x / 255) - 0.5) / 0.5``.  The distances (``idb_frb_pair_dist``) and the per-fold,
per-threshold counts (``idb_frb_fold_counts``, ``csrc/idb_frbench.hip``) run on the GPU in double; the rates, the argmax and the means
are float64 host arithmetic on those integer counts, formed exactly as ``calculate_roc`` / ``calculate_accuracy`` form them.  There is
no CPU fallback.

Out of scope:
``calculate_val`` (VAL @ FAR 1e-3 over ``arange(0, 4, 0.001)``): ``verification.test`` discards its result, and its ``interp1d`` over
duplicate FAR values is refused by current scipy, so ``test`` returns only what the reference keeps.
The ``pca > 0`` branch, ``test_da``, ``is_vae`` backbones and FR training.
Precision: the reference runs the backbone in fp32, here it runs on f16 / bf16 MFMA operands; parity with trained weights is unpinned,
as everywhere in this package.
"""
from __future__ import annotations

import io
import pickle
from typing import Dict, Tuple, Union

import numpy as np
import torch

from . import _lib

MAX_PAIRS = 1 << 30
MAX_FOLDS = 64
MAX_THRESHOLDS = 16384
MAX_DIM = 8192


# ---- the benchmark file ----------------------------------------------------------------------------------------------------------------
def load_bin(path: str, image_size: Tuple[int, int] = (112, 112)):
    """The pickled ``(bins, issame_list)`` of an insightface benchmark file (lfw.bin, cfp_fp.bin, ...) -> (uint8 tensor
    [2P, H, W, 3] in RGB, bool array [P]); images 2p and 2p + 1 are pair p.  Entries that already are H x W x 3 arrays are taken as
    they are; encoded entries (JPEG / PNG bytes) are decoded with Pillow and converted to RGB.  An image of another size raises
    ValueError (the reference's resize is commented out).  The reference decodes with ``mx.image.imdecode``: decoder parity (the
    JPEG IDCT and chroma upsampling of the two libraries) is unpinned."""
    try:
        with open(path, "rb") as f:
            bins, issame_list = pickle.load(f)
    except UnicodeDecodeError:
        with open(path, "rb") as f:
            bins, issame_list = pickle.load(f, encoding="bytes")
    issame = np.asarray(issame_list).astype(bool)
    if issame.ndim != 1 or issame.shape[0] < 1 or len(bins) < 2 * issame.shape[0]:
        raise ValueError(f"{path}: {len(bins)} images for {issame.shape} pair labels")
    h, w = int(image_size[0]), int(image_size[1])
    out = np.empty((2 * issame.shape[0], h, w, 3), dtype=np.uint8)
    for i in range(out.shape[0]):
        entry = bins[i]
        if not isinstance(entry, (bytes, bytearray)) and len(getattr(entry, "shape", ())) > 2:
            img = np.asarray(entry)
        else:
            from PIL import Image
            raw = bytes(entry) if isinstance(entry, (bytes, bytearray)) else np.asarray(entry, dtype=np.uint8).tobytes()
            img = np.asarray(Image.open(io.BytesIO(raw)).convert("RGB"))
        if img.shape != (h, w, 3):
            raise ValueError(f"{path}: image {i} is {img.shape}, expected {(h, w, 3)}")
        out[i] = img
    return torch.from_numpy(out), issame


# ---- embeddings ------------------------------------------------------------------------------------------------------------------------
def embed_with_flip(images_u8, backbone):
    """[embed_u8(images), embed_u8(images mirrored left-right)], both fp32 [2P, D] on the backbone's device: the reference's
    embeddings_list.  The mirror is a flip of the uint8 NHWC batch along W; chunking is the backbone's own."""
    t = images_u8 if torch.is_tensor(images_u8) else torch.from_numpy(np.ascontiguousarray(images_u8))
    if t.dtype != torch.uint8 or t.ndim != 4 or t.shape[-1] != 3 or t.shape[0] < 1:
        raise ValueError(f"embed_with_flip expects a uint8 [N, H, W, 3] batch, got {t.dtype} {tuple(t.shape)}")
    return [backbone.embed_u8(t), backbone.embed_u8(t.flip(2))]


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------------
def _stream(dev) -> int:
    return torch.cuda.current_stream(dev).cuda_stream


def _device(*xs):
    return next((x.device for x in xs if isinstance(x, torch.Tensor) and x.is_cuda), torch.device("cuda:0"))


def _check_embs(x, name: str):
    if not isinstance(x, (torch.Tensor, np.ndarray)):
        raise ValueError(f"{name}: expected a torch tensor or a numpy array")
    if len(x.shape) != 2 or x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError(f"{name}: expected a non-empty [N, D] matrix, got shape {tuple(x.shape)}")
    floating = x.is_floating_point() if isinstance(x, torch.Tensor) else np.issubdtype(x.dtype, np.floating)
    if not floating:
        raise ValueError(f"{name}: expected floating-point embeddings, got {x.dtype}")
    return x


def _finite(x) -> bool:
    return bool(torch.isfinite(x).all()) if isinstance(x, torch.Tensor) else bool(np.isfinite(x).all())


def _upload(x, dev) -> torch.Tensor:
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    return t.to(device=dev, dtype=torch.float32).contiguous()


def pair_dist_norms(e0, e1):
    """idb_frb_pair_dist on the fp32 embeddings e0 (images) and e1 (mirrors), both [2P, D]: (dist float64 [P], norms float64 [2, 2P]) on
    the device; the layout is the header's.  ValueError on non-finite embeddings, an odd row count or mismatched shapes."""
    e0, e1 = _check_embs(e0, "e0"), _check_embs(e1, "e1")
    if tuple(e0.shape) != tuple(e1.shape):
        raise ValueError(f"e0 is {tuple(e0.shape)}, e1 is {tuple(e1.shape)}")
    n, d = int(e0.shape[0]), int(e0.shape[1])
    if n % 2 or n // 2 > MAX_PAIRS or d > MAX_DIM:
        raise ValueError(f"expected an even number of rows (at most 2^31) and D <= {MAX_DIM}, got {(n, d)}")
    if not (_finite(e0) and _finite(e1)):
        raise ValueError("non-finite embeddings")
    lib = _lib.load()
    dev = _device(e0, e1)
    d0, d1 = _upload(e0, dev), _upload(e1, dev)
    dist = torch.empty(n // 2, dtype=torch.float64, device=dev)
    norms = torch.empty((2, n), dtype=torch.float64, device=dev)
    _lib.check(lib.idb_frb_pair_dist(d0.data_ptr(), d1.data_ptr(), n // 2, d, dist.data_ptr(), norms.data_ptr(), _stream(dev)),
               "idb_frb_pair_dist")
    return dist, norms


def pair_distances(e0, e1):
    """(dist, xnorm): dist a float64 device tensor [P], the squared distance of rows 2p and 2p + 1 of normalize(e0 + e1); xnorm the
    reference's _xnorm, the sum of the 4P row norms in its order (the rows of e0, then of e1) divided by 4P, on the host."""
    dist, norms = pair_dist_norms(e0, e1)
    total = 0.0
    for v in norms.cpu().numpy().reshape(-1):                # the reference's `_xnorm += _norm`, one row at a time
        total += v
    return dist, float(total / norms.numel())


def kfold_bounds(n: int, nfolds: int) -> np.ndarray:
    """int64 [nfolds + 1]: the boundaries of the contiguous test blocks of sklearn's KFold(nfolds, shuffle=False) over n samples (the
    first n % nfolds folds have n // nfolds + 1 members).  nfolds = 1 is the reference's LFold special case: one fold that is both
    train and test."""
    n, nfolds = int(n), int(nfolds)
    if nfolds < 1 or n < nfolds:
        raise ValueError(f"kfold_bounds: {nfolds} folds of {n} samples")
    sizes = np.full(nfolds, n // nfolds, dtype=np.int64)
    sizes[:n % nfolds] += 1
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def fold_counts(dist, issame, thresholds, nfolds: int = 10):
    """(counts int64 [nfolds, T, 2], fold_same int64 [nfolds], fold_size int64 [nfolds]) on the host: counts[f, t, 0] the pairs of
    test fold f with issame and dist < thresholds[t], counts[f, t, 1] the same for the pairs that are not the same identity; fold_same
    the "same" pairs of each fold.  dist: [P] float64 (device tensor or host array).  ValueError for decreasing thresholds, non-finite
    distances and len(issame) != len(dist) (the reference silently truncates to the shorter)."""
    thr = np.ascontiguousarray(np.asarray(thresholds, dtype=np.float64))
    if thr.ndim != 1 or thr.shape[0] < 1 or thr.shape[0] > MAX_THRESHOLDS:
        raise ValueError(f"thresholds: expected 1..{MAX_THRESHOLDS} values in a 1-d array, got shape {thr.shape}")
    if not np.isfinite(thr).all() or (np.diff(thr) < 0).any():
        raise ValueError("thresholds: expected finite, non-decreasing values")
    same = np.asarray(issame.cpu() if isinstance(issame, torch.Tensor) else issame)
    if same.ndim != 1 or same.dtype.kind not in "biu":
        raise ValueError(f"issame: expected a 1-d boolean array, got {same.dtype} {same.shape}")
    same = same.astype(bool)
    dev = _device(dist)
    d = dist if isinstance(dist, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(dist, dtype=np.float64)))
    if d.dim() != 1 or d.numel() < 1 or d.numel() > MAX_PAIRS or not d.is_floating_point():
        raise ValueError(f"dist: expected 1..2^30 floating-point distances in a 1-d array, got {d.dtype} {tuple(d.shape)}")
    n = d.numel()
    if same.shape[0] != n:
        raise ValueError(f"{same.shape[0]} labels for {n} distances")
    nfolds = int(nfolds)
    if nfolds < 1 or nfolds > MAX_FOLDS or nfolds > n:
        raise ValueError(f"nfolds = {nfolds}: expected 1..{MAX_FOLDS} and at most the {n} pairs")
    if not _finite(d):
        raise ValueError("dist: non-finite distances")
    d = d.to(device=dev, dtype=torch.float64).contiguous()
    lib = _lib.load()
    bounds = kfold_bounds(n, nfolds)
    T = thr.shape[0]
    need = lib.idb_frb_workspace_bytes(n, nfolds, T)
    if need == 0:
        raise _lib.IdbError(f"idb_frb_workspace_bytes({n}, {nfolds}, {T}) refused its arguments")
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    d_same = torch.from_numpy(same.astype(np.uint8)).to(dev)
    d_start = torch.from_numpy(bounds.astype(np.int32)).to(dev)
    d_thr = torch.from_numpy(thr).to(dev)
    counts = torch.empty((nfolds, T, 2), dtype=torch.int32, device=dev)
    _lib.check(lib.idb_frb_fold_counts(d.data_ptr(), d_same.data_ptr(), n, d_start.data_ptr(), nfolds, d_thr.data_ptr(), T,
                                       counts.data_ptr(), ws.data_ptr(), need, _stream(dev)), "idb_frb_fold_counts")
    fold_same = np.add.reduceat(same.astype(np.int64), bounds[:-1])
    return counts.cpu().numpy().astype(np.int64), fold_same.astype(np.int64), np.diff(bounds).astype(np.int64)


# ---- host statistics -------------------------------------------------------------------------------------------------------------------
def stats_from_counts(counts, fold_same, fold_size, thresholds) -> dict:
    """What calculate_roc returns, from the counts of the test folds: per fold the train counts are the totals minus the fold's own
    (for a single fold, the fold's own: train and test are both everything), the first argmax of the train accuracy is the fold's best
    threshold, tprs / fprs of the test fold follow calculate_accuracy's `0 if denominator == 0` rule, and accuracy[f] =
    float(tp + tn) / fold_size.  Returns tpr, fpr (np.mean over the folds, [T]), accuracy [nfolds], best_threshold [nfolds], acc =
    np.mean(accuracy), std = np.std(accuracy).  Pure host float64."""
    counts = np.asarray(counts, dtype=np.int64)
    fold_same, fold_size = np.asarray(fold_same, dtype=np.int64), np.asarray(fold_size, dtype=np.int64)
    thr = np.asarray(thresholds, dtype=np.float64)
    nfolds, T = counts.shape[0], counts.shape[1]
    if counts.shape != (nfolds, T, 2) or fold_same.shape != (nfolds,) or fold_size.shape != (nfolds,) or thr.shape != (T,):
        raise ValueError(f"counts {counts.shape}, fold_same {fold_same.shape}, fold_size {fold_size.shape}, thresholds {thr.shape}")
    total, total_same, total_size = counts.sum(axis=0), int(fold_same.sum()), int(fold_size.sum())
    tprs, fprs = np.zeros((nfolds, T)), np.zeros((nfolds, T))
    accuracy, best = np.zeros(nfolds), np.zeros(nfolds)
    for f in range(nfolds):
        n_same, n_all = int(fold_same[f]), int(fold_size[f])
        if nfolds > 1:
            train, tr_same, tr_all = total - counts[f], total_same - n_same, total_size - n_all
        else:
            train, tr_same, tr_all = counts[f], n_same, n_all
        acc_train = np.zeros(T)
        for t in range(T):
            tp, fp = int(train[t, 0]), int(train[t, 1])
            tn = (tr_all - tr_same) - fp
            acc_train[t] = float(tp + tn) / tr_all
        k = int(np.argmax(acc_train))
        for t in range(T):
            tp, fp = int(counts[f, t, 0]), int(counts[f, t, 1])
            fn, tn = n_same - tp, (n_all - n_same) - fp
            tprs[f, t] = 0 if (tp + fn == 0) else float(tp) / float(tp + fn)
            fprs[f, t] = 0 if (fp + tn == 0) else float(fp) / float(fp + tn)
        tp, fp = int(counts[f, k, 0]), int(counts[f, k, 1])
        accuracy[f] = float(tp + ((n_all - n_same) - fp)) / n_all
        best[f] = thr[k]
    return {"tpr": np.mean(tprs, 0), "fpr": np.mean(fprs, 0), "accuracy": accuracy, "best_threshold": best,
            "acc": float(np.mean(accuracy)), "std": float(np.std(accuracy))}


# ---- the benchmark ---------------------------------------------------------------------------------------------------------------------
def evaluate(e0, e1, issame, nfolds: int = 10) -> dict:
    """The reference's embedding_preprocessing + evaluate (without calculate_val) from the two embedding matrices: the keys of
    stats_from_counts plus xnorm, dist (float64, device), thresholds (np.arange(0, 4, 0.01), numpy's own doubles) and the genuine /
    impostor distances (host float64, the content of save_genuines_impostors, for the caller to write)."""
    same = np.asarray(issame.cpu() if isinstance(issame, torch.Tensor) else issame)
    dist, xnorm = pair_distances(e0, e1)
    thresholds = np.arange(0, 4, 0.01)
    counts, fold_same, fold_size = fold_counts(dist, same, thresholds, nfolds)
    out = stats_from_counts(counts, fold_same, fold_size, thresholds)
    host = dist.cpu().numpy()
    same = same.astype(bool)
    out.update(xnorm=xnorm, dist=dist, thresholds=thresholds, genuine=host[same], impostor=host[~same])
    return out


def test(images_u8, issame, backbone, nfolds: int = 10):
    """verification.test: (acc1, std1, acc2, std2, xnorm, embeddings_list) with acc1 = std1 = 0.0 as the reference leaves them, acc2 /
    std2 the mean and standard deviation of the fold accuracies, embeddings_list the two fp32 device matrices of embed_with_flip."""
    embeddings_list = embed_with_flip(images_u8, backbone)
    out = evaluate(embeddings_list[0], embeddings_list[1], issame, nfolds)
    return 0.0, 0.0, out["acc"], out["std"], out["xnorm"], embeddings_list


test.__test__ = False                                        # the reference's name; not a pytest test


def benchmark(backbone, sets: Dict[str, Union[str, tuple]], nfolds: int = 10) -> dict:
    """The record test_FR.py dumps: {name: [acc2], ..., "Average": [sum of acc2 / number of sets]}.  Each set is the path of a .bin file
    or an (images_u8, issame) tuple."""
    if not sets:
        raise ValueError("benchmark: no benchmark set")
    record: dict = {}
    for name, src in sets.items():
        images, issame = load_bin(src) if isinstance(src, (str, bytes)) or hasattr(src, "__fspath__") else src
        record[name] = [test(images, issame, backbone, nfolds)[2]]
    record["Average"] = [sum([v[0] / len(record) for v in record.values()])]
    return record
