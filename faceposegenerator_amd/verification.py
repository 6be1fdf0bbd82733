"""The identity-verification report of the reference's evaluation (``Evaluation/PyEER_analysis``: ``PyEER_report.json``), from the
ArcFace embeddings that ``embed_faces`` returns: embeddings grouped per identity, genuine and impostor pairs "among synthetic" or
"synthetic vs real", cosine scores, and pyeer's EER, FMR / FNMR operating points, AUC, decidability, FDR, Youden index and Matthews
coefficient.  No scipy, pandas or pyeer.

The scores (``idb_verif_cos_scores``) and the ROC reductions (``idb_verif_roc``, ``csrc/idb_verif.hip``) run on the GPU in double;
the sort between them is ``torch.sort`` on the device.  The pair lists are host work: they reproduce the reference's draws
(``random.Random(seed).shuffle`` over the identities, one ``np.random.RandomState(seed)`` for its ``choice`` calls) without touching
global random state.  The final rates, the choice between the two EER candidates, ``decidability`` and ``fdr`` are float64 host
arithmetic on the counts the kernel returns, exactly as the reference forms them.

Out of scope: the curves ``thrs`` / ``fmr`` / ``fnmr`` of pyeer's ``Stats``, plots, and exhaustive all-pairs impostor statistics.
There is no CPU fallback.
"""
from __future__ import annotations

import os
import random
from typing import Sequence

import numpy as np
import torch

from . import _lib

REPORT_KEYS = ("auc", "eer", "eer_th", "fnmr0", "fnmr100", "fnmr1000", "fmr0", "fmr100", "fmr1000", "gmean", "gstd", "imean", "istd",
               "fdr", "decidability", "mccoef")
MAX_PAIRS = 1 << 30


# ---- grouping ------------------------------------------------------------------------------------------------------------------------
def group_by_identity(embs, names: Sequence[str], valid=None):
    """Rows regrouped per identity, as the reference's save_emb_2_id + load_embeddings leave them: the identity of a row is
    ``basename(name).split("_")[0]``, identities are ordered as ``sorted(listdir)`` orders their ``<id>.npy`` files, rows keep their
    order of appearance, and rows with ``valid == False`` (no face found by embed_faces) are dropped.
    Returns (embeddings [M][D] in the new order, counts int64 [n_ids], identity names)."""
    n = embs.shape[0] if hasattr(embs, "shape") and len(embs.shape) == 2 else -1
    if n < 0:
        raise ValueError(f"embs: expected an [N, D] matrix, got shape {tuple(getattr(embs, 'shape', ()))}")
    if len(names) != n:
        raise ValueError(f"names: {len(names)} names for {n} rows")
    keep = np.ones(n, dtype=bool)
    if valid is not None:
        keep = np.asarray(valid.cpu() if isinstance(valid, torch.Tensor) else valid).astype(bool)
        if keep.shape != (n,):
            raise ValueError(f"valid: expected {n} flags, got shape {keep.shape}")
    rows: dict = {}
    for i, name in enumerate(names):
        if keep[i]:
            rows.setdefault(os.path.basename(str(name)).split("_")[0], []).append(i)
    if not rows:
        raise ValueError("no valid rows")
    ids = sorted(rows, key=lambda s: s + ".npy")
    order = np.concatenate([np.asarray(rows[k], dtype=np.int64) for k in ids])
    counts = np.asarray([len(rows[k]) for k in ids], dtype=np.int64)
    if isinstance(embs, torch.Tensor):
        return embs[torch.from_numpy(order).to(embs.device)], counts, ids
    return np.asarray(embs)[order], counts, ids


# ---- pair lists ----------------------------------------------------------------------------------------------------------------------
def _check_counts(counts, name: str) -> np.ndarray:
    c = np.asarray(counts)
    if c.ndim != 1 or c.shape[0] < 1 or not np.issubdtype(c.dtype, np.integer) or (c < 1).any():
        raise ValueError(f"{name}: expected a non-empty 1-d array of positive integer counts")
    if int(c.sum()) >= 2 ** 31:
        raise ValueError(f"{name}: {int(c.sum())} rows do not fit int32 indices")
    return c.astype(np.int64)


def _pairs(counts_a: np.ndarray, counts_b: np.ndarray, seed: int, min_samples: int, samples_skip: int):
    if min_samples < 1 or samples_skip < 1:
        raise ValueError(f"min_samples = {min_samples}, samples_skip = {samples_skip}: both at least 1")
    n_ids = len(counts_a)
    start_a = np.concatenate([[0], np.cumsum(counts_a)[:-1]])
    start_b = np.concatenate([[0], np.cumsum(counts_b)[:-1]])
    order = list(range(n_ids))
    random.Random(seed).shuffle(order)                       # the reference's random.seed(seed); random.shuffle(embeddings)
    rs = np.random.RandomState(seed)                         # the reference's np.random.seed(seed); np.random.choice(...)
    gen_a, gen_b, imp_a, imp_b = [], [], [], []
    for p in range(n_ids):
        ia = order[p]
        ca, cb_own = int(counts_a[ia]), int(counts_b[ia])
        # genuine: i over the first set, j in range(i + 1, len(second set)); among synthetic the two sets are one
        i, j = np.meshgrid(np.arange(ca), np.arange(cb_own), indexing="ij")
        sel = j > i
        gen_a.append(start_a[ia] + i[sel])
        gen_b.append(start_b[ia] + j[sel])
        n_own = min(ca, min_samples)
        for q in range(p + 1, n_ids, samples_skip):
            ib = order[q]
            cb = int(counts_b[ib])
            n_ref = min(cb, min_samples)
            first = rs.choice(ca, n_own, replace=False)
            second = np.stack([rs.choice(cb, n_ref, replace=False) for _ in first])
            imp_a.append(start_a[ia] + np.repeat(first, n_ref))
            imp_b.append(start_b[ib] + second.reshape(-1))
    cat = lambda parts: (np.concatenate(parts) if parts else np.zeros(0, dtype=np.int64)).astype(np.int32)  # noqa: E731
    return cat(gen_a), cat(gen_b), cat(imp_a), cat(imp_b)


def pairs_among_synth(counts, seed: int = 0, min_samples: int = 8, samples_skip: int = 18):
    """(gen_a, gen_b, imp_a, imp_b): flat int32 row indices into the grouped embeddings, in the order and from the random draws of the
    reference's genuine_and_impostor_AmongSynth.split_gen_imp.  Genuine: all i < j within an identity.  Impostor: identity p of the
    shuffled order against identities p + 1, p + 1 + samples_skip, ..., min(count, min_samples) rows of the first drawn once and as
    many rows of the other drawn anew for each of them."""
    c = _check_counts(counts, "counts")
    return _pairs(c, c, seed, min_samples, samples_skip)


def pairs_synth_vs_real(counts_synth, counts_real, seed: int = 0, min_samples: int = 8, samples_skip: int = 17):
    """The same for genuine_and_imposter_SynthVsReal.split_gen_imp: `a` indices address the grouped synthetic rows, `b` indices the
    grouped real rows; identities are zipped positionally, as the reference zips its two sorted file lists (unequal numbers of
    identities are refused).  The reference's genuine loop is `for i in range(len(synth)): for j in range(i + 1, len(real))`: synthetic
    row i meets only the real rows with a larger index, although the two sets are different images.  That quirk is reproduced."""
    cs, cr = _check_counts(counts_synth, "counts_synth"), _check_counts(counts_real, "counts_real")
    if len(cs) != len(cr):
        raise ValueError(f"{len(cs)} synthetic identities against {len(cr)} real ones: the reference pairs them by position")
    return _pairs(cs, cr, seed, min_samples, samples_skip)


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------------
def _stream(dev) -> int:
    return torch.cuda.current_stream(dev).cuda_stream


def _check_embs(x, name: str):
    if not isinstance(x, (torch.Tensor, np.ndarray)):
        raise ValueError(f"{name}: expected a torch tensor or a numpy array")
    if len(x.shape) != 2 or x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError(f"{name}: expected a non-empty [N, D] matrix, got shape {tuple(x.shape)}")
    floating = x.is_floating_point() if isinstance(x, torch.Tensor) else np.issubdtype(x.dtype, np.floating)
    if not floating:
        raise ValueError(f"{name}: expected floating-point embeddings, got {x.dtype}")
    return x


def _check_index(idx, n_rows: int, name: str) -> np.ndarray:
    i = np.asarray(idx.cpu() if isinstance(idx, torch.Tensor) else idx)
    if i.ndim != 1 or not np.issubdtype(i.dtype, np.integer):
        raise ValueError(f"{name}: expected a 1-d integer index array")
    if i.shape[0] and (int(i.min()) < 0 or int(i.max()) >= n_rows):
        raise ValueError(f"{name}: index out of range for {n_rows} rows")
    return i.astype(np.int32)


def _upload(x, dev) -> torch.Tensor:
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    return t.to(device=dev, dtype=torch.float32).contiguous()


def cos_scores(a, b, idx_a, idx_b) -> torch.Tensor:
    """float64 device tensor [n_pairs]: the reference's pairwise_cos_sim, 1 - scipy.spatial.distance.cosine(a[idx_a[p]], b[idx_b[p]]),
    with the three dot products accumulated in double.  `a is b` is allowed.  ValueError on any non-finite score (a zero row)."""
    a = _check_embs(a, "a")
    b = a if b is a else _check_embs(b, "b")
    if a.shape[1] != b.shape[1]:
        raise ValueError(f"a has D = {a.shape[1]}, b has D = {b.shape[1]}")
    ia, ib = _check_index(idx_a, a.shape[0], "idx_a"), _check_index(idx_b, b.shape[0], "idx_b")
    if ia.shape != ib.shape or ia.shape[0] < 1 or ia.shape[0] > MAX_PAIRS:
        raise ValueError(f"idx_a, idx_b: two index arrays of one length in 1..2^30, got {ia.shape[0]} and {ib.shape[0]}")
    lib = _lib.load()
    dev = next((x.device for x in (a, b) if isinstance(x, torch.Tensor) and x.is_cuda), torch.device("cuda:0"))
    da = _upload(a, dev)
    db = da if b is a else _upload(b, dev)
    dia, dib = torch.from_numpy(ia).to(dev), torch.from_numpy(ib).to(dev)
    out = torch.empty(ia.shape[0], dtype=torch.float64, device=dev)
    _lib.check(lib.idb_verif_cos_scores(da.data_ptr(), da.shape[0], db.data_ptr(), db.shape[0], da.shape[1], dia.data_ptr(), dib.data_ptr(),
                                        ia.shape[0], out.data_ptr(), _stream(dev)), "idb_verif_cos_scores")
    if not bool(torch.isfinite(out).all()):
        raise ValueError("cos_scores: non-finite score (a zero or non-finite embedding row)")
    return out


def roc_points(g_sorted: torch.Tensor, i_sorted: torch.Tensor):
    """idb_verif_roc on two ascending float64 device tensors: (points float64 [P], ints int64 [2 P + 3], moments float64 [4]) as host
    arrays, P = len(_lib.IDB_VERIF_POINTS); the layout is the header's."""
    lib = _lib.load()
    dev, npts = g_sorted.device, len(_lib.IDB_VERIF_POINTS)
    ng, ni = g_sorted.numel(), i_sorted.numel()
    need = lib.idb_verif_workspace_bytes(ng, ni)
    if need == 0:
        raise _lib.IdbError(f"idb_verif_workspace_bytes({ng}, {ni}) refused its arguments")
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    points = torch.empty(npts, dtype=torch.float64, device=dev)
    ints = torch.empty(2 * npts + 3, dtype=torch.int64, device=dev)
    moments = torch.empty(4, dtype=torch.float64, device=dev)
    _lib.check(lib.idb_verif_roc(g_sorted.data_ptr(), ng, i_sorted.data_ptr(), ni, points.data_ptr(), ints.data_ptr(), moments.data_ptr(),
                                 ws.data_ptr(), need, _stream(dev)), "idb_verif_roc")
    return points.cpu().numpy(), ints.cpu().numpy(), moments.cpu().numpy()


def _check_scores(x, name: str, dev) -> torch.Tensor:
    if isinstance(x, torch.Tensor):
        t = x
    else:
        arr = np.asarray(x)
        if not (np.issubdtype(arr.dtype, np.floating) or np.issubdtype(arr.dtype, np.integer)):
            raise ValueError(f"{name}: expected numeric scores, got {arr.dtype}")
        t = torch.from_numpy(np.ascontiguousarray(arr, dtype=np.float64))
    if t.dim() != 1 or t.numel() < 1 or t.numel() > MAX_PAIRS:
        raise ValueError(f"{name}: expected 1..2^30 scores in a 1-d array, got shape {tuple(t.shape)}")
    if isinstance(x, torch.Tensor) and not (t.is_floating_point() or t.dtype in (torch.int32, torch.int64)):
        raise ValueError(f"{name}: expected numeric scores, got {t.dtype}")
    if not bool(torch.isfinite(t.double()).all()):
        raise ValueError(f"{name}: non-finite scores")
    return t.to(device=dev, dtype=torch.float64).contiguous()


def stats_from_roc(points, ints, moments, ng: int, ni: int) -> dict:
    """Every scalar field of pyeer's Stats, plus fdr, from the outputs of idb_verif_roc: the float64 host arithmetic of get_eer_stats."""
    idx = {name: k for k, name in enumerate(_lib.IDB_VERIF_POINTS)}
    th = lambda name: float(points[idx[name]])                                               # noqa: E731
    fmr = lambda name: np.float64(int(ints[2 * idx[name]])) / np.float64(ni)                 # noqa: E731
    fnmr = lambda name: np.float64(int(ints[2 * idx[name] + 1])) / np.float64(ng)            # noqa: E731
    npts = len(idx)
    n_le0, auc2 = int(ints[2 * npts + 1]), int(ints[2 * npts + 2])
    out: dict = {"auc": auc2 / (2 * ni * ng)}
    if n_le0 == 0:                                           # the curves do not cross: upstream returns index 0 and 1, 1, 1
        out.update(eer=1.0, eer_low=1.0, eer_high=1.0, eer_th=th("first"))
    else:
        t2 = "eer_t2"
        # t1 = t2 - 1 if diff[t2] != 0 and t2 != 0 else t2
        t1 = "eer_t1" if fmr(t2) - fnmr(t2) != 0 and int(ints[2 * idx["eer_t1"]]) >= 0 else t2
        if fmr(t1) + fnmr(t1) <= fmr(t2) + fnmr(t2):
            out.update(eer=float((fnmr(t1) + fmr(t1)) / 2), eer_low=float(fnmr(t1)), eer_high=float(fmr(t1)), eer_th=th(t1))
        else:
            out.update(eer=float((fnmr(t2) + fmr(t2)) / 2), eer_low=float(fmr(t2)), eer_high=float(fnmr(t2)), eer_th=th(t2))
    for name in ("fmr0", "fmr1000", "fmr100", "fmr20", "fmr10"):
        out[name], out[name + "_th"] = float(fnmr(name)), th(name)
    for name in ("fnmr0", "fnmr100", "fnmr1000"):
        out[name] = float(fmr(name))
    out["fnmr0_th"] = th("fnmr0")
    out["j_index"], out["j_index_th"] = float(1 - fnmr("youden") - fmr("youden")), th("youden")
    fm, fnm = np.float64(int(ints[2 * idx["mcc"]])), np.float64(int(ints[2 * idx["mcc"] + 1]))
    tn, tp = ni - fm, ng - fnm
    den = (np.sqrt(tp + fm) * np.sqrt(tp + fnm)) * (np.sqrt(tn + fm) * np.sqrt(tn + fnm))
    out["mccoef"], out["mccoef_th"] = float((tp * tn - fm * fnm) / (den if den != 0 else 1.0)), th("mcc")
    gmean, gstd, imean, istd = (np.float64(m) for m in moments)
    out.update(gmean=float(gmean), gstd=float(gstd), imean=float(imean), istd=float(istd))
    with np.errstate(divide="ignore", invalid="ignore"):
        out["decidability"] = 1.0 if gstd == 0 and istd == 0 else float(abs(gmean - imean) / np.sqrt(0.5 * (gstd ** 2 + istd ** 2)))
        out["fdr"] = float((gmean - imean) ** 2 / (gstd ** 2 + istd ** 2))
    return out


def eer_stats(gen_scores, imp_scores) -> dict:
    """pyeer's get_eer_stats(gen_scores, imp_scores) for similarity scores: every scalar field of its Stats, plus the reference's
    fdr.  Scores: 1-d float64 device tensors (cos_scores) or host arrays (uploaded)."""
    dev = next((x.device for x in (gen_scores, imp_scores) if isinstance(x, torch.Tensor) and x.is_cuda), torch.device("cuda:0"))
    g, i = _check_scores(gen_scores, "gen_scores", dev), _check_scores(imp_scores, "imp_scores", dev)
    points, ints, moments = roc_points(torch.sort(g).values, torch.sort(i).values)
    return stats_from_roc(points, ints, moments, g.numel(), i.numel())


def verification_report(embs, names, real_embs=None, real_names=None, valid=None, real_valid=None, seed: int = 0) -> dict:
    """From embeddings to the reference's PyEER_report.json: the 16 keys of its report_which_metrics in its order, under "report";
    the genuine and impostor score tensors (float64, device) under "gen_scores" and "imp_scores"; "config" is "vsSynth" when no real
    set is given (pairs among the synthetic identities) and "vsReal" otherwise (synthetic against real, identities paired by
    position in the sorted order)."""
    if (real_embs is None) != (real_names is None):
        raise ValueError("real_embs and real_names go together")
    synth, counts, _ = group_by_identity(_check_embs(embs, "embs"), names, valid)
    if real_embs is None:
        ga, gb, ia, ib = pairs_among_synth(counts, seed=seed)
        other, config = synth, "vsSynth"
    else:
        other, counts_real, _ = group_by_identity(_check_embs(real_embs, "real_embs"), real_names, real_valid)
        ga, gb, ia, ib = pairs_synth_vs_real(counts, counts_real, seed=seed)
        config = "vsReal"
    if len(ga) == 0 or len(ia) == 0:
        raise ValueError(f"{len(ga)} genuine and {len(ia)} impostor pairs: the report needs at least one of each")
    gen, imp = cos_scores(synth, other, ga, gb), cos_scores(synth, other, ia, ib)
    stats = eer_stats(gen, imp)
    return {"config": config, "report": {k: stats[k] for k in REPORT_KEYS}, "gen_scores": gen, "imp_scores": imp}
