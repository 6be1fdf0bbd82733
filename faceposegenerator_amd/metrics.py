"""The distribution metrics of the reference's evaluation run over image features (``python -m dgm_eval REAL GEN --model dinov2
--metrics prdc vendi fd kd authpct``), from the ``[N, D]`` float32 matrices that ``DinoV2.features_u8`` returns.

PRDC, KD and AuthPct are all-pairs work, O(N^2 D): they run on the GPU through the ``idb_pair_*`` kernels (exact f32-input MFMA,
``csrc/idb_pair.hip``), which never write an N x N matrix.  Distances are taken on features centred on the mean of the real set
(they are translation invariant, and the centring removes most of the cancellation in |a|^2 + |b|^2 - 2 a.b); the polynomial kernel
of KD is not translation invariant and runs on the features as they are.

``fd`` and ``vendi_per_class`` are deliberately CPU code, float64 numpy / scipy: FD is a D x D covariance and a matrix square root
(about 20 GFLOP, sensitive to round-off in the small eigenvalues), per-class Vendi an eigen-decomposition of tiny Gram matrices.

Inputs are torch tensors on the GPU or numpy arrays (uploaded once).  There is no CPU fallback for the GPU metrics.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib

MAX_KTH = 8                      # idb_pair_knn_radii keeps 8 candidates per query
SCORE_KEYS = ("fd", "kd_value", "kd_variance", "precision", "recall", "density", "coverage", "mean vendi per class",
              "std vendi per class", "authpct")


# ---- validation (before anything touches the GPU) ----------------------------------------------------------------------------------
def _check_matrix(x, name: str):
    if isinstance(x, torch.Tensor):
        if x.dim() != 2 or x.shape[0] < 1 or x.shape[1] < 1:
            raise ValueError(f"{name}: expected a non-empty [N, D] matrix, got shape {tuple(x.shape)}")
        if not x.is_floating_point():
            raise ValueError(f"{name}: expected floating-point features, got {x.dtype}")
        if not bool(torch.isfinite(x).all()):
            raise ValueError(f"{name}: non-finite values")
        return x
    a = np.asarray(x)
    if a.ndim != 2 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f"{name}: expected a non-empty [N, D] matrix, got shape {a.shape}")
    if not np.issubdtype(a.dtype, np.floating):
        raise ValueError(f"{name}: expected floating-point features, got {a.dtype}")
    if not np.isfinite(a).all():
        raise ValueError(f"{name}: non-finite values")
    return a


def _check_pair(real, gen):
    real, gen = _check_matrix(real, "real"), _check_matrix(gen, "gen")
    if real.shape[1] != gen.shape[1]:
        raise ValueError(f"real has D = {real.shape[1]}, gen has D = {gen.shape[1]}")
    return real, gen


def _check_k(real, gen, nearest_k: int) -> None:
    if nearest_k < 1:
        raise ValueError(f"nearest_k = {nearest_k}: must be at least 1")
    if nearest_k + 1 > MAX_KTH:
        raise ValueError(f"nearest_k + 1 = {nearest_k + 1} > {MAX_KTH}: the k-nearest kernel keeps {MAX_KTH} candidates per query")
    for name, x in (("real", real), ("gen", gen)):
        if x.shape[0] <= nearest_k:
            raise ValueError(f"{name}: N = {x.shape[0]} <= nearest_k = {nearest_k}")


def _device_of(*xs) -> torch.device:
    for x in xs:
        if isinstance(x, torch.Tensor) and x.is_cuda:
            return x.device
    return torch.device("cuda:0")


def _upload(x, dev: torch.device) -> torch.Tensor:
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    return t.to(device=dev, dtype=torch.float32).contiguous()


def _host(x) -> np.ndarray:
    return (x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)).astype(np.float64)


# ---- the C ABI, one function per entry ---------------------------------------------------------------------------------------------
def _stream(dev) -> int:
    return torch.cuda.current_stream(dev).cuda_stream


def _workspace(lib, mode: int, na: int, nb: int, subsets: int, dev) -> torch.Tensor:
    need = lib.idb_pair_workspace_bytes(mode, na, nb, subsets)
    if need == 0:
        raise _lib.IdbError(f"idb_pair_workspace_bytes(mode {mode}, {na}, {nb}, {subsets}) refused its arguments")
    return torch.empty(need, dtype=torch.uint8, device=dev)


def _shift_ptr(shift: Optional[torch.Tensor]):
    return shift.data_ptr() if shift is not None else None


def pair_dist2(a: torch.Tensor, b: torch.Tensor, shift: Optional[torch.Tensor]) -> torch.Tensor:
    """d2 [Na][Nb] of two float32 device matrices (the store mode: tests and tiny inputs)."""
    lib = _lib.load()
    out = torch.empty(a.shape[0], b.shape[0], dtype=torch.float32, device=a.device)
    ws = _workspace(lib, _lib.IDB_PAIR_DIST2, a.shape[0], b.shape[0], 0, a.device)
    _lib.check(lib.idb_pair_dist2(a.data_ptr(), a.shape[0], b.data_ptr(), b.shape[0], a.shape[1], _shift_ptr(shift), out.data_ptr(),
                                  ws.data_ptr(), ws.numel(), _stream(a.device)), "idb_pair_dist2")
    return out


def pair_knn_radii(x: torch.Tensor, shift: Optional[torch.Tensor], kth: int) -> torch.Tensor:
    """r2 [N]: the kth smallest of each row of d2(x, x), the point itself (exactly 0) being the first."""
    lib = _lib.load()
    out = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
    ws = _workspace(lib, _lib.IDB_PAIR_KNN, x.shape[0], 0, 0, x.device)
    _lib.check(lib.idb_pair_knn_radii(x.data_ptr(), x.shape[0], x.shape[1], _shift_ptr(shift), kth, out.data_ptr(), ws.data_ptr(),
                                      ws.numel(), _stream(x.device)), "idb_pair_knn_radii")
    return out


def pair_prdc_counts(real: torch.Tensor, gen: torch.Tensor, shift, r2_real: torch.Tensor, r2_gen: torch.Tensor):
    """(in_real_sphere int32 [Ng], covered int32 [Nr], row_min float32 [Nr]) in one pass over d2(real, gen)."""
    lib = _lib.load()
    nr, ng, dev = real.shape[0], gen.shape[0], real.device
    inside = torch.empty(ng, dtype=torch.int32, device=dev)
    covered = torch.empty(nr, dtype=torch.int32, device=dev)
    row_min = torch.empty(nr, dtype=torch.float32, device=dev)
    ws = _workspace(lib, _lib.IDB_PAIR_PRDC, nr, ng, 0, dev)
    _lib.check(lib.idb_pair_prdc_counts(real.data_ptr(), nr, gen.data_ptr(), ng, real.shape[1], _shift_ptr(shift), r2_real.data_ptr(),
                                        r2_gen.data_ptr(), inside.data_ptr(), covered.data_ptr(), row_min.data_ptr(), ws.data_ptr(),
                                        ws.numel(), _stream(dev)), "idb_pair_prdc_counts")
    return inside, covered, row_min


def pair_nearest(a: torch.Tensor, b: torch.Tensor, shift, exclude_diag: bool):
    """(min_i d2(i, j) float32 [Nb], its argmin int32 [Nb], lowest index on a tie); exclude_diag leaves i == j out."""
    lib = _lib.load()
    na, nb, dev = a.shape[0], b.shape[0], a.device
    mins = torch.empty(nb, dtype=torch.float32, device=dev)
    args = torch.empty(nb, dtype=torch.int32, device=dev)
    ws = _workspace(lib, _lib.IDB_PAIR_NEAREST, na, nb, 0, dev)
    _lib.check(lib.idb_pair_nearest(a.data_ptr(), na, b.data_ptr(), nb, a.shape[1], _shift_ptr(shift), int(exclude_diag), mins.data_ptr(),
                                    args.data_ptr(), ws.data_ptr(), ws.numel(), _stream(dev)), "idb_pair_nearest")
    return mins, args


def pair_poly_sums(x: torch.Tensor, y: torch.Tensor, idx_x: torch.Tensor, idx_y: torch.Tensor, gamma: float, coef0: float) -> torch.Tensor:
    """float64 [S][3]: sum_{i != j} k(x_i, x_j), sum_{i != j} k(y_i, y_j), sum_{i, j} k(x_i, y_j) over the rows idx_x[s], idx_y[s]
    (int32 device [S][m]) with k(a, b) = (gamma a.b + coef0)^3."""
    lib = _lib.load()
    s, m = idx_x.shape
    if idx_y.shape != idx_x.shape or idx_x.dtype != torch.int32 or idx_y.dtype != torch.int32:
        raise ValueError("idx_x and idx_y: int32 [S][m] of one shape")
    if int(idx_x.min()) < 0 or int(idx_x.max()) >= x.shape[0] or int(idx_y.min()) < 0 or int(idx_y.max()) >= y.shape[0]:
        raise ValueError("subset index out of range")
    out = torch.empty(s, 3, dtype=torch.float64, device=x.device)
    ws = _workspace(lib, _lib.IDB_PAIR_POLY, m, 0, s, x.device)
    idx_x, idx_y = idx_x.contiguous(), idx_y.contiguous()
    _lib.check(lib.idb_pair_poly_sums(x.data_ptr(), x.shape[0], y.data_ptr(), y.shape[0], x.shape[1], idx_x.data_ptr(), idx_y.data_ptr(),
                                      s, m, gamma, coef0, out.data_ptr(), ws.data_ptr(), ws.numel(), _stream(x.device)),
               "idb_pair_poly_sums")
    return out


def _centre(real: torch.Tensor) -> torch.Tensor:
    return real.mean(dim=0, dtype=torch.float64).float().contiguous()


# ---- the metrics -------------------------------------------------------------------------------------------------------------------
def prdc(real, gen, nearest_k: int = 5) -> dict:
    """Precision, recall, density and coverage (Naeem et al. 2020) as dgm-eval's compute_prdc forms them: the radius of a point is
    the distance to its nearest_k-th neighbour within its own set; precision = the share of generated points inside some real
    sphere, recall = the share of real points inside some generated sphere, density = the mean number of real spheres a generated
    point lies in, over nearest_k, coverage = the share of real points whose nearest generated point lies inside their sphere.
    All comparisons are strict and on squared distances."""
    real, gen = _check_pair(real, gen)
    _check_k(real, gen, nearest_k)
    dev = _device_of(real, gen)
    r, g = _upload(real, dev), _upload(gen, dev)
    mu = _centre(r)
    r2_real, r2_gen = pair_knn_radii(r, mu, nearest_k + 1), pair_knn_radii(g, mu, nearest_k + 1)
    inside, covered, row_min = pair_prdc_counts(r, g, mu, r2_real, r2_gen)
    nr, ng = r.shape[0], g.shape[0]
    return {"precision": int((inside > 0).sum()) / ng, "recall": int(covered.sum()) / nr,
            "density": int(inside.sum(dtype=torch.int64)) / (float(nearest_k) * ng),
            "coverage": int((row_min < r2_real).sum()) / nr}


def authpct(real, gen) -> float:
    """The percentage of generated points that are 'authentic' (Alaa et al. 2022, as dgm-eval computes it): a generated point whose
    nearest real point has another real point closer to it than the generated point is."""
    real, gen = _check_pair(real, gen)
    if real.shape[0] < 2:
        raise ValueError("real: N = 1, there is no nearest other real point")
    dev = _device_of(real, gen)
    r, g = _upload(real, dev), _upload(gen, dev)
    mu = _centre(r)
    real_min, _ = pair_nearest(r, r, mu, True)
    gen_min, gen_arg = pair_nearest(r, g, mu, False)
    authentic = real_min[gen_arg.long()] < gen_min
    return 100.0 * int(authentic.sum()) / g.shape[0]


def mmd2_from_sums(sums: np.ndarray, m: int) -> np.ndarray:
    """The unbiased MMD^2 estimate from the three kernel sums of a subset of m rows each."""
    return (sums[..., 0] + sums[..., 1]) / (m * (m - 1)) - 2.0 * sums[..., 2] / (m * m)


def kd(real, gen, n_subsets: int = 100, subset_size: int = 1000, rng=None, subsets=None) -> np.ndarray:
    """Kernel distance (the KID estimator of Binkowski et al. 2018 on these features): the unbiased MMD^2 with the kernel
    (a.b / D + 1)^3 on n_subsets random subsets of min(subset_size, N_real, N_gen) rows each, drawn without replacement on the host
    (the reference does not seed its draws, so there is no stream to reproduce).  subsets = (idx_real, idx_gen), two [S][m] integer
    arrays, replaces the draw.  Returns the n_subsets values; their mean and standard deviation are the reference's kd_value and
    kd_variance."""
    real, gen = _check_pair(real, gen)
    if subsets is None:
        m = min(subset_size, real.shape[0], gen.shape[0])
        if n_subsets < 1 or m < 2:
            raise ValueError(f"n_subsets = {n_subsets}, subset size = {m}: need at least 1 subset of 2 rows")
        rng = np.random.default_rng() if rng is None else rng
        ix = np.stack([rng.choice(real.shape[0], m, replace=False) for _ in range(n_subsets)])
        iy = np.stack([rng.choice(gen.shape[0], m, replace=False) for _ in range(n_subsets)])
    else:
        ix, iy = np.asarray(subsets[0]), np.asarray(subsets[1])
        if ix.ndim != 2 or ix.shape != iy.shape or ix.shape[1] < 2:
            raise ValueError("subsets: two [S][m] index arrays of one shape, m >= 2")
        if ix.min() < 0 or ix.max() >= real.shape[0] or iy.min() < 0 or iy.max() >= gen.shape[0]:
            raise ValueError("subsets: index out of range")
        m = ix.shape[1]
    dev = _device_of(real, gen)
    r, g = _upload(real, dev), _upload(gen, dev)
    out = np.zeros(ix.shape[0])
    step = 4096                                                        # subsets per launch (the grid's z extent is 3 per subset)
    for s0 in range(0, ix.shape[0], step):
        dx = torch.from_numpy(np.ascontiguousarray(ix[s0:s0 + step], dtype=np.int32)).to(dev)
        dy = torch.from_numpy(np.ascontiguousarray(iy[s0:s0 + step], dtype=np.int32)).to(dev)
        sums = pair_poly_sums(r, g, dx, dy, 1.0 / r.shape[1], 1.0).cpu().numpy()
        out[s0:s0 + step] = mmd2_from_sums(sums, m)
    return out


def fd(real, gen, eps: float = 1e-6) -> float:
    """Frechet distance between the Gaussians fitted to the two sets, |mu1 - mu2|^2 + Tr(C1 + C2 - 2 sqrt(C1 C2)).  Deliberately CPU,
    float64: np.cov and scipy's sqrtm, with eps on both diagonals when the product is singular (a non-finite root)."""
    from scipy import linalg
    real, gen = _check_pair(real, gen)
    a, b = _host(real), _host(gen)
    mu1, mu2 = a.mean(axis=0), b.mean(axis=0)
    c1, c2 = np.atleast_2d(np.cov(a, rowvar=False)), np.atleast_2d(np.cov(b, rowvar=False))
    root = linalg.sqrtm(c1 @ c2)
    if not np.isfinite(root).all():
        off = np.eye(c1.shape[0]) * eps
        root = linalg.sqrtm((c1 + off) @ (c2 + off))
    if np.iscomplexobj(root):
        if not np.allclose(np.diagonal(root).imag, 0, atol=1e-3):
            raise ValueError(f"fd: imaginary component {np.abs(root.imag).max()} in sqrt(C1 C2)")
        root = root.real
    d = mu1 - mu2
    return float(d @ d + np.trace(c1) + np.trace(c2) - 2.0 * np.trace(root))


def vendi(x) -> float:
    """Vendi score (Friedman & Dieng 2022) with q = 1: exp of the Shannon entropy of the eigenvalues of K / n, K the linear kernel of
    the L2-normalised rows.  Deliberately CPU, float64."""
    from scipy import linalg
    a = _host(_check_matrix(x, "x"))
    norm = np.sqrt((a * a).sum(axis=1, keepdims=True))
    a = a / np.where(norm == 0.0, 1.0, norm)
    w = linalg.eigvalsh(a @ a.T / a.shape[0])
    w = w[w > 0]
    return float(np.exp(-(w * np.log(w)).sum()))


def vendi_per_class(gen, labels) -> np.ndarray:
    """vendi() of the rows of every class 0 .. C-1, C = the number of distinct labels (the reference's per-class loop)."""
    gen = _check_matrix(gen, "gen")
    lab = np.asarray(labels.cpu() if isinstance(labels, torch.Tensor) else labels)
    if lab.ndim != 1 or lab.shape[0] != gen.shape[0]:
        raise ValueError(f"labels: expected {gen.shape[0]} labels, got shape {lab.shape}")
    a = _host(gen)
    classes = len(np.unique(lab))
    out = np.zeros(classes)
    for c in range(classes):
        rows = a[lab == c]
        if rows.shape[0] == 0:
            raise ValueError(f"labels: class {c} of {classes} is empty (labels must be 0 .. C-1)")
        out[c] = vendi(rows)
    return out


def compute_scores(real, gen, labels=None, metrics: Sequence[str] = ("prdc", "vendi", "fd", "kd", "authpct"), nearest_k: int = 5,
                   reduced_n: int = 10000, rng=None) -> dict:
    """The reference's record (its compute_scores, with its key names) for the requested metrics: fd; kd_value / kd_variance (mean
    and standard deviation of the subset values); precision / recall / density / coverage on reduced_n rows of each set drawn
    without replacement; mean / std vendi per class (needs labels of the generated set); authpct."""
    known = {"prdc", "vendi", "fd", "kd", "authpct"}
    unknown = set(metrics) - known
    if unknown:
        raise ValueError(f"unknown metric(s) {sorted(unknown)}; this module has {sorted(known)}")
    real, gen = _check_pair(real, gen)
    if "vendi" in metrics and labels is None:
        raise ValueError("'vendi' is per class and needs the labels of the generated set (or leave it out of metrics)")
    if "prdc" in metrics:
        n = min(reduced_n, real.shape[0], gen.shape[0])
        if n <= nearest_k:
            raise ValueError(f"prdc on {n} rows per set with nearest_k = {nearest_k}")
        if nearest_k + 1 > MAX_KTH:
            raise ValueError(f"nearest_k + 1 = {nearest_k + 1} > {MAX_KTH}")
    rng = np.random.default_rng() if rng is None else rng
    dev = _device_of(real, gen)
    gpu = bool({"prdc", "kd", "authpct"} & set(metrics))
    r, g = (_upload(real, dev), _upload(gen, dev)) if gpu else (real, gen)
    scores: dict = {}
    if "fd" in metrics:
        scores["fd"] = fd(real, gen)
    if "kd" in metrics:
        values = kd(r, g, rng=rng)
        scores["kd_value"], scores["kd_variance"] = float(values.mean()), float(values.std())
    if "prdc" in metrics:
        i0 = torch.from_numpy(rng.choice(real.shape[0], n, replace=False)).to(dev)
        i1 = torch.from_numpy(rng.choice(gen.shape[0], min(gen.shape[0], n), replace=False)).to(dev)
        scores.update(prdc(r[i0], g[i1], nearest_k))
    if "vendi" in metrics:
        per_class = vendi_per_class(gen, labels)
        scores["mean vendi per class"], scores["std vendi per class"] = float(per_class.mean()), float(per_class.std())
    if "authpct" in metrics:
        scores["authpct"] = authpct(r, g)
    return scores
