"""The test matrix of the all-pairs metric kernels (csrc/idb_pair.hip: idb_pair_dist2, idb_pair_knn_radii, idb_pair_prdc_counts,
idb_pair_nearest, idb_pair_poly_sums), shared by test_pair_matrix_cpu.py (conditions on the inputs, teeth, argument checks) and
test_pair_matrix_gpu.py (launch through the C ABI + compare): cases, input recipes, the float64 references of tests/metrics_oracle.py, an
fp32 restatement of the kernels, injectable defects and the criteria (the verdict `within` is matrix_common.py's).  numpy only, no GPU.

Criteria (every number is metrics_oracle's or follows from the arithmetic, none was tuned):

  distances  |got - float64| <= TAU * scale, TAU = 4e-6 (metrics_oracle.TAU), scale = |a - s|^2 + |b - s|^2 with s the shift actually
             passed (0 when it is NULL).  Every case has D <= 65.  Condition on the inputs (CPU half): the fp32 restatement of the expansion
             stays at or below TAU / 4 on every case, the 4x headroom the figure was derived with.  The first neighbour of a point within
             its own set is the point itself: exactly 0.
  decisions  PRDC counts, `covered`, coverage and argmin: wherever float64's gap exceeds TAU * scale the result must be float64's, by the
             bracketing lo <= inside <= hi of test_metrics_gpu.test_prdc_counts.  The radii the count kernel is given are the float64
             radii rounded to fp32 (a relative 6e-8 of a distance that is at most 2 * scale: inside the headroom), so a count depends on
             the count kernel alone.  Undecided comparisons are at most UNDECIDED_CAP = 1e-3 of a case and of its authenticity columns
             (CPU half).
  integers   small integer coordinates make every product and partial sum exact in fp32 (asserted: every intermediate below 2^24), so the
             float64 answer must come back bit for bit, ties and their lowest index included.

The restatement follows the kernels' structure, not only their arithmetic: 128-row blocks; splits = min(blocks, 8), split s takes blocks
s, s + 8, ...; two half-wave lists per split, half h of a block owning the rows with (row mod 8) / 4 == h (tile_row) in ascending order;
an 8-entry insertion list kept with multiplicity; the merge over all 2 * splits lists in list order; the values from the fp32 expansion
(k-ordered fused multiply-adds for the dot product; the norms as pair_norms_kernel forms them, a chain per lane over columns l, l + 64,
... and the wave's xor butterfly over the 64 lanes, because a norm formed in k order would equal the dot product of a row with itself
bit for bit and hide a diagonal that is not forced to 0; (na + nb) - 2 dot, clamped at 0).  DEFECTS lists what is
injected into it on the CPU and DEFECT_CASES the case and mode each one must fail under the criteria above.  HARMLESS is empty: the
only candidate was the zero fill of the rows past the end taken before the shift (they would hold -shift), which every epilogue masks by
index; the defect kept instead, `pad_minus_shift`, puts the last shift element into the K columns between D and the end of the 32-wide
stage of both operands, which every dot product sees."""
from dataclasses import dataclass
from functools import lru_cache
from typing import Callable, Dict, Optional, Tuple

import numpy as np

import metrics_oracle as O
from matrix_common import F32, GUARD, NAN32, NAN64, within  # noqa: F401  (re-exported to the two test files)

TAU = O.TAU
UNDECIDED_CAP = O.UNDECIDED_CAP
PT = 128                              # rows of a block
PK = 32                               # K per stage
MAX_SPLITS = 8
KNN_MAX = 8
INT_MAX = 0x7FFFFFFF
INF_BITS = 0x7F800000


# ---- cases -----------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    name: str
    nr: int
    ng: int
    d: int
    seed: int = 3
    ks: Tuple[int, ...] = (1, 5, 7)   # nearest_k of the PRDC runs
    noshift: bool = False             # also run the distance modes with a NULL shift


CASES = (
    Case("loop9", 1025, 130, 12),                     # 9 row blocks: split 0 takes a second pass that holds one row
    Case("loop18_scalar", 2200, 2100, 10, seed=4, ks=(5,)),   # 18 blocks: splits 0, 1 take 3 passes, the rest 2; scalar loads
    Case("wide", 33, 300, 40, noshift=True),          # ng > nr, two K stages with a tail of 8
    Case("wide_loop", 129, 1153, 34),                 # ng > nr, 10 column blocks; the gen set's k-nearest loops; scalar, tail of 2
    Case("tail33", 150, 140, 33, noshift=True),       # one element over a stage, scalar
    Case("tail5", 150, 140, 5, noshift=True),         # a partial 4-group
    Case("tail3", 150, 140, 3),                       # d < 4
    Case("tiny", 9, 7, 4, ks=(1, 5)),                 # n <= 8 for gen: the candidate list still holds +inf
    Case("edge127", 127, 129, 8, seed=5),             # 127 / 128 / 129 as the row set and as the column set; seed 3 leaves one
    Case("edge128", 128, 127, 8, seed=5),             # authenticity column of edge127 undecided, seeds 5, 6 and 10 none anywhere
    Case("edge129", 129, 128, 8, seed=5),
)
BY_NAME = {c.name: c for c in CASES}
MISALIGNED = ("wide", "loop9")        # d = 40 and d = 12: the vector path until one pointer is 4 bytes past a 16-byte boundary
DEGENERATE_KNN = ((1, 1), (2, 2), (8, 8))             # (n, kth)
POLY_CASES = ((300, 280, 5, 2, 3), (300, 280, 5, 127, 2), (300, 280, 8, 128, 2), (300, 280, 33, 129, 5), (400, 300, 5, 300, 1))
KD_CHUNK = dict(nx=40, ny=30, d=4, m=2, subsets=4100)  # metrics.kd: the second chunk of the 4096-subset step


@lru_cache(maxsize=None)
def inputs(name: str):
    """(real, gen, shift fp32 = the float64 mean of real rounded, as metrics._centre forms it)."""
    c = BY_NAME[name]
    real, gen = O.fixture(c.nr, c.ng, c.d, c.seed)
    return real, gen, real.astype(np.float64).mean(axis=0).astype(F32)


def shift64(shift, d: int) -> np.ndarray:
    return np.zeros(d) if shift is None else np.asarray(shift, np.float64)


@lru_cache(maxsize=None)
def dist2_ref(name: str, shifted: bool = True):
    real, gen, mu = inputs(name)
    return O.dist2(real, gen), O.scale(real, gen, shift64(mu if shifted else None, real.shape[1]))


@lru_cache(maxsize=None)
def prdc_ref(name: str, k: int) -> O.Prdc:
    real, gen, _ = inputs(name)
    return O.Prdc(real, gen, k)


@lru_cache(maxsize=None)
def auth_ref(name: str) -> O.Auth:
    real, gen, _ = inputs(name)
    return O.Auth(real, gen)


@lru_cache(maxsize=None)
def _knn_table(name: str, which: str):
    real, gen, _ = inputs(name)
    x = real if which == "real" else gen
    return O.knn_table(x, min(KNN_MAX, len(x)))


def knn_ref(name: str, which: str, kth: int, shifted: bool = True):
    """(radii, scale of each radius) of the real or the gen set of a case, float64: O.knn_radii_scale from one sort per set."""
    real, gen, mu = inputs(name)
    x = real if which == "real" else gen
    radii, nbr = _knn_table(name, which)
    nrm = O.sq_norms(x, shift64(mu if shifted else None, x.shape[1]))
    return radii[:, kth - 1], nrm + nrm[nbr[:, kth - 1]]


@lru_cache(maxsize=None)
def nearest_ref(name: str, shifted: bool) -> Tuple[O.Nearest, O.Nearest]:
    """(real x real without the diagonal, real x gen) on the scale of the shift passed."""
    if shifted:
        a = auth_ref(name)
        return a.rr, a.rg
    real, gen, _ = inputs(name)
    z = np.zeros(real.shape[1])
    return O.Nearest(real, real, z, exclude_diag=True), O.Nearest(real, gen, z)


@lru_cache(maxsize=None)
def degenerate_inputs(n: int):
    real, _ = O.fixture(8, 2, 4)
    x = np.ascontiguousarray(real[:n])
    return x, x.astype(np.float64).mean(axis=0).astype(F32)


@lru_cache(maxsize=None)
def ties_inputs():
    """Integer coordinates in -3..3: `a` (2200, 6) with a[3] copied one pass later in its own split (1027), into another split (130) and
    into the last block (2199); `b` (260, 6) with b[7] = a[3]."""
    rng = np.random.default_rng(9)
    a = rng.integers(-3, 4, size=(2200, 6)).astype(F32)
    for r in (1027, 130, 2199):
        a[r] = a[3]
    b = rng.integers(-3, 4, size=(260, 6)).astype(F32)
    b[7] = a[3]
    return a, b


@lru_cache(maxsize=None)
def poly_inputs(case):
    """(x, y, idx_x, idx_y) of a polynomial-sum case: integer features in -1..1; subset 0 in descending order, the last subset holds rows
    nx - 1 and ny - 1 (when there is one subset it does both)."""
    nx, ny, d, m, s = case
    rng = np.random.default_rng(100 + d + m)
    x = rng.integers(-1, 2, size=(nx, d)).astype(F32)
    y = rng.integers(-1, 2, size=(ny, d)).astype(F32)
    ix = np.stack([rng.choice(nx, m, replace=False) for _ in range(s)]).astype(np.int32)
    iy = np.stack([rng.choice(ny, m, replace=False) for _ in range(s)]).astype(np.int32)
    for idx, n in ((ix, nx), (iy, ny)):
        if n - 1 not in idx[-1]:
            idx[-1, 0] = n - 1
        idx[0] = np.sort(idx[0])[::-1]
    return x, y, ix, iy


@lru_cache(maxsize=None)
def kd_chunk_inputs():
    c = KD_CHUNK
    rng = np.random.default_rng(77)
    x = rng.integers(-1, 2, size=(c["nx"], c["d"])).astype(F32)
    y = rng.integers(-1, 2, size=(c["ny"], c["d"])).astype(F32)
    ix = np.stack([rng.choice(c["nx"], c["m"], replace=False) for _ in range(c["subsets"])])
    iy = np.stack([rng.choice(c["ny"], c["m"], replace=False) for _ in range(c["subsets"])])
    return x, y, ix, iy


def poly_reference(x, y, ix, iy, gamma=1.0, coef0=1.0) -> np.ndarray:
    return np.stack([O.poly_sums(x[a], y[b], gamma, coef0)[0] for a, b in zip(ix, iy)])


# ---- the fp32 arithmetic ---------------------------------------------------------------------------------------------------------------
def fma32(a, b, c):
    """fp32 fused multiply-add: the product of two fp32 values is exact in float64."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F32)


def splits_of(n: int) -> int:
    return min((n + PT - 1) // PT, MAX_SPLITS)


def passes_of(n: int, defect: Optional[str] = None):
    """Per split, the row blocks it walks, in order."""
    blocks = (n + PT - 1) // PT
    out = [list(range(s, blocks, splits_of(n))) for s in range(splits_of(n))]
    if defect == "drop_last_pass":
        out = [p[:-1] if len(p) > 1 else p for p in out]
    return out


def half_rows(h: int) -> np.ndarray:
    """Block-local rows of half-wave h in the order a lane meets them: tile_row(t, reg, h), t and reg ascending."""
    return np.array([t * 32 + (r & 3) + 8 * (r >> 2) + 4 * h for t in range(4) for r in range(16)])


def staged(x, shift, vec: bool, defect: Optional[str]) -> np.ndarray:
    """The operand as pair_fetch stages it: x - shift in fp32, K padded with zeros to the 32-wide stage."""
    x = np.asarray(x, F32)
    n, d = x.shape
    use = shift is not None and not (defect == "scalar_no_shift" and not vec)
    out = np.zeros((n, -(-d // PK) * PK), F32)
    out[:, :d] = x - np.asarray(shift, F32)[None, :] if use else x
    if defect == "pad_minus_shift" and use:
        out[:, d:] = -F32(shift[-1])
    return out


def row_norms(x, shift) -> np.ndarray:
    x = np.asarray(x, F32)
    v = x - np.asarray(shift, F32)[None, :] if shift is not None else x
    lanes = np.zeros((x.shape[0], 64), F32)            # lane l takes columns l, l + 64, ...: a fused multiply-add chain per lane
    for k in range(x.shape[1]):
        lanes[:, k % 64] = fma32(v[:, k], v[:, k], lanes[:, k % 64])
    for o in (32, 16, 8, 4, 2, 1):                     # wave_sum: the xor butterfly, every lane ends with the same sum
        lanes = (lanes + lanes[:, np.arange(64) ^ o]).astype(F32)
    return lanes[:, 0].copy()


def dots(sa: np.ndarray, sb: np.ndarray) -> np.ndarray:
    acc = np.zeros((sa.shape[0], sb.shape[0]), F32)
    for k in range(sa.shape[1]):
        acc = fma32(sa[:, k, None], sb[None, :, k], acc)
    return acc


def dist2_of(na, nb, dot) -> np.ndarray:
    d = (na + nb).astype(F32) - (F32(2) * dot).astype(F32)
    return np.where(d > 0, d, F32(0)).astype(F32)


class Engine:
    """dot products and norms of a x b as the tile engine forms them, and the distance a workgroup computes for a row it meets in one of
    its passes (the norm comes from sN, which a defect may leave stale)."""

    def __init__(self, a, b, shift, vec: Optional[bool] = None, defect: Optional[str] = None):
        a, b = np.asarray(a, F32), np.asarray(b, F32)
        self.na, self.nb, self.defect = a.shape[0], b.shape[0], defect
        vec = a.shape[1] % 4 == 0 if vec is None else vec
        self.dot = dots(staged(a, shift, vec, defect), staged(b, shift, vec, defect))
        self.norm_a, self.norm_b = row_norms(a, shift), row_norms(b, shift)

    def all(self) -> np.ndarray:
        return dist2_of(self.norm_a[:, None], self.norm_b[None, :], self.dot)

    def row(self, i: int, first_block: int) -> np.ndarray:
        """d2 of row i against every column, met by a workgroup whose first pass was block `first_block`.  A row past the end is zero
        after the shift and its norm is loaded as 0: its distance is the column's norm."""
        if i >= self.na:
            return dist2_of(F32(0), self.norm_b, np.zeros(self.nb, F32))
        src = i
        if self.defect == "stale_norms":
            src = first_block * PT + i % PT
        na = self.norm_a[src] if src < self.na else F32(0)
        return dist2_of(na, self.norm_b, self.dot[i])


def emulate_dist2(a, b, shift, vec=None, defect=None) -> np.ndarray:
    return Engine(a, b, shift, vec, defect).all()


def knn_insert(L: np.ndarray, v: np.ndarray, defect: Optional[str] = None) -> np.ndarray:
    """knn_insert over every column at once: L [n][8] ascending, v [n]; v goes behind its equals and the last entry falls out."""
    ok = v < L[:, -1]
    if defect == "list_dedupe":
        ok &= ~(L == v[:, None]).any(axis=1)
    pos = (L <= v[:, None]).sum(axis=1)
    idx = np.arange(KNN_MAX)[None, :]
    moved = np.concatenate([L[:, :1], L[:, :-1]], axis=1)
    new = np.where(idx < pos[:, None], L, np.where(idx == pos[:, None], v[:, None], moved))
    return np.where(ok[:, None], new, L)


def emulate_knn_lists(x, shift, vec=None, defect=None) -> np.ndarray:
    """[2 * splits][n][8]: the candidate list of every half-wave."""
    eng = Engine(x, x, shift, vec, defect)
    n = eng.na
    cols = np.arange(n)
    lists = np.full((2 * splits_of(n), n, KNN_MAX), np.inf, F32)
    for s, blocks in enumerate(passes_of(n, defect)):
        for h in (0, 1):
            L = lists[2 * s + h]
            for mb in blocks:
                for i in mb * PT + half_rows(h):
                    if i >= n and defect != "no_row_mask":
                        continue
                    v = eng.row(i, blocks[0])
                    if defect != "diag_first_pass" or mb == blocks[0]:
                        v = np.where(cols == i, F32(0), v)
                    L = knn_insert(L, v, defect)
            lists[2 * s + h] = L
    return lists


def emulate_knn_merge(lists: np.ndarray, kth: int, defect=None) -> np.ndarray:
    count = lists.shape[0] // 2 if defect == "merge_half" else lists.shape[0]
    L = np.full(lists.shape[1:], np.inf, F32)
    for s in range(count):
        for e in range(KNN_MAX):
            L = knn_insert(L, lists[s, :, e], defect)
    return L[:, kth - 1].copy()


def emulate_knn(x, shift, kth: int, vec=None, defect=None) -> np.ndarray:
    return emulate_knn_merge(emulate_knn_lists(x, shift, vec, defect), kth, defect)


def emulate_nearest(a, b, shift, exclude_diag: bool, vec=None, defect=None):
    """(min_d2 fp32 [nb], argmin int32 [nb]) through the per-half-wave (best, index) pairs and their merge."""
    eng = Engine(a, b, shift, vec, defect)
    na, nb = eng.na, eng.nb
    cols = np.arange(nb)
    lists = 2 * splits_of(na)
    ws_min, ws_idx = np.full((lists, nb), np.inf, F32), np.full((lists, nb), INT_MAX, np.int64)
    for s, blocks in enumerate(passes_of(na, defect)):
        for h in (0, 1):
            best, bi = ws_min[2 * s + h], ws_idx[2 * s + h]
            for mb in blocks:
                for il in half_rows(h):
                    i = mb * PT + il
                    if i >= na and defect != "no_row_mask":
                        continue
                    d = eng.row(i, blocks[0])
                    ok = (d <= best) if defect == "tie_le" else ((d < best) | ((d == best) & (i < bi)))
                    if exclude_diag:
                        ok &= cols != (il if defect == "excl_local" else i)
                    best, bi = np.where(ok, d, best), np.where(ok, i, bi)
            ws_min[2 * s + h], ws_idx[2 * s + h] = best, bi
    best, bi = np.full(nb, np.inf, F32), np.full(nb, INT_MAX, np.int64)
    for s in range(lists // 2 if defect == "merge_half" else lists):
        d, i = ws_min[s], ws_idx[s]
        ok = (i != INT_MAX) & ((d <= best) if defect == "tie_le" else ((d < best) | ((d == best) & (i < bi))))
        best, bi = np.where(ok, d, best), np.where(ok, i, bi)
    return best, np.where(bi == INT_MAX, -1, bi).astype(np.int32)


def emulate_prdc(real, gen, shift, r2_real, r2_gen, vec=None, defect=None):
    """(in_real_sphere int32 [ng], covered int32 [nr], row_min fp32 [nr]).  The counts and flags are integer atomics and the minimum an
    unsigned one on the bits: no order to restate.  What the init kernel does not reach keeps the guard pattern of a fresh buffer."""
    d = emulate_dist2(real, gen, shift, vec, defect)
    nr, ng = d.shape
    r2_real, r2_gen = np.asarray(r2_real, F32), np.asarray(r2_gen, F32)
    reach = min(nr, ng) if defect == "init_min" else max(nr, ng)
    inside = np.where(np.arange(ng) < reach, 0, NAN32).astype(np.int64) + (d < r2_real[:, None]).sum(axis=0)
    covered = np.where(np.arange(nr) < reach, 0, NAN32).astype(np.int64) | (d < r2_gen[None, :]).any(axis=1)
    bits = np.minimum(np.where(np.arange(nr) < reach, INF_BITS, NAN32).astype(np.uint32), d.min(axis=1).view(np.uint32))
    return inside.astype(np.int32), covered.astype(np.int32), bits.view(F32)


def emulate_poly(x, y, ix, iy, gamma=1.0, coef0=1.0, defect=None) -> np.ndarray:
    """float64 [S][3]: per 128 x 128 tile the fp32 sum of (gamma a.b + c0)^3, the tiles added in double in row-major order.  (On the
    integer cases every partial is exact, so the order within a tile is not restated.)"""
    s_count, m = ix.shape
    out = np.zeros((s_count, 3))
    i, j = np.arange(m)[:, None], np.arange(m)[None, :]
    for s in range(s_count):
        gx, gy = (ix[0], iy[0]) if defect == "gather_subset0" else (ix[s], iy[s])
        for which, (a, b) in enumerate(((x[gx], x[gx]), (y[gy], y[gy]), (x[gx], y[gy]))):
            v = fma32(F32(gamma), dots(staged(a, None, True, None), staged(b, None, True, None)), F32(coef0))
            k3 = ((v * v).astype(F32) * v).astype(F32)
            if which != 2:
                diag = (i == j) & ((i < PT) if defect == "poly_diag_tile0" else True)
                k3 = np.where(diag, F32(0), k3)
            total = 0.0
            for m0 in range(0, m, PT):
                for n0 in range(0, m, PT):
                    total += float(k3[m0:m0 + PT, n0:n0 + PT].sum(dtype=F32))
            out[s, which] = total
    return out


# ---- criteria --------------------------------------------------------------------------------------------------------------------------
def judge_dist2(what: str, got, want, scale) -> float:
    ratio = within(what, got, want, TAU * scale)
    assert (np.asarray(got) >= 0).all() and not np.signbit(got).any(), f"{what}: a negative distance or -0"
    return ratio


def judge_knn(what: str, got, want, scale, kth: int) -> float:
    ratio = within(what, got, want, TAU * scale)
    if kth == 1:
        bad = np.flatnonzero(np.asarray(got).view(np.uint32) != 0)
        assert bad.size == 0, f"{what}: the point itself must be exactly 0, query {int(bad[0])} has {got[bad[0]]!r}: error {got[bad[0]]:.3e}, bound 0"
    return ratio


def judge_prdc(what: str, ref: O.Prdc, r2_real32, inside, covered, row_min) -> float:
    inside, covered = np.asarray(inside, np.int64), np.asarray(covered, np.int64)
    lo = (ref.in_sphere & ~ref.in_sphere_und).sum(axis=0)
    hi = lo + ref.in_sphere_und.sum(axis=0)
    bad = np.flatnonzero((inside < lo) | (inside > hi))
    assert bad.size == 0, f"{what}: in_real_sphere[{int(bad[0])}] = {int(inside[bad[0]])}, float64 decides {int(lo[bad[0]])}..{int(hi[bad[0]])}"
    sure = (ref.in_gen & ~ref.in_gen_und).any(axis=1)
    maybe = sure | ref.in_gen_und.any(axis=1)
    bad = np.flatnonzero(~np.isin(covered, (0, 1)) | (sure & (covered != 1)) | (~maybe & (covered != 0)))
    assert bad.size == 0, f"{what}: covered[{int(bad[0])}] = {int(covered[bad[0]])}, float64 decides {int(sure[bad[0]])}..{int(maybe[bad[0]])}"
    ratio = within(f"{what} row_min", row_min, ref.row_min, TAU * ref.scale[np.arange(ref.nr), ref.row_arg])
    cov = np.asarray(row_min, F32) < np.asarray(r2_real32, F32)
    bad = np.flatnonzero((cov != ref.cov) & ~ref.cov_und)
    assert bad.size == 0, (f"{what}: coverage of row {int(bad[0])} is {bool(cov[bad[0]])}, float64 has row_min {ref.row_min[bad[0]]!r} against "
                           f"r2 {ref.r2_real[bad[0]]!r}")
    return ratio


def judge_nearest(what: str, ref: O.Nearest, mins, args, na: int, exclude_diag: bool) -> float:
    args = np.asarray(args, np.int64)
    ratio = within(f"{what} min", mins, ref.min, TAU * ref.scale)
    bad = np.flatnonzero((args < 0) | (args >= na))
    assert bad.size == 0, f"{what}: argmin[{int(bad[0])}] = {int(args[bad[0]])} outside 0..{na - 1}"
    bad = np.flatnonzero((args != ref.arg) & ref.decided)
    assert bad.size == 0, f"{what}: argmin[{int(bad[0])}] = {int(args[bad[0]])}, float64 decides {int(ref.arg[bad[0]])}"
    if exclude_diag:
        bad = np.flatnonzero(args == np.arange(len(args)))
        assert bad.size == 0, f"{what}: argmin[{int(bad[0])}] is the excluded diagonal"
    return ratio


def judge_auth(what: str, ref: O.Auth, rr_min, rg_min, rg_arg) -> None:
    """The authenticity decision metrics.authpct takes on the host from the two nearest-neighbour results."""
    authentic = np.asarray(rr_min, F32)[np.asarray(rg_arg, np.int64)] < np.asarray(rg_min, F32)
    bad = np.flatnonzero((authentic != ref.authentic) & ~ref.und)
    assert bad.size == 0, f"{what}: authenticity of column {int(bad[0])} is {bool(authentic[bad[0]])}, float64 decides otherwise"


def judge_exact(what: str, got, want) -> float:
    """Integer cases: the float64 answer, as values (both are exact): a bound of 0."""
    return within(what, got, want, 0.0)


def exact_dist_precondition(a, b) -> float:
    """The largest intermediate of the expansion of an integer case: |a|^2 + |b|^2 + 2 sum |a_k b_k| (exact in fp32 below 2^24)."""
    a, b = np.abs(np.asarray(a, np.float64)), np.abs(np.asarray(b, np.float64))
    return float((a * a).sum(1).max() + (b * b).sum(1).max() + 2 * (a @ b.T).max())


def exact_poly_precondition(case) -> float:
    """The largest fp32 intermediate of a polynomial case: a whole tile's sum of |k|, |k| <= (d + 1)^3 reached at most."""
    x, y, ix, iy = poly_inputs(case)
    worst = 0.0
    for s in range(ix.shape[0]):
        for a, b in ((x[ix[s]], x[ix[s]]), (y[iy[s]], y[iy[s]]), (x[ix[s]], y[iy[s]])):
            k = np.abs(a.astype(np.float64) @ b.astype(np.float64).T + 1.0) ** 3
            worst = max(worst, max(k[m0:m0 + PT, n0:n0 + PT].sum() for m0 in range(0, len(a), PT) for n0 in range(0, len(a), PT)))
    return worst


# ---- the whole matrix through any implementation ---------------------------------------------------------------------------------------
class Restated:
    """The five entries as the restatement computes them, with one optional defect; test_pair_matrix_gpu.py has the same five methods
    over the C ABI."""

    def __init__(self, defect: Optional[str] = None):
        self.defect = defect

    def dist2(self, a, b, shift):
        return emulate_dist2(a, b, shift, None, self.defect)

    def knn(self, x, shift, kths):
        lists = emulate_knn_lists(x, shift, None, self.defect)
        return {kth: emulate_knn_merge(lists, kth, self.defect) for kth in kths}

    def prdc(self, real, gen, shift, r2_real, r2_gen):
        return emulate_prdc(real, gen, shift, r2_real, r2_gen, None, self.defect)

    def nearest(self, a, b, shift, exclude_diag):
        return emulate_nearest(a, b, shift, exclude_diag, None, self.defect)

    def poly(self, x, y, ix, iy, gamma=1.0):
        return emulate_poly(x, y, ix, iy, gamma, 1.0, self.defect)


MODES = ("dist2", "knn", "prdc", "nearest", "poly")


def run_real_case(impl, name: str, mode: str, note: Callable = lambda *a: None) -> None:
    """One mode of one real-valued case through `impl` under the criteria; note(mode, worst err / (TAU * scale), what)."""
    c = BY_NAME[name]
    real, gen, mu = inputs(name)
    for shifted in ((True, False) if c.noshift else (True,)):
        shift, tag = (mu, "") if shifted else (None, " no shift")
        if mode == "dist2":
            want, scale = dist2_ref(name, shifted)
            what = f"{name} dist2{tag}"
            note(mode, judge_dist2(what, impl.dist2(real, gen, shift), want, scale), what)
        elif mode == "knn":
            for which, x in (("real", real), ("gen", gen)):
                kths = tuple(range(1, min(KNN_MAX, len(x)) + 1)) if name == "tiny" else tuple(sorted({1} | {k + 1 for k in c.ks}))
                got = impl.knn(x, shift, kths)
                for kth in kths:
                    what = f"{name} knn {which} kth {kth}{tag}"
                    note(mode, judge_knn(what, got[kth], *knn_ref(name, which, kth, shifted), kth), what)
        elif mode == "nearest":
            rr, rg = nearest_ref(name, shifted)
            m_rr, a_rr = impl.nearest(real, real, shift, True)
            m_rg, a_rg = impl.nearest(real, gen, shift, False)
            note(mode, judge_nearest(f"{name} nearest real x real{tag}", rr, m_rr, a_rr, c.nr, True), name)
            note(mode, judge_nearest(f"{name} nearest real x gen{tag}", rg, m_rg, a_rg, c.nr, False), name)
            if shifted:
                judge_auth(f"{name} authenticity", auth_ref(name), m_rr, m_rg, a_rg)
        elif mode == "prdc" and shifted:
            for k in c.ks:
                ref = prdc_ref(name, k)
                r2r, r2g = ref.r2_real.astype(F32), ref.r2_gen.astype(F32)
                what = f"{name} prdc k {k}"
                note(mode, judge_prdc(what, ref, r2r, *impl.prdc(real, gen, shift, r2r, r2g)), what)


def run_degenerate(impl, note: Callable = lambda *a: None) -> None:
    for n, kth in DEGENERATE_KNN:
        x, mu = degenerate_inputs(n)
        got = impl.knn(x, mu, (kth,))[kth]
        what = f"degenerate knn n {n} kth {kth}"
        note("knn", judge_knn(what, got, *O.knn_radii_scale(x, kth, mu.astype(np.float64)), kth), what)
        if n == 1:
            assert got.view(np.uint32)[0] == 0, f"{what}: {got[0]!r}, exactly 0 expected: error {got[0]:.3e}, bound 0"
    x, mu = degenerate_inputs(2)
    mins, args = impl.nearest(x, x, mu, True)
    assert args.tolist() == [1, 0], f"degenerate nearest 2 x 2 without the diagonal: argmin {args.tolist()}, expected [1, 0]"
    d = O.dist2(x, x)[0, 1]
    note("nearest", within("degenerate nearest 2 x 2", mins, [d, d], TAU * O.scale(x, x, mu.astype(np.float64))[0, 1] * np.ones(2)), "degenerate")


def run_ties(impl, which: str, note: Callable = lambda *a: None) -> None:
    """The integer cases: `forward`, `reversed` and `exclude` of ties_loop, and knn_ties_loop."""
    a, b = ties_inputs()
    if which == "knn":
        got = impl.knn(a, None, tuple(range(1, KNN_MAX + 1)))
        for kth in range(1, KNN_MAX + 1):
            note("knn", judge_exact(f"knn_ties_loop kth {kth}", got[kth], O.knn_radii(a, kth)), "knn_ties_loop")
        return
    if which == "exclude":
        d = O.dist2(a, a)
        np.fill_diagonal(d, np.inf)
        rows, cols = a, a
    else:
        rows = {"forward": a, "reversed": np.ascontiguousarray(a[::-1]), "swapped": ties_swapped()}[which]
        cols, d = b, O.dist2(rows, b)
    mins, args = impl.nearest(rows, cols, None, which == "exclude")
    note("nearest", judge_exact(f"ties_loop {which} min", mins, d.min(axis=0)), "ties_loop")
    judge_exact(f"ties_loop {which} argmin", args, d.argmin(axis=0))          # numpy's argmin is the first = lowest index
    first = {"forward": 3, "reversed": 0, "swapped": 130}                      # a[2199] is row 0 of the reversed set
    assert which not in first or args[7] == first[which], f"ties_loop {which}: argmin[7] = {int(args[7])}, the lowest copy is row {first[which]}"


def ties_swapped() -> np.ndarray:
    """ties_loop's `a` with rows 3 and 900 exchanged: the copies are rows 130 (list 2), 900 (list 15), 1027 (list 0) and 2199 (list 3),
    so the merge meets the lowest index after a higher one at the same distance."""
    a = ties_inputs()[0].copy()
    a[[3, 900]] = a[[900, 3]]
    return a


def run_poly(impl, case, note: Callable = lambda *a: None) -> None:
    x, y, ix, iy = poly_inputs(case)
    what = f"poly {case}"
    note("poly", judge_exact(what, impl.poly(x, y, ix, iy), poly_reference(x, y, ix, iy)), what)


# ---- teeth -----------------------------------------------------------------------------------------------------------------------------
DEFECTS: Dict[str, str] = {
    "drop_last_pass": "a split that has more than one pass leaves its last one out (`mb + splits` handled once instead of the loop)",
    "stale_norms": "sN keeps the norms of the split's first block in every later pass",
    "diag_first_pass": "the k-nearest diagonal is forced to 0 only in a split's first pass",
    "excl_local": "exclude_diag is tested against the block-local row",
    "tie_le": "ties are taken on <=, so the highest index wins",
    "merge_half": "the merges read `splits` lists instead of 2 * splits",
    "list_dedupe": "the candidate list drops a value it already holds",
    "scalar_no_shift": "the scalar load path ignores `shift` (the norms still subtract it)",
    "pad_minus_shift": "the K columns between D and the end of the stage hold -shift (its last element) instead of 0",
    "no_row_mask": "rows past n are not masked in the last block",
    "init_min": "the PRDC init covers min(nr, ng) elements",
    "poly_diag_tile0": "the polynomial diagonal is excluded only in tile (0, 0)",
    "gather_subset0": "the gather uses subset 0's indices for every subset",
}
HARMLESS: Tuple[str, ...] = ()
# defect -> (runner, arguments): the smallest named case whose criteria it must fail
DEFECT_CASES: Dict[str, Tuple] = {
    "drop_last_pass": (run_real_case, "loop9", "knn"),            # row 1024 is its own first neighbour only in the dropped pass
    "stale_norms": (run_ties, "forward"),
    "diag_first_pass": (run_real_case, "wide_loop", "knn"),       # 129 queries of the gen set meet themselves in a second pass
    "excl_local": (run_ties, "exclude"),
    "tie_le": (run_ties, "forward"),
    "merge_half": (run_ties, "knn"),
    "list_dedupe": (run_ties, "knn"),
    "scalar_no_shift": (run_real_case, "tail33", "dist2"),
    "pad_minus_shift": (run_real_case, "tail33", "dist2"),
    "no_row_mask": (run_real_case, "loop9", "knn"),
    "init_min": (run_real_case, "wide", "prdc"),
    "poly_diag_tile0": (run_poly, POLY_CASES[3]),
    "gather_subset0": (run_poly, POLY_CASES[0]),
}


def defect_fails(defect: str) -> Optional[str]:
    """The criterion's message when the defect fails its named case, None when it passes."""
    runner, *args = DEFECT_CASES[defect]
    try:
        runner(Restated(defect), *args)
    except AssertionError as e:
        return str(e) or "assertion"
    return None
