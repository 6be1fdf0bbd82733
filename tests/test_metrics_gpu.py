"""The idb_pair_* kernels and faceposegenerator_amd/metrics.py on the GPU against tests/metrics_oracle.py (float64, distances by direct
differences).

Bounds.  The kernels form d2 = |a - mu|^2 + |b - mu|^2 - 2 (a - mu).(b - mu) in fp32 on the f32-input MFMA, which is a k-ordered fmaf
chain: about 1.5e-7 of sum |a_k b_k| per dot product at K <= 1024.  The expansion has the cross term twice and two norms of the same
kind, and sum |a_k b_k| <= (|a|^2 + |b|^2) / 2, so the error is a small multiple of 1e-7 of scale = |a - mu|^2 + |b - mu|^2; a numpy
float32 emulation of the expansion gave 4.2e-7, 4.7e-7 and 1.1e-6 of that scale at the three shapes below.  TAU = 4e-6 is that with
about 4x headroom and is used for every distance here.  A hard comparison d2 < r2 whose float64 gap is at most TAU * scale is
*undecided* (float64 itself is within round-off of the threshold): decided comparisons must agree with float64 exactly, undecided
ones are left out and may be at most 0.1 % of a case's comparisons.  The kernel sums of KD are three rounded operations on such a dot
product: 5e-6 of the float64 sum of |k| over the matrix.

Every test prints the figure it measured before it asserts."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import metrics_oracle as O  # noqa: E402

from faceposegenerator_amd import metrics as M  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TAU = O.TAU
KSUM = 5e-6
SHAPES = [(200, 168, 72), (333, 257, 96), (520, 400, 384)]
EDGE = (65, 33, 8)                  # one row over a 32-row MFMA tile and one column over it
ALL_SHAPES = SHAPES + [EDGE]
ids = lambda s: "x".join(map(str, s))  # noqa: E731


@functools.lru_cache(maxsize=None)
def data(shape):
    return O.fixture(*shape)


@functools.lru_cache(maxsize=None)
def dev(shape):
    real, gen = data(shape)
    r, g = torch.from_numpy(real).to(DEV), torch.from_numpy(gen).to(DEV)
    return r, g, r.mean(dim=0, dtype=torch.float64).float().contiguous()


@functools.lru_cache(maxsize=None)
def mu64(shape):
    return data(shape)[0].astype(np.float64).mean(axis=0)


@functools.lru_cache(maxsize=None)
def prdc_ref(shape, k):
    return O.Prdc(*data(shape), k)


@functools.lru_cache(maxsize=None)
def auth_ref(shape):
    return O.Auth(*data(shape))


def n64(t):
    return t.cpu().numpy().astype(np.float64)


# ---- dist2 (store): pins the engine's numerics -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ALL_SHAPES + [(40, 50, 7), (130, 129, 1)], ids=ids)
def test_dist2_within_bound_with_and_without_shift(shape):
    real, gen = data(shape)
    r, g, mu = dev(shape)
    want = O.dist2(real, gen)
    got = n64(M.pair_dist2(r, g, mu))
    ratio = (np.abs(got - want) / O.scale(real, gen, mu64(shape))).max()
    zero = torch.zeros_like(mu)
    got0 = n64(M.pair_dist2(r, g, zero))
    ratio0 = (np.abs(got0 - want) / O.scale(real, gen, np.zeros(shape[2]))).max()
    # the centred result measured on the UNSHIFTED scale: what the shift buys, and that it is applied at all (see below)
    gain = (np.abs(got0 - want)).max() / max((np.abs(got - want)).max(), 1e-30)
    print(f"dist2 {ids(shape)}: max err / scale = {ratio:.3e} (shift = mean), {ratio0:.3e} (shift = 0); max abs err ratio {gain:.1f}")
    assert ratio <= TAU and ratio0 <= TAU
    assert (got >= 0).all() and (got0 >= 0).all()
    assert np.array_equal(n64(M.pair_dist2(r, g, None)), got0)            # NULL shift = zero shift, bit for bit
    # the shift is really subtracted: shifting by an arbitrary vector c gives exactly the distances of the pre-shifted operands
    # whenever a - c is exact in fp32 (integers here), which a kernel that ignored `shift` would not
    rng = np.random.default_rng(5)
    a = torch.from_numpy(rng.integers(-8, 9, size=(37, shape[2])).astype(np.float32)).to(DEV)
    b = torch.from_numpy(rng.integers(-8, 9, size=(70, shape[2])).astype(np.float32)).to(DEV)
    c = torch.from_numpy(rng.integers(-4, 5, size=(shape[2],)).astype(np.float32)).to(DEV)
    assert torch.equal(M.pair_dist2(a + c, b + c, c), M.pair_dist2(a, b, None))
    assert np.array_equal(n64(M.pair_dist2(a, b, None)), O.dist2(a.cpu().numpy(), b.cpu().numpy()))   # small integers: exact


# ---- knn radii ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 5, 7])
@pytest.mark.parametrize("shape", ALL_SHAPES, ids=ids)
def test_knn_radii(shape, k):
    real, gen = data(shape)
    r, g, mu = dev(shape)
    ref = prdc_ref(shape, k)
    worst = 0.0
    for x, xd, want in ((real, r, ref.r2_real), (gen, g, ref.r2_gen)):
        got = n64(M.pair_knn_radii(xd, mu, k + 1))
        again, scl = O.knn_radii_scale(x, k + 1, mu64(shape))
        assert np.array_equal(again, want)
        worst = max(worst, (np.abs(got - want) / scl).max())
        assert (np.abs(got - want) <= TAU * scl).all()
    print(f"knn radii {ids(shape)} k={k}: max err / scale = {worst:.3e}")
    first = n64(M.pair_knn_radii(r, mu, 1))
    assert (first == 0).all()                          # the point itself, forced to exactly 0


def test_knn_radii_with_duplicated_rows():
    shape = SHAPES[0]
    x = data(shape)[0].copy()
    x[50] = x[3]
    x[51] = x[3]
    x[120] = x[77]
    x[199] = x[0]                                      # a duplicate pair across two workgroups' row blocks
    xd = torch.from_numpy(x).to(DEV)
    mu = dev(shape)[2]
    for kth in (1, 2, 3, 4, 6, 8):
        want, scl = O.knn_radii_scale(x, kth, mu64(shape))
        assert np.array_equal(want, O.knn_radii(x, kth))
        got = n64(M.pair_knn_radii(xd, mu, kth))
        err = (np.abs(got - want) / scl).max()
        print(f"knn duplicates kth={kth}: max err / scale = {err:.3e}")
        assert err <= TAU
    # row 3 has itself and two copies at distance 0: its 4th smallest is the first real neighbour, and the diagonal counted once
    assert O.knn_radii(x, 3)[3] == 0 and O.knn_radii(x, 4)[3] > 0
    got4, got3 = n64(M.pair_knn_radii(xd, mu, 4)), n64(M.pair_knn_radii(xd, mu, 3))
    own = 2 * O.sq_norms(x, mu64(shape))[3]            # the scale of row 3 against a copy of itself
    assert got4[3] > 100 * TAU * own >= 100 * got3[3]


# ---- prdc counts -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,k", [(s, 5) for s in ALL_SHAPES] + [(SHAPES[0], 1), (SHAPES[1], 7)], ids=lambda v: ids(v) if isinstance(v, tuple) else f"k{v}")
def test_prdc_counts(shape, k):
    real, gen = data(shape)
    r, g, mu = dev(shape)
    ref = prdc_ref(shape, k)
    share = ref.undecided_share()
    print(f"prdc {ids(shape)} k={k}: undecided share {share:.2e}")
    assert share <= O.UNDECIDED_CAP                    # a condition on the test itself
    r2_real, r2_gen = M.pair_knn_radii(r, mu, k + 1), M.pair_knn_radii(g, mu, k + 1)
    inside, covered, row_min = M.pair_prdc_counts(r, g, mu, r2_real, r2_gen)
    inside, covered, row_min = inside.cpu().numpy(), covered.cpu().numpy(), n64(row_min)
    # in_real_sphere[j]: every decided-true comparison counted, nothing beyond the undecided ones
    lo = (ref.in_sphere & ~ref.in_sphere_und).sum(axis=0)
    hi = lo + ref.in_sphere_und.sum(axis=0)
    assert ((lo <= inside) & (inside <= hi)).all()
    # covered[i]
    sure = (ref.in_gen & ~ref.in_gen_und).any(axis=1)
    maybe = sure | ref.in_gen_und.any(axis=1)
    assert set(np.unique(covered)) <= {0, 1}
    assert (covered[sure] == 1).all() and (covered[~maybe] == 0).all()
    # row_min and coverage's comparison
    scl = ref.scale[np.arange(ref.nr), ref.row_arg]
    err = (np.abs(row_min - ref.row_min) / scl).max()
    print(f"prdc {ids(shape)} k={k}: row_min max err / scale = {err:.3e}")
    assert err <= TAU
    cov = row_min < n64(r2_real)
    assert (cov == ref.cov)[~ref.cov_und].all()
    # the four scalars, exactly, when float64 decides everything
    got = M.prdc(r, g, k)
    want = ref.scores()
    print(f"prdc {ids(shape)} k={k}: gpu {got} float64 {want}")
    if share == 0:
        nr, ng = ref.nr, ref.ng
        assert round(got["precision"] * ng) == round(want["precision"] * ng) and round(got["recall"] * nr) == round(want["recall"] * nr)
        assert round(got["density"] * k * ng) == round(want["density"] * k * ng)
        assert round(got["coverage"] * nr) == round(want["coverage"] * nr)
    if k == 5 and shape in SHAPES:
        assert share == 0                              # the fixture: all three shapes are compared exactly
    assert got == M.prdc(real, gen, k)                 # numpy input, uploaded once: the same numbers


# ---- nearest neighbour / AuthPct ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ALL_SHAPES, ids=ids)
def test_nearest_and_authpct(shape):
    real, gen = data(shape)
    r, g, mu = dev(shape)
    ref = auth_ref(shape)
    for name, (a, b, excl, want) in {"real x real, no diagonal": (r, r, True, ref.rr), "real x gen": (r, g, False, ref.rg)}.items():
        mins, args = M.pair_nearest(a, b, mu, excl)
        mins, args = n64(mins), args.cpu().numpy()
        err = (np.abs(mins - want.min) / want.scale).max()
        print(f"nearest {ids(shape)} {name}: min max err / scale = {err:.3e}; decided columns {want.decided.mean():.3f}")
        assert err <= TAU
        assert (args == want.arg)[want.decided].all()
        assert ((args >= 0) & (args < a.shape[0])).all()
        if excl:
            assert (args != np.arange(len(args))).all()
    # without the flag a set against itself finds every point at distance exactly... its own index (d2 of a row with itself rounds
    # to within the bound of 0, and nothing else is that close on this fixture)
    mins, args = M.pair_nearest(r, r, mu, False)
    assert (args.cpu().numpy() == np.arange(r.shape[0])).all()
    got = M.authpct(r, g)
    print(f"authpct {ids(shape)}: gpu {got} float64 {ref.pct()} undecided {int(ref.und.sum())}")
    if ref.und.sum() == 0:
        assert round(got * len(gen) / 100) == round(ref.pct() * len(gen) / 100)
    if shape in SHAPES:
        assert ref.und.sum() == 0
    assert got == M.authpct(real, gen)


def test_nearest_takes_lowest_index_on_exact_tie():
    # integer coordinates: every product and sum is exact in fp32, so equal distances are equal bit for bit
    rng = np.random.default_rng(9)
    a = rng.integers(-3, 4, size=(300, 6)).astype(np.float32)
    a[260] = a[4]                                      # duplicates in different row blocks and different workgroups
    a[131] = a[4]
    b = rng.integers(-3, 4, size=(150, 6)).astype(np.float32)
    b[7] = a[4]
    d = O.dist2(a, b)
    mins, args = M.pair_nearest(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV), None, False)
    assert np.array_equal(n64(mins), d.min(axis=0))
    assert np.array_equal(args.cpu().numpy(), d.argmin(axis=0))           # numpy's argmin is the first = lowest index
    assert args[7].item() == 4


# ---- KD ------------------------------------------------------------------------------------------------------------------------------
KD_SHAPES = {72: (300, 280, 72), 384: SHAPES[2]}


def kd_indices(shape, m, seed=0):
    rng = np.random.default_rng(seed)
    return (np.stack([rng.choice(shape[0], m, replace=False) for _ in range(3)]),
            np.stack([rng.choice(shape[1], m, replace=False) for _ in range(3)]))


@pytest.mark.parametrize("m", [100, 257])
@pytest.mark.parametrize("d", [72, 384])
def test_kd_sums_and_mean(d, m):
    shape = KD_SHAPES[d]
    real, gen = data(shape)
    r, g, _ = dev(shape)
    ix, iy = kd_indices(shape, m)
    got = M.pair_poly_sums(r, g, torch.from_numpy(ix.astype(np.int32)).to(DEV), torch.from_numpy(iy.astype(np.int32)).to(DEV), 1.0 / d, 1.0)
    got = got.cpu().numpy()
    bounds = []
    for s in range(3):
        sums, abs_sums = O.poly_sums(real[ix[s]], gen[iy[s]], 1.0 / d)
        ratio = np.abs(got[s] - sums) / abs_sums
        print(f"kd sums D={d} m={m} subset {s}: err / sum|k| = {ratio}")
        assert (ratio <= KSUM).all()
        bounds.append(KSUM * ((abs_sums[0] + abs_sums[1]) / (m * (m - 1)) + 2 * abs_sums[2] / (m * m)))
    want = O.kd(real, gen, ix, iy)
    vals = M.kd(r, g, subsets=(ix, iy))
    print(f"kd D={d} m={m}: gpu {vals} float64 {want} bounds {bounds}")
    assert (np.abs(vals - want) <= np.array(bounds)).all()
    assert abs(vals.mean() - want.mean()) <= np.mean(bounds)


def test_kd_excludes_the_diagonal():
    shape = KD_SHAPES[72]
    real, gen = data(shape)
    x = real.copy()
    x[7] *= 30.0                                       # k(x_7, x_7) alone is far larger than every off-diagonal sum's bound
    ix, iy = kd_indices(shape, 100, seed=1)
    for s in range(3):
        if 7 not in ix[s]:
            ix[s, s] = 7
    xd, g = torch.from_numpy(x).to(DEV), dev(shape)[1]
    got = M.pair_poly_sums(xd, g, torch.from_numpy(ix.astype(np.int32)).to(DEV), torch.from_numpy(iy.astype(np.int32)).to(DEV), 1.0 / 72, 1.0)
    got = got.cpu().numpy()
    for s in range(3):
        sums, abs_sums = O.poly_sums(x[ix[s]], gen[iy[s]], 1.0 / 72)
        diag = (float(x[7].astype(np.float64) @ x[7].astype(np.float64)) / 72 + 1.0) ** 3
        assert diag > 100 * KSUM * abs_sums[0]
        ratio = np.abs(got[s] - sums) / abs_sums
        print(f"kd diagonal subset {s}: err / sum|k| = {ratio}; diagonal term / sum = {diag / abs_sums[0]:.3e}")
        assert (ratio <= KSUM).all()


# ---- determinism -------------------------------------------------------------------------------------------------------------------
def test_every_mode_is_bit_identical_from_run_to_run():
    shape = SHAPES[1]
    r, g, mu = dev(shape)
    ix, iy = kd_indices(shape, 200)
    dx, dy = torch.from_numpy(ix.astype(np.int32)).to(DEV), torch.from_numpy(iy.astype(np.int32)).to(DEV)

    def run():
        r2r, r2g = M.pair_knn_radii(r, mu, 6), M.pair_knn_radii(g, mu, 6)
        return (M.pair_dist2(r, g, mu), r2r, r2g, *M.pair_prdc_counts(r, g, mu, r2r, r2g), *M.pair_nearest(r, r, mu, True),
                *M.pair_nearest(r, g, mu, False), M.pair_poly_sums(r, g, dx, dy, 1.0 / shape[2], 1.0))

    first, second = run(), run()
    for a, b in zip(first, second):
        assert torch.equal(a, b)


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
def test_compute_scores_end_to_end():
    shape = SHAPES[0]
    real, gen = data(shape)
    labels = np.arange(shape[1]) % 4
    s = M.compute_scores(real, gen, labels, rng=np.random.default_rng(21))
    assert set(s) == set(M.SCORE_KEYS)
    assert all(np.isfinite(v) for v in s.values())
    rng = np.random.default_rng(21)                    # the same draws, in compute_scores' order: kd, then the prdc subsample
    values = M.kd(real, gen, rng=rng)
    assert s["kd_value"] == values.mean() and s["kd_variance"] == values.std()
    n = min(shape[0], shape[1])
    i0, i1 = rng.choice(shape[0], n, replace=False), rng.choice(shape[1], n, replace=False)
    want = M.prdc(real[i0], gen[i1], 5)
    assert {k: s[k] for k in want} == want
    assert s["authpct"] == M.authpct(real, gen)
    assert s["fd"] == M.fd(real, gen)
    per_class = M.vendi_per_class(gen, labels)
    assert s["mean vendi per class"] == per_class.mean() and s["std vendi per class"] == per_class.std()
    small = M.compute_scores(real, gen, metrics=("prdc", "authpct"), reduced_n=100, rng=np.random.default_rng(3))
    assert set(small) == {"precision", "recall", "density", "coverage", "authpct"}
