"""float64 oracle for faceposegenerator_amd/metrics.py and the idb_pair_* kernels (test infrastructure only).

Written from the published formulas (Naeem et al. 2020 for PRDC, Alaa et al. 2022 for the authenticity test, Binkowski et al. 2018
for the unbiased MMD^2 with the cubic polynomial kernel), independently of metrics.py: squared distances are taken by direct
differences sum_k (a_k - b_k)^2, never by the norm expansion the kernels use, and every hard threshold comparison comes with its
float64 gap |d2 - r2| and the scale |a - mu|^2 + |b - mu|^2 of the pair, mu the mean of the real set, so that a test can tell a
comparison float64 decides from one that lies within round-off of its threshold (`undecided`).
"""
import numpy as np

TAU = 4e-6            # a comparison is undecided when gap <= TAU * scale (tests/test_metrics_gpu.py derives the figure)
UNDECIDED_CAP = 1e-3  # at most this share of a case's comparisons may be undecided


def fixture(nr, ng, d, seed=3):
    """Real and generated float32 feature sets: 8 cluster centres in a 6-dimensional latent space, latent noise 0.7, the generated set
    shifted by 0.25 in the latent space, one fixed random 6 -> d linear map, 0.05 isotropic noise in d, and +2.0 on every feature
    (real features have a mean far from 0).  With the default seed float64 leaves no comparison of PRDC (nearest_k = 5) or of the
    authenticity test undecided at the shapes the tests use (test_metrics_cpu.py asserts it)."""
    rng = np.random.default_rng(1000 + seed)
    centres = rng.normal(size=(8, 6)) * 1.5
    lift = rng.normal(size=(6, d)) / np.sqrt(6.0)

    def draw(n, shift):
        z = centres[rng.integers(0, 8, size=n)] + 0.7 * rng.normal(size=(n, 6)) + shift
        return (z @ lift + 0.05 * rng.normal(size=(n, d)) + 2.0).astype(np.float32)

    return draw(nr, 0.0), draw(ng, 0.25)


def dist2(a, b):
    """[Na][Nb] squared distances by direct differences, float64."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    out = np.empty((a.shape[0], b.shape[0]))
    for i in range(a.shape[0]):
        diff = b - a[i]
        out[i] = np.einsum("jk,jk->j", diff, diff)
    return out


def sq_norms(x, mu):
    c = np.asarray(x, np.float64) - np.asarray(mu, np.float64)
    return np.einsum("ik,ik->i", c, c)


def scale(a, b, mu):
    """[Na][Nb]: |a_i - mu|^2 + |b_j - mu|^2, what the round-off of the expansion is proportional to."""
    return sq_norms(a, mu)[:, None] + sq_norms(b, mu)[None, :]


def knn_radii(x, kth):
    """The kth smallest of every row of d2(x, x): the point itself (distance 0) is the first."""
    d = dist2(x, x)
    np.fill_diagonal(d, 0.0)
    return np.partition(d, kth - 1, axis=1)[:, kth - 1]


def knn_radii_scale(x, kth, mu):
    """(knn_radii, the scale of each radius: |x_i - mu|^2 + |x_n - mu|^2 with n the kth nearest row of i, the point itself included)."""
    d = dist2(x, x)
    np.fill_diagonal(d, -1.0)                         # the point itself sorts first whatever its duplicates
    nbr = np.argsort(d, axis=1, kind="stable")[:, kth - 1]
    nrm = sq_norms(x, mu)
    return np.maximum(d[np.arange(len(d)), nbr], 0.0), nrm + nrm[nbr]


def knn_table(x, kmax):
    """(radii [n][kmax], neighbours [n][kmax]): column kth - 1 holds what knn_radii_scale(x, kth, .) takes its radius and its scale
    from, for every kth up to kmax from one sort."""
    d = dist2(x, x)
    np.fill_diagonal(d, -1.0)
    nbr = np.argsort(d, axis=1, kind="stable")[:, :kmax]
    return np.maximum(np.take_along_axis(d, nbr, axis=1), 0.0), nbr


def undecided(gap, scl, tau=TAU):
    return gap <= tau * scl


class Prdc:
    """Everything PRDC compares, for `real` against `gen` with nearest_k neighbours."""

    def __init__(self, real, gen, nearest_k):
        mu = np.asarray(real, np.float64).mean(axis=0)
        self.k, self.nr, self.ng = nearest_k, len(real), len(gen)
        self.d = dist2(real, gen)
        self.scale = scale(real, gen, mu)
        self.r2_real, self.r2_gen = knn_radii(real, nearest_k + 1), knn_radii(gen, nearest_k + 1)
        self.in_sphere = self.d < self.r2_real[:, None]                 # gen j inside the sphere of real i
        self.in_sphere_und = undecided(np.abs(self.d - self.r2_real[:, None]), self.scale)
        self.in_gen = self.d < self.r2_gen[None, :]                     # real i inside the sphere of gen j
        self.in_gen_und = undecided(np.abs(self.d - self.r2_gen[None, :]), self.scale)
        self.row_min = self.d.min(axis=1)
        self.row_arg = self.d.argmin(axis=1)
        self.cov = self.row_min < self.r2_real
        self.cov_und = undecided(np.abs(self.row_min - self.r2_real), self.scale[np.arange(self.nr), self.row_arg])

    def scores(self):
        return {"precision": float(self.in_sphere.any(axis=0).mean()), "recall": float(self.in_gen.any(axis=1).mean()),
                "density": float(self.in_sphere.sum(axis=0).mean() / self.k), "coverage": float(self.cov.mean())}

    def undecided_share(self):
        n = self.in_sphere_und.size + self.in_gen_und.size + self.cov_und.size
        return (self.in_sphere_und.sum() + self.in_gen_und.sum() + self.cov_und.sum()) / n


def prdc(real, gen, nearest_k=5):
    return Prdc(real, gen, nearest_k).scores()


class Nearest:
    """min_i d2(i, j), its argmin (lowest index on a tie), the runner-up's distance and the margin below which float64 itself does
    not separate the two: each carries an error of at most TAU * its own scale, so the order is decided when the difference exceeds
    TAU * (scale of the best + scale of the runner-up)."""

    def __init__(self, a, b, mu, exclude_diag=False):
        d = dist2(a, b)
        if exclude_diag:
            np.fill_diagonal(d, np.inf)
        s = scale(a, b, mu)
        cols = np.arange(d.shape[1])
        self.arg = d.argmin(axis=0)
        self.min = d[self.arg, cols]
        self.scale = s[self.arg, cols]
        rest = d.copy()
        rest[self.arg, cols] = np.inf
        second = rest.argmin(axis=0)
        self.decided = rest[second, cols] - self.min > TAU * (self.scale + s[second, cols])


class Auth:
    def __init__(self, real, gen):
        mu = np.asarray(real, np.float64).mean(axis=0)
        self.rr = Nearest(real, real, mu, exclude_diag=True)
        self.rg = Nearest(real, gen, mu)
        lhs, rhs = self.rr.min[self.rg.arg], self.rg.min
        self.authentic = lhs < rhs
        self.und = undecided(np.abs(lhs - rhs), self.rr.scale[self.rg.arg] + self.rg.scale) | ~self.rg.decided

    def pct(self):
        return 100.0 * float(self.authentic.mean())


def authpct(real, gen):
    return Auth(real, gen).pct()


def poly_sums(x, y, gamma, coef0=1.0):
    """(sums [3], sums of |k| [3]) of k(a, b) = (gamma a.b + coef0)^3 over x x x and y x y without their diagonals and over x x y."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    off = ~np.eye(len(x), dtype=bool)
    kxx, kyy, kxy = (gamma * x @ x.T + coef0) ** 3, (gamma * y @ y.T + coef0) ** 3, (gamma * x @ y.T + coef0) ** 3
    sums = np.array([kxx[off].sum(), kyy[off].sum(), kxy.sum()])
    return sums, np.array([np.abs(kxx[off]).sum(), np.abs(kyy[off]).sum(), np.abs(kxy).sum()])


def mmd2(sums, m):
    return (sums[0] + sums[1]) / (m * (m - 1)) - 2.0 * sums[2] / (m * m)


def kd(real, gen, idx_real, idx_gen):
    """The unbiased MMD^2 of every subset pair (rows idx_real[s] of real against rows idx_gen[s] of gen), gamma = 1 / D, coef0 = 1."""
    real, gen = np.asarray(real, np.float64), np.asarray(gen, np.float64)
    g = 1.0 / real.shape[1]
    return np.array([mmd2(poly_sums(real[ix], gen[iy], g)[0], len(ix)) for ix, iy in zip(idx_real, idx_gen)])
