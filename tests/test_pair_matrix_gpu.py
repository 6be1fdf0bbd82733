"""Every case of the all-pairs kernel test matrix (tests/pair_matrix.py) on the device, through the C ABI (lib.idb_pair_*, not the
metrics.py wrappers), against the float64 references and the criteria stated there: distances within TAU * scale of float64, decisions
equal to float64's wherever float64's gap exceeds TAU * scale, the integer cases bit for bit.

Every output buffer lies between 64 guard elements of a NaN bit pattern that are checked after the launch; an output element the kernel did
not write keeps that pattern and fails its criterion.  The workspace is exactly idb_pair_workspace_bytes(...) long inside a guarded
buffer, 16-byte aligned, and its guards must stay intact.  Every launch is made twice into separate buffers and workspaces and the two
results must be equal bit for bit.  The misalignment tests place one operand 4 bytes past a 16-byte boundary inside a larger allocation,
which sends every mode down pair_fetch's scalar path, and demand the bits of the aligned run.  A failure names the case, the worst
element's index, its error and its bound.  test_summary prints the worst err / (TAU * scale) and the launches per mode (recorded in
profiles/metrics/README.md, never used as thresholds).

Measured on an MI355X, worst err / (TAU * scale) over all cases: dist2 0.092, knn 0.082, nearest 0.079, prdc row_min 0.068, the integer
cases and the misaligned runs bit-equal (profiles/metrics/README.md)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import matrix_common as MC  # noqa: E402
import metrics_oracle as O  # noqa: E402
import pair_matrix as P  # noqa: E402
from faceposegenerator_amd import _lib as L  # noqa: E402

pytestmark = pytest.mark.gpu

NAMES = [c.name for c in P.CASES]
W = MC.Worst("pair matrix", "err / (TAU * scale)", launches=True)


class _In:
    """A host array on the device, 4 bytes past a 16-byte boundary inside a larger allocation when `off`."""

    def __init__(self, a, off=False):
        a = np.ascontiguousarray(a)
        assert a.dtype.itemsize == 4
        self.buf = torch.zeros(a.size + 8, dtype=torch.int32, device=MC.DEV)
        self.buf[int(off):int(off) + a.size] = torch.from_numpy(a.reshape(-1).view(np.int32)).to(MC.DEV)
        self.ptr = self.buf.data_ptr() + 4 * int(off)
        assert self.buf.data_ptr() % 16 == 0 and self.ptr % 16 == (4 if off else 0)


class Gpu:
    """The five entries over the C ABI with pair_matrix.Restated's methods.  mis = 'a', 'b' or 'shift' misaligns that operand."""

    def __init__(self, lib, mis=None):
        self.lib, self.mis = lib, mis

    def _twice(self, mode, what, size_args, outs, launch):
        """launch(out pointers, ws pointer, ws bytes) twice into separate buffers; bit-equal; the first results as numpy arrays."""
        need = self.lib.idb_pair_workspace_bytes(*size_args)
        assert need > 0 and need % 4 == 0, f"{what}: idb_pair_workspace_bytes{size_args} refused"
        runs = []
        for _ in range(2):
            bufs, ws = [MC.Guarded(n, np.dtype(dt).itemsize) for n, dt in outs], MC.Guarded(need // 4)
            L.check(launch([b.ptr for b in bufs], ws.ptr, need), what)
            runs.append((bufs, ws))
        torch.cuda.synchronize()
        W.launched(mode, 2)
        res = []
        for bufs, ws in runs:
            ws.raw(what + ": the workspace")
            res.append([b.raw(what).view(dt) for b, (_, dt) in zip(bufs, outs)])
        for x, y in zip(*res):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), f"{what}: a relaunch gave different bits"
        return res[0]

    def _shift(self, shift):
        return None if shift is None else _In(np.asarray(shift, np.float32), self.mis == "shift")

    def dist2(self, a, b, shift):
        na, nb, d = len(a), len(b), a.shape[1]
        ad, bd, sd = _In(a, self.mis == "a"), _In(b, self.mis == "b"), self._shift(shift)
        out, = self._twice("dist2", f"idb_pair_dist2 {na} x {nb} x {d}", (L.IDB_PAIR_DIST2, na, nb, 0), [(na * nb, np.float32)],
                           lambda o, ws, sz: self.lib.idb_pair_dist2(ad.ptr, na, bd.ptr, nb, d, sd and sd.ptr, o[0], ws, sz, MC.stream()))
        return out.reshape(na, nb)

    def knn(self, x, shift, kths):
        n, d = x.shape
        xd, sd = _In(x, self.mis in ("a", "b")), self._shift(shift)
        return {kth: self._twice("knn", f"idb_pair_knn_radii {n} x {d} kth {kth}", (L.IDB_PAIR_KNN, n, 0, 0), [(n, np.float32)],
                                 lambda o, ws, sz: self.lib.idb_pair_knn_radii(xd.ptr, n, d, sd and sd.ptr, kth, o[0], ws, sz, MC.stream()))[0]
                for kth in kths}

    def prdc(self, real, gen, shift, r2_real, r2_gen):
        nr, ng, d = len(real), len(gen), real.shape[1]
        rd, gd, sd = _In(real, self.mis == "a"), _In(gen, self.mis == "b"), self._shift(shift)
        r2r, r2g = _In(np.asarray(r2_real, np.float32)), _In(np.asarray(r2_gen, np.float32))
        return self._twice("prdc", f"idb_pair_prdc_counts {nr} x {ng} x {d}", (L.IDB_PAIR_PRDC, nr, ng, 0),
                           [(ng, np.int32), (nr, np.int32), (nr, np.float32)],
                           lambda o, ws, sz: self.lib.idb_pair_prdc_counts(rd.ptr, nr, gd.ptr, ng, d, sd and sd.ptr, r2r.ptr, r2g.ptr, o[0], o[1], o[2],
                                                                           ws, sz, MC.stream()))

    def nearest(self, a, b, shift, exclude_diag):
        na, nb, d = len(a), len(b), a.shape[1]
        ad, bd, sd = _In(a, self.mis == "a"), _In(b, self.mis == "b"), self._shift(shift)
        return self._twice("nearest", f"idb_pair_nearest {na} x {nb} x {d} exclude_diag {int(exclude_diag)}", (L.IDB_PAIR_NEAREST, na, nb, 0),
                           [(nb, np.float32), (nb, np.int32)],
                           lambda o, ws, sz: self.lib.idb_pair_nearest(ad.ptr, na, bd.ptr, nb, d, sd and sd.ptr, int(exclude_diag), o[0], o[1], ws, sz,
                                                                       MC.stream()))

    def poly(self, x, y, ix, iy, gamma=1.0):
        (nx, d), ny, (s, m) = x.shape, len(y), ix.shape
        xd, yd = _In(x, self.mis == "a"), _In(y, self.mis == "b")
        dx, dy = _In(ix.astype(np.int32)), _In(iy.astype(np.int32))
        out, = self._twice("poly", f"idb_pair_poly_sums {nx} x {ny} x {d}, {s} subsets of {m}", (L.IDB_PAIR_POLY, m, 0, s), [(3 * s, np.float64)],
                           lambda o, ws, sz: self.lib.idb_pair_poly_sums(xd.ptr, nx, yd.ptr, ny, d, dx.ptr, dy.ptr, s, m, gamma, 1.0, o[0], ws, sz,
                                                                         MC.stream()))
        return out.reshape(s, 3)


# ---- the cases -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", P.MODES[:4])
@pytest.mark.parametrize("name", NAMES)
def test_real_case(lib, name, mode):
    P.run_real_case(Gpu(lib), name, mode, W.note)


def test_degenerate_sets(lib):
    P.run_degenerate(Gpu(lib), W.note)


@pytest.mark.parametrize("which", ("forward", "reversed", "swapped", "exclude", "knn"))
def test_integer_ties_across_passes_and_splits(lib, which):
    P.run_ties(Gpu(lib), which, W.note)


@pytest.mark.parametrize("case", P.POLY_CASES, ids=lambda c: "x".join(map(str, c)))
def test_poly_sums_exact(lib, case):
    P.run_poly(Gpu(lib), case, W.note)


def test_kd_chunking(lib):
    """metrics.kd over 4100 subsets: the second chunk of its 4096-subset step.  The sums are exact (integer features, gamma = 1 / 4), so
    each value differs from float64's by the rounding of its own two divisions at most: 4 ulp of the larger term."""
    from faceposegenerator_amd import metrics as M
    x, y, ix, iy = P.kd_chunk_inputs()
    m = P.KD_CHUNK["m"]
    got = M.kd(x, y, subsets=(ix, iy))
    sums = P.poly_reference(x, y, ix, iy, gamma=1.0 / x.shape[1])
    want = np.array([O.mmd2(s, m) for s in sums])
    bound = 4 * np.spacing(np.maximum(np.abs(sums[:, 0] + sums[:, 1]) / (m * (m - 1)), 2 * np.abs(sums[:, 2]) / (m * m)))
    assert got.shape == want.shape
    P.within("kd chunking", got, want, bound)
    assert np.array_equal(got[4096:], M.kd(x, y, subsets=(ix[4096:], iy[4096:])))     # the second chunk alone: the same values


_ALIGNED = {}
_LABELS = ("dist2", "knn radii of real", "knn radii of gen", "in_real_sphere", "covered", "row_min", "nearest min", "nearest argmin",
           "nearest min (no diagonal)", "nearest argmin (no diagonal)", "poly sums")


def _every_mode(lib, name, mis):
    """The outputs of every mode on one case, in the order of _LABELS."""
    real, gen, mu = P.inputs(name)
    impl = Gpu(lib, mis)
    ref = P.prdc_ref(name, 5)
    rng = np.random.default_rng(11)
    m = min(len(real), len(gen))
    ix = np.stack([rng.choice(len(real), m, replace=False) for _ in range(2)])
    iy = np.stack([rng.choice(len(gen), m, replace=False) for _ in range(2)])
    return [impl.dist2(real, gen, mu), impl.knn(real, mu, (6,))[6], impl.knn(gen, mu, (6,))[6],
            *impl.prdc(real, gen, mu, ref.r2_real.astype(np.float32), ref.r2_gen.astype(np.float32)),
            *impl.nearest(real, gen, mu, False), *impl.nearest(real, real, mu, True),
            impl.poly(real, gen, ix, iy, gamma=1.0 / real.shape[1])]          # takes no shift: `shift` repeats the aligned run there


@pytest.mark.parametrize("mis", ("a", "b", "shift"))
@pytest.mark.parametrize("name", P.MISALIGNED)
def test_misaligned_operand_gives_the_aligned_bits(lib, name, mis):
    """pair_fetch loads the same values through either path and the arithmetic behind the load is the same code."""
    if name not in _ALIGNED:
        _ALIGNED[name] = _every_mode(lib, name, None)
    for label, g, w in zip(_LABELS, _every_mode(lib, name, mis), _ALIGNED[name]):
        assert g.shape == w.shape and g.dtype == w.dtype
        MC.same_bits(f"{name}, `{mis}` misaligned, {label} against the aligned run", g, w)


def test_summary():
    W.show()
