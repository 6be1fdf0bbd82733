"""The CPU half of the all-pairs kernel test matrix (tests/pair_matrix.py), no GPU: the conditions the input recipes must meet (at most
0.1 % undecided comparisons per case and among its authenticity columns; the fp32 restatement of the expansion at or below TAU / 4;
every intermediate of the integer cases below 2^24), that the cases reach the paths they were chosen for, the teeth of the criteria (the
unmodified restatement passes every case, every defect of pair_matrix.DEFECTS fails its named case) and the argument checks of
csrc/idb_pair.hip that tests/test_metrics_cpu.py does not already make, which answer before any HIP call."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import metrics_oracle as O  # noqa: E402
import pair_matrix as P  # noqa: E402

NAMES = [c.name for c in P.CASES]


# ---- the cases reach what they were chosen for -------------------------------------------------------------------------------------------
def test_cases_cover_what_they_were_chosen_for():
    assert len(set(NAMES)) == len(NAMES)
    by = P.BY_NAME
    assert [len(p) for p in P.passes_of(by["loop9"].nr)] == [2, 1, 1, 1, 1, 1, 1, 1] and by["loop9"].nr - 8 * P.PT == 1
    assert [len(p) for p in P.passes_of(by["loop18_scalar"].nr)] == [3, 3, 2, 2, 2, 2, 2, 2] and by["loop18_scalar"].d % 4 != 0
    assert [len(p) for p in P.passes_of(by["wide_loop"].ng)] == [2, 2, 1, 1, 1, 1, 1, 1] and by["wide_loop"].d % 4 == 2
    assert all(by[n].ng > by[n].nr for n in ("wide", "wide_loop"))
    assert by["wide"].d % P.PK == 8 and by["wide"].d > P.PK and by["tail33"].d == P.PK + 1 and by["tail5"].d % 4 == 1 and by["tail3"].d < 4
    assert by["tiny"].ng < P.KNN_MAX < by["tiny"].nr
    assert {(by[n].nr, by[n].ng) for n in ("edge127", "edge128", "edge129")} == {(127, 129), (128, 127), (129, 128)}
    for n in P.MISALIGNED:
        assert by[n].d % 4 == 0                                            # the vector path until a pointer is misaligned
    # half-wave h owns the rows with (row mod 8) / 4 == h, ascending
    for h in (0, 1):
        rows = P.half_rows(h)
        assert (np.diff(rows) > 0).all() and ((rows % 8) // 4 == h).all() and len(rows) == 64
    a, b = P.ties_inputs()
    assert all((a[r] == a[3]).all() for r in (130, 1027, 2199)) and (b[7] == a[3]).all()
    blocks = {r: r // P.PT for r in (3, 130, 1027, 2199)}
    assert blocks[1027] % 8 == blocks[3] % 8 and blocks[1027] != blocks[3] and blocks[130] % 8 != 0 and blocks[2199] == 17
    ms = [c[3] for c in P.POLY_CASES]
    assert {2, 127, 128, 129} <= set(ms) and any(c[0] != c[1] for c in P.POLY_CASES)
    for case in P.POLY_CASES:
        x, y, ix, iy = P.poly_inputs(case)
        assert (np.diff(ix[0]) < 0).all() and (np.diff(iy[0]) < 0).all()   # one subset in descending order
        assert case[0] - 1 in ix[-1] and case[1] - 1 in iy[-1]             # one reaches the last row of both sets
        assert all(len(set(r)) == case[3] for r in ix) and ix.max() < case[0] and iy.max() < case[1] and min(ix.min(), iy.min()) >= 0
    assert P.KD_CHUNK["subsets"] > 4096


def test_knn_table_is_knn_radii_scale():
    for name, which in (("tiny", "gen"), ("tail5", "real"), ("edge129", "real")):
        real, gen, mu = P.inputs(name)
        x = real if which == "real" else gen
        for kth in range(1, min(P.KNN_MAX, len(x)) + 1):
            for shifted in (True, False):
                want = O.knn_radii_scale(x, kth, P.shift64(mu if shifted else None, x.shape[1]))
                got = P.knn_ref(name, which, kth, shifted)
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[0], O.knn_radii(x, kth))


# ---- the conditions on the inputs --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_undecided_cap(name):
    c = P.BY_NAME[name]
    for k in c.ks:
        share = P.prdc_ref(name, k).undecided_share()
        print(f"{name} k = {k}: PRDC undecided share {share:.2e}")
        assert share <= P.UNDECIDED_CAP, (name, k, share)
    auth = P.auth_ref(name)
    print(f"{name}: authenticity columns undecided {int(auth.und.sum())} of {auth.und.size}; argmin undecided {int((~auth.rg.decided).sum())}, "
          f"{int((~auth.rr.decided).sum())}")
    # a column whose real x gen argmin float64 does not decide counts as undecided in `und`; the real x real argmin is compared where
    # it is decided and enters no metric (authenticity reads that run's minimum only)
    assert auth.und.mean() <= P.UNDECIDED_CAP


@pytest.mark.parametrize("name", NAMES)
def test_fp32_expansion_stays_within_a_quarter_of_tau(name):
    real, gen, mu = P.inputs(name)
    for shifted in (True, False):
        want, scale = P.dist2_ref(name, shifted)
        got = P.emulate_dist2(real, gen, mu if shifted else None)
        ratio = float((np.abs(got.astype(np.float64) - want) / scale).max())
        print(f"{name} {'shift = mean' if shifted else 'no shift'}: fp32 expansion max err / scale = {ratio:.2e}")
        assert ratio <= P.TAU / 4, (name, shifted, ratio)


def test_integer_cases_are_exact_in_fp32():
    a, b = P.ties_inputs()
    assert np.array_equal(a, np.round(a)) and np.abs(a).max() <= 3 and np.abs(b).max() <= 3
    assert P.exact_dist_precondition(a, b) < 2 ** 24 and P.exact_dist_precondition(a, a) < 2 ** 24
    for case in P.POLY_CASES:
        x, y, _, _ = P.poly_inputs(case)
        assert np.abs(x).max() <= 1 and np.abs(y).max() <= 1 and np.array_equal(x, np.round(x))
        worst = P.exact_poly_precondition(case)
        print(f"poly {case}: largest tile sum of |k| = {worst:.0f}")
        assert worst < 2 ** 24, (case, worst)
    x, y, ix, iy = P.kd_chunk_inputs()
    # gamma = 1 / 4 and at most 4 terms of +-1: gamma a.b + 1 is a multiple of 1/4 in 0..2, its cube a multiple of 1/64 below 8
    assert x.shape[1] == 4 and np.abs(x).max() <= 1 and np.abs(y).max() <= 1 and ix.shape == (4100, 2)


# ---- teeth -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", P.MODES[:4])
@pytest.mark.parametrize("name", NAMES)
def test_restatement_passes_every_real_case(name, mode):
    worst = {}
    P.run_real_case(P.Restated(), name, mode, lambda m, r, what: worst.update({m: max(worst.get(m, 0.0), r)}))
    print(f"{name} {mode}: restatement worst err / (TAU * scale) = {worst}")
    assert all(v <= 0.25 for v in worst.values())                          # the condition above, seen through every mode


def test_restatement_passes_the_degenerate_and_integer_cases():
    impl = P.Restated()
    P.run_degenerate(impl)
    for which in ("forward", "reversed", "swapped", "exclude", "knn"):
        P.run_ties(impl, which)
    for case in P.POLY_CASES:
        P.run_poly(impl, case)


def test_defect_list_is_complete():
    assert set(P.DEFECT_CASES) == set(P.DEFECTS) - set(P.HARMLESS) and len(P.DEFECTS) == 13 and P.HARMLESS == ()


@pytest.mark.parametrize("defect", [d for d in P.DEFECTS if d not in P.HARMLESS])
def test_every_defect_fails_its_named_case(defect):
    msg = P.defect_fails(defect)
    print(f"{defect}: {msg}")
    assert msg is not None, (defect, P.DEFECT_CASES[defect][1:])


def test_knn_insert_is_the_kernels_list():
    """The vectorised insertion against the kernel's statement of it, entry by entry."""
    def kernel(L, v):
        L = list(L)
        if v < L[-1]:
            for t in range(P.KNN_MAX - 1, 0, -1):
                L[t] = L[t - 1] if v < L[t - 1] else (v if v < L[t] else L[t])
            L[0] = v if v < L[0] else L[0]
        return L
    rng = np.random.default_rng(0)
    vals = rng.integers(0, 6, size=(40, 50)).astype(np.float32)            # many equal values
    L = np.full((50, P.KNN_MAX), np.inf, np.float32)
    want = [list(r) for r in L]
    for v in vals:
        L = P.knn_insert(L, v)
        want = [kernel(r, x) for r, x in zip(want, v)]
        assert np.array_equal(L, np.array(want, np.float32))
    assert np.array_equal(L, np.sort(vals, axis=0)[:P.KNN_MAX].T)


# ---- argument checks: answered before any HIP call -----------------------------------------------------------------------------------------
A = 1 << 20              # any non-null 16-byte aligned address: none of these calls dereferences it


def _refused(lib, rc, text):
    msg = lib.idb_last_error()
    assert rc == -1 and text.encode() in msg, (rc, msg)


def test_workspace_must_be_16_byte_aligned_and_large_enough(lib):
    from faceposegenerator_amd import _lib as L
    q = lib.idb_pair_workspace_bytes
    need = {m: q(m, 300, 200, 2) for m in (L.IDB_PAIR_DIST2, L.IDB_PAIR_KNN, L.IDB_PAIR_PRDC, L.IDB_PAIR_NEAREST, L.IDB_PAIR_POLY)}
    assert all(v > 0 and v % 256 == 0 for v in need.values())
    for ws, size in ((A + 4, 1 << 24), (A + 8, 1 << 24), (A, None)):
        sz = lambda m: need[m] - 1 if size is None else size                # noqa: E731
        _refused(lib, lib.idb_pair_dist2(A, 300, A, 200, 8, A, A, ws, sz(L.IDB_PAIR_DIST2), None), "workspace")
        _refused(lib, lib.idb_pair_knn_radii(A, 300, 8, A, 6, A, ws, sz(L.IDB_PAIR_KNN), None), "workspace")
        _refused(lib, lib.idb_pair_prdc_counts(A, 300, A, 200, 8, A, A, A, A, A, A, ws, sz(L.IDB_PAIR_PRDC), None), "workspace")
        _refused(lib, lib.idb_pair_nearest(A, 300, A, 200, 8, A, 0, A, A, ws, sz(L.IDB_PAIR_NEAREST), None), "workspace")
        _refused(lib, lib.idb_pair_poly_sums(A, 300, A, 300, 8, A, A, 2, 300, 1.0, 1.0, A, ws, sz(L.IDB_PAIR_POLY), None), "workspace")


def test_degenerate_sizes_are_refused_or_accepted_by_rule(lib):
    big = 1 << 24
    _refused(lib, lib.idb_pair_knn_radii(A, 1, 4, A, 2, A, A, big, None), "kth")          # kth <= n
    _refused(lib, lib.idb_pair_knn_radii(A, 8, 4, A, 9, A, A, big, None), "kth")
    _refused(lib, lib.idb_pair_nearest(A, 1, A, 2, 4, A, 1, A, A, A, big, None), "exclude_diag")
    _refused(lib, lib.idb_pair_poly_sums(A, 300, A, 280, 5, A, A, 1, 281, 1.0, 1.0, A, A, big, None), "subset size")   # m <= min(nx, ny)
    _refused(lib, lib.idb_pair_poly_sums(A, 300, A, 280, 5, A, A, 21846, 2, 1.0, 1.0, A, A, big, None), "subsets")
    _refused(lib, lib.idb_pair_poly_sums(A, 300, A, 280, 5, None, A, 1, 2, 1.0, 1.0, A, A, big, None), "null")
    for f, args in ((lib.idb_pair_dist2, (A, (1 << 22) + 1, A, 4, 8, A, A, A, big, None)),
                    (lib.idb_pair_prdc_counts, (A, 4, A, 4, (1 << 16) + 1, A, A, A, A, A, A, A, big, None)),
                    (lib.idb_pair_knn_radii, (A, 4, 0, A, 1, A, A, big, None))):
        _refused(lib, f(*args), " in 1..")
