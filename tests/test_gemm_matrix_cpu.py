"""Host-only side of the idb_gemm test matrix (tests/gemm_matrix.py): the case x tile x feature enumeration through idb_gemm_plan and
the idb_gemm refusal probes, with no GPU call.

- every tile id the plan-table fixture accepts is run by at least one case in each dtype;
- every family runs plain, residual, sample bias, split-K (where it has one) and both weight layouts;
- the (family, feature) pairs that are never accepted are exactly the documented refusals below, so a new variant or feature cannot
  enter without coverage and a combination cannot be dropped quietly;
- the element-wise comparison rejects what the old global bound let through and accepts the exactly rounded result."""
import gzip
import json
import math
import os
import sys
from collections import defaultdict

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_matrix as GM  # noqa: E402
from faceposegenerator_amd import _lib as L  # noqa: E402

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_plan_table.json.gz")
DTS = (L.IDB_BF16, L.IDB_F16)

_GN = {"gn", "gn_nosilu", "gn2", "gn_gnp"}          # GroupNorm fused into the GEMM (gn_in_*)
_LN = {"ln", "ln_flags256"}                          # folded LayerNorm consumer (ln_*)
_ROWS = {"rows", "rows_flags16"}                     # row statistics producer (row_stats_out)
_PRELU = {"prelu", "prelu_out2"}
_RES_PRELU = {"prelu_out2_res"}                      # act 2 takes no residual: refused on every family

# (family -> features no case runs on it).  Reasons:
#   ring / lw256: the fused GroupNorm has normalizer-wave twins on the 64-row loader-wave tiles (5x-7x) and the patch tiles (10x) only;
#   regstaged: no LDS-staged epilogue (no row statistics, no folded LayerNorm), no ReLU twin;
#   persistent: plain [M][K] operands, operand-dtype output, no split-K (so no act 2 / out2), no ReLU twin, no row statistics, no
#               per-group weights, folds a LayerNorm only with flags bit 8;
#   patch256: no split-K (act 2 / out2), pure conv epilogue (no GELU / GEGLU / ReLU), no folded LayerNorm or GroupNorm;
#   patch_small: conv epilogue without act / GEGLU, no folded LayerNorm, no row statistics.
REFUSED = {
    "ring2": _GN | _RES_PRELU,
    "ring3": _GN | _RES_PRELU,
    "ring4": _GN | _RES_PRELU,
    "regstaged": _GN | _LN | _ROWS | {"relu"} | _RES_PRELU,
    "persistent": _GN | _ROWS | _PRELU | _RES_PRELU | {"ln", "f32", "gnp", "res_sb_gnp", "out2", "res_out2", "relu", "wgroups"},
    "lw3x4": _RES_PRELU,
    "lw3x8": _RES_PRELU,
    "lw4x4": _RES_PRELU,
    "lw256": _GN | _RES_PRELU,
    "patch256": _GN | _LN | _PRELU | _RES_PRELU | {"geglu", "gelu", "relu", "out2", "res_out2"},
    "patch_small": _LN | _PRELU | _RES_PRELU | {"geglu", "gelu", "relu", "rows"},
}
MUST_RUN = ("plain", "res", "sb", "tiled")             # + split-K where the family has it
NO_SPLIT = {"persistent", "patch256"}


@pytest.fixture(scope="module")
def matrix(lib):
    return GM.enumerate_matrix(lib)


def test_variant_ids_are_the_planners(lib):
    """gemm_matrix.VARIANT_IDS lists exactly the tile ids idb_gemm builds: a forced id plans iff it is one of them (for some case)."""
    seen = set()
    for case in GM.CASES:
        for tile in range(1, 110):
            if GM.classify(lib, case, L.IDB_BF16, tile, "plain").accepted:
                seen.add(tile)
    assert sorted(seen) == GM.VARIANT_IDS


def test_every_fixture_tile_is_run(matrix):
    with gzip.open(FIXTURE, "rt") as f:
        table = json.load(f)
    fixture_tiles = {v[1] for v in table.values() if v[0] == 0}
    for dt in DTS:
        run = {v.tile for (c, d, t, f), v in matrix.items() if d == dt and v.accepted}
        assert fixture_tiles <= run, (dt, sorted(fixture_tiles - run))
        assert set(GM.VARIANT_IDS) <= run, (dt, sorted(set(GM.VARIANT_IDS) - run))


def test_every_family_runs_the_basic_features(matrix):
    for dt in DTS:
        feats, split = defaultdict(set), defaultdict(bool)
        for (c, d, t, f), v in matrix.items():
            if d == dt and v.accepted:
                feats[GM.family_of(v.tile)].add(f)
                split[GM.family_of(v.tile)] |= v.split_k > 1
        for fam in GM.FAMILIES.values():
            assert set(MUST_RUN) <= feats[fam], (dt, fam, set(MUST_RUN) - feats[fam])
            assert split[fam] == (fam not in NO_SPLIT), (dt, fam)


def test_refusals_match_the_documented_table(matrix):
    """A (family, feature) pair with no accepted combination must be listed in REFUSED, and every listed pair must stay refused.
    Prints the per-family count of planned and refused combinations (forced tile ids of the family)."""
    for dt in DTS:
        feats = defaultdict(set)
        runs, refused = defaultdict(int), defaultdict(int)
        for (c, d, t, f), v in matrix.items():
            if d != dt:
                continue
            if v.accepted:
                feats[GM.family_of(v.tile)].add(f)
                runs[GM.family_of(v.tile)] += 1
            elif t in GM.VARIANT_IDS:
                refused[GM.family_of(t)] += 1
        for fam in GM.FAMILIES.values():
            print(f"gemm matrix dtype {dt} {fam:12s} planned {runs[fam]:5d}  refused {refused[fam]:5d}")
            never = set(GM.FEATURES) - feats[fam]
            assert never == REFUSED[fam], (dt, fam, "undocumented refusals", sorted(never - REFUSED[fam]),
                                           "documented but accepted", sorted(REFUSED[fam] - never))


def test_probes_agree_with_the_queries(matrix):
    """Where the planner's own queries speak for a feature, idb_gemm's refusal agrees with them: row statistics without the in-kernel
    split-K reduce are accepted iff idb_gemm_row_stats_tiles > 0, a fused GroupNorm iff idb_gemm_fuses_groupnorm."""
    for (c, d, t, f), v in matrix.items():
        if v.where == "plan":
            continue
        if f == "rows":
            assert v.accepted == (v.row_tiles > 0), (c, d, t, f)
        if "gn" in GM.FEATURES[f]:
            assert v.accepted == (v.fuses_gn == 1), (c, d, t, f)


# ------------------------------------------------------------------------------------------------------------------------------------
# the comparison function itself
# ------------------------------------------------------------------------------------------------------------------------------------
def _old_global_check(out, ref, tol):
    return (out.double() - ref).abs().max().item() <= tol * max(1.0, ref.abs().max().item())


def test_check_rejects_one_element_in_a_small_column():
    g = torch.Generator().manual_seed(1)
    K = 320
    A = torch.randn(64, K, generator=g, dtype=torch.float64)
    W = torch.randn(2, K, generator=g, dtype=torch.float64) * K ** -0.5
    W[0] *= 1000.0                       # column 0 large, column 1 of order 1
    W[1] *= 1e-3                         # column 1 small
    ref = A @ W.t()
    absprod = A.abs() @ W.abs().t()
    out = ref.to(torch.bfloat16)
    assert GM.check(out, ref, absprod, L.IDB_BF16, K) <= 1.0
    b = GM.bound(ref, absprod, L.IDB_BF16, K)
    bad = out.double().clone()
    bad[17, 1] = ref[17, 1] + 1.5 * b[17, 1]
    assert _old_global_check(bad, ref, 2.0 ** -7)          # the old global bound lets it through ...
    with pytest.raises(AssertionError, match=r"element \(17, 1\).*\(1 of 128 elements"):
        GM.check(bad, ref, absprod, L.IDB_BF16, K)          # ... the element-wise one does not
    # the same with fp32 output: no output-rounding slack
    out32 = ref.float()
    assert GM.check(out32, ref, absprod, L.IDB_F32, K) <= 1.0
    b32 = GM.bound(ref, absprod, L.IDB_F32, K)
    bad32 = out32.double().clone()
    bad32[17, 1] = ref[17, 1] + 1.5 * b32[17, 1]
    with pytest.raises(AssertionError, match=r"element \(17, 1\)"):
        GM.check(bad32, ref, absprod, L.IDB_F32, K)


@pytest.mark.parametrize("odt,tdt", [(L.IDB_BF16, torch.bfloat16), (L.IDB_F16, torch.float16), (L.IDB_F32, torch.float32)])
def test_check_rejects_a_dropped_last_k_step(odt, tdt):
    g = torch.Generator().manual_seed(2)
    K = 2880
    A = torch.randn(128, K, generator=g).to(torch.bfloat16).double()
    W = (torch.randn(96, K, generator=g) * K ** -0.5).to(torch.bfloat16).double()
    ref = A @ W.t()
    absprod = A.abs() @ W.abs().t()
    short = (A[:, :K - 64] @ W[:, :K - 64].t()).to(tdt)      # the last 64-wide K-step never added
    with pytest.raises(AssertionError):
        GM.check(short, ref, absprod, odt, K)


@pytest.mark.parametrize("odt,tdt", [(L.IDB_BF16, torch.bfloat16), (L.IDB_F16, torch.float16), (L.IDB_F32, torch.float32)])
def test_check_accepts_the_exactly_rounded_result(odt, tdt):
    g = torch.Generator().manual_seed(3)
    K = 576
    A = torch.randn(200, K, generator=g).to(torch.float16).double()
    W = (torch.randn(100, K, generator=g) * K ** -0.5).to(torch.float16).double()
    ref = A @ W.t() + torch.randn(100, generator=g, dtype=torch.float64)
    absprod = A.abs() @ W.abs().t()
    assert GM.check(ref.to(tdt), ref, absprod, odt, K) <= 1.0
    # a NaN (an element the kernel never wrote into a NaN-filled buffer) is rejected
    bad = ref.to(tdt).clone()
    bad[3, 4] = math.nan
    with pytest.raises(AssertionError):
        GM.check(bad, ref, absprod, odt, K)
