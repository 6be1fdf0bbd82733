"""The kernel arguments of the implicit-GEMM kernels, on the smallest shapes where a wrongly fetched or wrongly selected one shows.

The ring, loader-wave, patch and fused-GroupNorm kernels take their launch scalars as leading plain parameters (GemmTile: tile index,
K range, the step counts the K seek walks), fetch the head of GemmParams and the source record of their first K-step in one go, and
select everything else from those registers (csrc/idb_gemm_epi.h).  Each case below makes one of these values non-trivial:

  1. plain linears of one and two K-steps, ragged and whole last tiles: the ring-stage guards `st < nk`, M / N out of the head;
  2. a 3x3 conv of two 3x3 sources (64 + 128 channels = 27 K-steps), split 4: the slices start at K-steps 0, 6, 13, 20 = a non-zero
     tap of source 0, source 1 at channel offset 0, source 1 at channel offset 64 — the seek's (source, tap, channel) all non-trivial;
  3. the same with a third, 1x1 source of 320 channels (32 K-steps), split 2 and 8: slice 7 of 8 starts at K-step 28, inside the 1x1
     source (tap 4) at channel offset 64;
  4. grouped weights on the linear and on the conv: the weight descriptor depends on the tile's row group;
  5. the fused GroupNorm: the patch conv at 8x8 and 16x16, 64 -> 64 and 128 -> 64, with a split of 2 and with none (forced 1), on the
     transforming patch loaders and on the normalizer waves of idb_gemm_kernel_gn, and that kernel's 1x1 form at 16x16 with 64 channels.

Every case runs on every tile id of the variant table that accepts it (forced `tile`, as tests/test_gemm_matrix_gpu.py does), in f16 and
bf16, and is checked per element against that file's float64 reference with the bound of tests/gemm_matrix.py.  A case that silently
fell back to another kernel or split would prove nothing, so the plan is asserted: the split is the forced one, the fused GroupNorm is
planned where asked for, and every kernel family the case names has run."""
import os
import sys
from collections import defaultdict

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_matrix as GM  # noqa: E402
from test_gemm_matrix_gpu import DTYPES, CaseData  # noqa: E402

pytestmark = pytest.mark.gpu


def _kind(verdict, feat):
    """Kernel family of a plan: ring / lw / patch, "gn" = idb_gemm_kernel_gn, "patch_gn" = the transforming patch loaders."""
    fam = verdict.tile // 10
    gn = "gn" in GM.FEATURES[feat] and verdict.fuses_gn
    if fam <= 2:
        return "ring"
    if 5 <= fam <= 8:
        return "gn" if gn else "lw"
    if fam >= 9:
        return "patch_gn" if gn else "patch"
    return GM.FAMILIES[fam]


def _two_src(name, split_k, third=()):
    srcs = ((64, 9, 8, 8, 0), (128, 9, 8, 8, 0)) + third
    return GM.Case(name, 2, 8, 8, 128, srcs, split_k=split_k)


def _gn_conv(hw, cin, split_k):
    return GM.Case(f"gnconv_{hw}x{hw}_{cin}_sk{split_k}", 2, hw, hw, 64, ((cin, 9, hw, hw, 0),), split_k=split_k)


# (case, features, kernel families that must have run)
SPECS = [(GM.Case(f"lin_{m}x{n}x{k}", m, 1, 1, n, ((k, 1, 1, 1, 0),)), ("plain", "wgroups") if (m, n, k) == (100, 160, 128) else ("plain",),
          ("ring", "lw")) for m in (64, 100) for n in (64, 160) for k in (64, 128)]
SPECS += [
    (_two_src("conv_64+128_sk4", 4), ("plain", "wgroups"), ("ring", "lw", "patch")),
    (_two_src("conv_64+128+1x1_sk2", 2, ((320, 1, 8, 8, 0),)), ("plain",), ("ring", "lw", "patch")),
    (_two_src("conv_64+128+1x1_sk8", 8, ((320, 1, 8, 8, 0),)), ("plain",), ("ring", "lw", "patch")),
]
SPECS += [(_gn_conv(hw, cin, sk), ("gn",), ("patch_gn", "gn")) for hw in (8, 16) for cin in (64, 128) for sk in (1, 2)]   # 1: forced unsplit
SPECS += [(GM.Case("gn1x1_16x16_64", 2, 16, 16, 64, ((64, 1, 16, 16, 0),)), ("gn",), ("gn",))]


@pytest.mark.parametrize("dtname", list(DTYPES))
@pytest.mark.parametrize("spec", SPECS, ids=lambda s: s[0].name)
def test_gemm_kernel_arguments(lib, dtname, spec):
    case, feats, families = spec
    dt, tdt = DTYPES[dtname]
    data = CaseData(lib, case, dt, tdt, seed=4000 + SPECS.index(spec))
    ran = defaultdict(int)
    worst = 0.0
    for feat in feats:
        assert GM.applicable(case, feat), (case.name, feat)
        for tile in GM.VARIANT_IDS:
            v = GM.classify(lib, case, dt, tile, feat)
            if not v.accepted:
                continue
            assert v.tile == tile, f"{case.name} {feat}: tile {tile} planned as {v.tile}"
            if case.split_k:
                assert v.split_k == case.split_k, f"{case.name} {feat} tile {tile}: split {v.split_k}, not the forced {case.split_k}"
            kind = _kind(v, feat)
            if "gn" in GM.FEATURES[feat] and kind not in ("gn", "patch_gn"):
                continue                      # the GroupNorm is not fused on this tile: another test's business
            worst = max(worst, data.run(tile, feat, v))
            ran[(kind, feat)] += 1
    torch.cuda.synchronize()
    print(f"kernargs {case.name} {dtname}: " + ", ".join(f"{k}/{f} x{n}" for (k, f), n in sorted(ran.items())) + f"; worst err/bound {worst:.3f}")
    for feat in feats:
        for fam in families:
            assert ran[(fam, feat)] > 0, f"{case.name} {feat}: no {fam} kernel accepted it"
