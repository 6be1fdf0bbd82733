"""The launch geometry idb_gemm resolves on the host (GemmParams: idb_fill_geometry / idb_fastdiv.h) at the smallest shapes where its
arithmetic can go wrong: output grids that are no power of two (12x12: 64-row tiles straddle samples and the last tile is partial; 7x7:
several samples in one tile, the per-row sample-bias path), stride 2 and upsampled sources, K ranges of a split that start inside a
tap, inside the second K segment and inside a patch chunk, the three XCD remaps, and every tile family that decodes rows or seeks in K
(3-stage ring, 4-loader 4-stage loader-wave, fused GroupNorm through normalizer waves, patch-resident small tiles plain and with the
GroupNorm fused) with the epilogue paths that divide (per-sample bias, residual, folded LayerNorm, row statistics, GroupNorm partials
from the epilogue and from the reduce launch's blocked slabs, fp32 output, grouped weights).

Forced tile ids on raw descriptors, the float64 reference and the element-wise bounds are those of tests/gemm_matrix.py and of
test_gemm_matrix_gpu.CaseData (imported, unchanged).  Every combination runs TWICE into NaN-filled buffers and the two outputs must be
equal; where DESIGN states two families bit-identical — a loader-wave tile and the ring tile of the same shape and split — their outputs
must be equal bit for bit as well.

IDB_GEOMETRY_DIGESTS=<file>: also write one SHA-1 per output (A/B of two builds of the library through IDB_LIB: the files must be equal)."""
import hashlib
import json
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_matrix as GM  # noqa: E402
from gemm_matrix import Case, _conv  # noqa: E402
from test_gemm_matrix_gpu import DEV, DTYPES, CaseData  # noqa: E402

pytestmark = pytest.mark.gpu

# ring3, lw 4x4 and patch-small tiles of the 64x64 / 64x160 / 64x128 / 128x160 / 128x128 shapes
RING3 = [14, 16, 17, 18, 19]
LW = [74, 76, 77, 78, 79]
PATCH = [104, 106, 107, 108, 109]
TILES = RING3 + LW + PATCH
EPILOGUES = ["plain", "res", "sb", "f32", "gnp", "rows", "ln", "wgroups", "tiled_res_sb", "res_sb_gnp"]
FUSED_GN = ["gn", "gn_nosilu", "gn2", "gn_gnp"]


def _grid(name, b, h, w, cin, n, split_k=0):
    return Case(name, b, h, w, n, ((cin, 1, h, w, 0),), split_k=split_k)


CASES = [
    # ---- grids that are no power of two: M = 432 (7 row tiles of 64, the last partial; 14 workgroups at N 160: not a multiple of 8)
    _grid("g12_n160", 3, 12, 12, 64, 160),
    _grid("g12_n192", 3, 12, 12, 64, 192),
    _conv("c12_n160", 3, 12, 12, 64, 160),
    _conv("c12_s2", 3, 24, 24, 64, 160, stride=2),
    _conv("c12_up", 3, 6, 6, 64, 192, up=1),
    # ---- 7x7, batch 5: M = 245, five samples in four 64-row tiles
    _grid("g7_n160", 5, 7, 7, 64, 160),
    _conv("c7_n192", 5, 7, 7, 64, 192),
    _conv("c7_s2", 5, 14, 14, 64, 160, stride=2),
    # ---- K ranges: 9 K-steps at split 2 / 4 / 5; 3x3.64 + 1x1.128 (11 K-steps) at split 3: the third slice starts inside the second
    # segment; cat of two 3x3 sources at split 2: the second slice starts at the segment boundary
    _conv("k9_sk2", 2, 8, 8, 64, 160, split_k=2),
    _conv("k9_sk4", 2, 8, 8, 64, 160, split_k=4),
    _conv("k9_sk5", 2, 8, 8, 64, 160, split_k=5),
    _conv("k11_sk3", 2, 8, 8, 64, 160, extra=((128, 1),), split_k=3),
    Case("cat_sk2", 2, 8, 8, 128, ((64, 9, 8, 8, 0), (64, 9, 8, 8, 0)), split_k=2),
    Case("cat12_sk3", 3, 12, 12, 160, ((64, 9, 12, 12, 0), (128, 9, 12, 12, 0)), split_k=3),
    # ---- XCD remaps: split 8 on 54 K-steps (mode 1); split 4 on an even tile count (mode 2) and on an odd one (mode 0)
    _conv("k54_sk8", 2, 8, 8, 384, 160, split_k=8),
    _conv("k18_sk4_even", 2, 8, 8, 128, 128, split_k=4),
    _conv("k18_sk4_odd", 3, 12, 12, 128, 64, split_k=4),
    # ---- fused GroupNorm and the patch-resident tiles: 8x8, 16x16, 32x32; C 64 / 128 (groups of 2 / 4) and 192 (groups of 6)
    _conv("p8_c64", 2, 8, 8, 64, 160),
    _conv("p16_c128", 2, 16, 16, 128, 128, split_k=2),
    _conv("p32_c64", 1, 32, 32, 64, 160),
    _conv("p16_c192", 3, 16, 16, 192, 128),
    _grid("gn8_c64", 2, 8, 8, 64, 128),
    _grid("gn16_c64", 2, 16, 16, 64, 160),
    Case("gn2_16", 1, 16, 16, 128, ((128, 9, 16, 16, 0), (64, 9, 16, 16, 0))),
]

_DIGESTS = {}


@pytest.fixture(scope="module", autouse=True)
def _write_digests():
    yield
    path = os.environ.get("IDB_GEOMETRY_DIGESTS")
    if path:
        with open(path, "w") as f:
            json.dump(_DIGESTS, f, indent=0, sort_keys=True)


@pytest.mark.parametrize("dtname", list(DTYPES))
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_geometry(lib, monkeypatch, dtname, case):
    dt, tdt = DTYPES[dtname]
    data = CaseData(lib, case, dt, tdt, seed=4000 + CASES.index(case))
    seen = []                                             # the output tensor CaseData.run hands to the element-wise check
    check = GM.check
    monkeypatch.setattr(GM, "check", lambda out, *a, **k: (seen.append(out.clone()), check(out, *a, **k))[1])
    failures, outs, ran = [], {}, 0
    for feat in EPILOGUES + FUSED_GN:
        if not GM.applicable(case, feat):
            continue
        for tile in TILES:
            v = GM.classify(lib, case, dt, tile, feat)
            if not v.accepted:
                continue
            assert v.tile == tile
            try:
                del seen[:]
                data.run(tile, feat, v)
                data.run(tile, feat, v)
            except AssertionError as e:
                failures.append(str(e))
                continue
            ran += 1
            a, b = seen
            what = f"{case.name} {dtname} tile {tile} sk {v.split_k} {feat}"
            if not torch.equal(a.view(torch.uint8), b.view(torch.uint8)):
                failures.append(f"{what}: two runs differ")
            outs[(feat, tile)] = (a, v.split_k)
            _DIGESTS[what] = hashlib.sha1(a.cpu().view(torch.uint8).numpy().tobytes()).hexdigest()
    # loader-wave tile vs the ring tile of the same shape and split: bit-identical (DESIGN: same fragment mapping, accumulation order, epilogue)
    for (feat, tile), (a, sk) in outs.items():
        if tile in LW and feat not in FUSED_GN and (feat, tile - 60) in outs and outs[(feat, tile - 60)][1] == sk:
            if not torch.equal(a.view(torch.uint8), outs[(feat, tile - 60)][0].view(torch.uint8)):
                failures.append(f"{case.name} {dtname} {feat}: tile {tile} differs from ring tile {tile - 60} (split {sk})")
    torch.cuda.synchronize()
    assert ran > 0, f"{case.name}: no tile accepted"
    assert not failures, f"{len(failures)} failing combinations:\n" + "\n".join(failures[:30])


def test_every_family_and_path_ran(lib):
    """The list above must reach what it is written for: checked on the host, so a planner change that drops a path fails here."""
    dt = DTYPES["f16"][0]
    fams, feats, modes = set(), set(), set()
    for case in CASES:
        for feat in EPILOGUES + FUSED_GN:
            if not GM.applicable(case, feat):
                continue
            for tile in TILES:
                v = GM.classify(lib, case, dt, tile, feat)
                if v.accepted:
                    fams.add((GM.family_of(tile), "gn" if feat in FUSED_GN else "plain"))
                    feats.add(feat)
                    if v.split_k > 1:
                        tiles = -(-case.M // GM.tile_dims(tile)[0]) * -(-case.n // GM.tile_dims(tile)[1])
                        modes.add(1 if v.split_k % 8 == 0 else 2 if v.split_k == 4 and tiles % 2 == 0 else 0)
                        if feat in ("gnp", "res_sb_gnp"):
                            feats.add("gnp from the reduce launch" if v.emits_gn == 1 else "gnp by a statistics launch")
                    elif feat in ("gnp", "res_sb_gnp") and v.emits_gn == 2:
                        feats.add("gnp from the epilogue")
    assert fams >= {("ring3", "plain"), ("lw4x4", "plain"), ("lw4x4", "gn"), ("patch_small", "plain"), ("patch_small", "gn")}, fams
    assert feats >= set(EPILOGUES + FUSED_GN) | {"gnp from the reduce launch", "gnp from the epilogue"}, feats
    assert modes == {0, 1, 2}, modes
