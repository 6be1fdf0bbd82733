"""Host-only checks of the Python call path around idb_gemm (no GPU call):
  * the library's two queries about a grouped descriptor (w_groups > 1) — idb_gemm_row_stats_tiles, idb_gemm_folds_layernorm — answer
    0 exactly where idb_gemm refuses the grouped launch, by the rule the engine applied itself before the queries knew about groups;
  * _lib.gemm_desc, the one place the package fills an idb_gemm_desc, writes the bytes a field-by-field descriptor has."""
import ctypes as C

import pytest

from faceposegenerator_amd import _lib as L

PTR = 1 << 20          # any non-null 16-byte-aligned address: the planner never dereferences

# the LoRA-target projections of the UNet: (n, k, geglu)
PROJECTIONS = [(320, 320, 0), (960, 320, 0), (640, 1024, 0), (1280, 1280, 0), (2560, 320, 1)]
ROWS_PER_GROUP = [64, 77, 128, 4096]
# (rows per group, G, n, k, geglu): a GEGLU feed-forward large enough for the persistent variant
PERSISTENT = (32768, 2, 2560, 320, 1)
CASES = [(rpg, G, n, k, geglu) for rpg in ROWS_PER_GROUP for G in (2, 3) for (n, k, geglu) in PROJECTIONS] + [PERSISTENT]


def _linear(dt, rows, n, k, geglu, groups=0, rpg=0):
    d = L.GemmDesc()
    d.dtype, d.batch, d.out_h, d.out_w, d.stride, d.n, d.nsrc = dt, rows, 1, 1, 1, n, 1
    d.src[0].ptr, d.src[0].channels, d.src[0].taps, d.src[0].in_h, d.src[0].in_w = PTR, k, 1, 1, 1
    d.w, d.out, d.out_dtype, d.out_ld, d.geglu, d.w_layout = PTR, PTR, dt, (n // 2 if geglu else n), geglu, 1
    if groups:
        d.w_groups, d.w_group_rows, d.w_group_stride = groups, rpg, n * k * 2
    return d


def _per_group_by_the_engines_former_rule(tile_id, rpg):
    """What HipEngine.gemm computed from idb_gemm_plan's tile id (shape + 10 * family) to predict idb_gemm's refusal: the shape's tile
    height, doubled on the 256-row families 8 and 9; the persistent family 4 always runs per group.  (That code doubled family 10 as
    well, which is wrong; plain matrices never plan the patch-resident conv families 9 and 10, asserted here.)"""
    shape, fam = tile_id % 10, tile_id // 10
    assert fam < 9, tile_id
    bm = {1: 128, 2: 128, 3: 64, 4: 64, 5: 128, 6: 64, 7: 64, 8: 128, 9: 128}[shape] * (2 if fam == 8 else 1)
    return "persistent" if fam == 4 else "height" if rpg % bm else None


@pytest.mark.parametrize("dt", [L.IDB_F16, L.IDB_BF16], ids=["f16", "bf16"])
def test_grouped_queries_answer_zero_where_idb_gemm_refuses_the_grouped_launch(dt):
    lib = L.load()
    outcomes = {"height": 0, "persistent": 0, None: 0}
    zeroed = kept = 0          # answers the grouping turned to 0 / positive answers it left alone
    for rpg, G, n, k, geglu in CASES:
        rows = 2 * G * rpg                                      # CFG repeat 2
        plain, grouped = _linear(dt, rows, n, k, geglu), _linear(dt, rows, n, k, geglu, G, rpg)
        tile, tile_g = C.c_int32(), C.c_int32()
        assert lib.idb_gemm_plan(C.byref(plain), C.byref(tile), None, None) == 0
        assert lib.idb_gemm_plan(C.byref(grouped), C.byref(tile_g), None, None) == 0
        assert tile.value == tile_g.value                       # the planner does not read w_groups
        why = _per_group_by_the_engines_former_rule(tile.value, rpg)
        outcomes[why] += 1
        for query in (lib.idb_gemm_row_stats_tiles, lib.idb_gemm_folds_layernorm):
            base, got = query(C.byref(plain)), query(C.byref(grouped))
            assert got == (0 if why else base), (rpg, G, n, k, geglu, tile.value, why, base, got)
            zeroed += bool(why and base > 0)
            kept += bool(not why and base > 0)
    assert all(outcomes.values()), outcomes                     # refused for height, refused for persistent, one grouped launch
    assert zeroed and kept, (zeroed, kept)                      # and the answers are not 0 on both sides everywhere


# ---- gemm_desc -----------------------------------------------------------------------------------------------------------------------
def _src(d, i, ptr, ch, taps, ih, iw, up=0):
    d.src[i].ptr, d.src[i].channels, d.src[i].taps, d.src[i].in_h, d.src[i].in_w, d.src[i].upsample = ptr, ch, taps, ih, iw, up


def test_gemm_desc_two_source_stride2_conv_with_out2():
    """ArcFace block conv2 of a stage's first block: 3x3 stride 2 + the 1x1 downsample as a second K segment, the next bn1 as out2."""
    d = L.GemmDesc()
    d.dtype, d.batch, d.out_h, d.out_w, d.stride, d.n, d.nsrc = L.IDB_F16, 2, 28, 28, 2, 128, 2
    _src(d, 0, 0x10000, 128, 9, 56, 56)
    _src(d, 1, 0x20000, 64, 1, 56, 56)
    d.w, d.bias = 0x30000, 0x40000
    d.out, d.out_dtype, d.out_ld = 0x50000, L.IDB_F16, 128
    d.split_k, d.tile = 3, 14
    d.act, d.act_slope = 2, 0x60000
    d.out2, d.out2_scale, d.out2_shift = 0x70000, 0x80000, 0x90000
    got = L.gemm_desc(L.IDB_F16, [(0x10000, 128, 9, 56, 56), (0x20000, 64, 1, 56, 56)], 0x30000, 128, 2, 28, 28, stride=2, bias=0x40000,
                      out=0x50000, split_k=3, tile=14, act=2, act_slope=0x60000, out2=0x70000, out2_scale=0x80000, out2_shift=0x90000)
    assert bytes(got) == bytes(d)


def test_gemm_desc_conv_writing_a_column_slice():
    """HeadPose grouped block: group 1 of 2 writes its 128 output channels at column offset 128 of rows 256 wide."""
    d = L.GemmDesc()
    d.dtype, d.batch, d.out_h, d.out_w, d.stride, d.n, d.nsrc = L.IDB_BF16, 4, 28, 28, 1, 128, 1
    _src(d, 0, 0x10000, 128, 9, 28, 28)
    d.w, d.bias, d.out, d.out_dtype, d.out_ld = 0x30000 + 128 * 1152 * 2, 0x40000 + 128 * 4, 0x50000 + 128 * 2, L.IDB_BF16, 256
    d.act, d.split_k, d.tile = 3, 0, 0
    got = L.gemm_desc(L.IDB_BF16, [(0x10000, 128, 9, 28, 28)], 0x30000 + 128 * 1152 * 2, 128, 4, 28, 28, stride=1, bias=0x40000 + 128 * 4,
                      out=0x50000 + 128 * 2, out_ld=256, act=3, split_k=0, tile=0)
    assert bytes(got) == bytes(d)


def test_gemm_desc_geglu_linear_with_folded_layernorm():
    d = L.GemmDesc()
    d.dtype, d.batch, d.out_h, d.out_w, d.stride, d.n, d.nsrc = L.IDB_F16, 8192, 1, 1, 1, 2560, 1
    _src(d, 0, 0x10000, 320, 1, 1, 1, 0)
    d.w, d.bias, d.residual, d.geglu = 0x30000, None, None, 1
    d.out, d.out_dtype, d.out_ld = 0x50000, L.IDB_F16, 1280
    d.out_scale, d.flags, d.w_layout = 0.0, 256, 1
    d.counters, d.counters_len = 0x60000, 1 << 16
    d.ln_stats, d.ln_tiles, d.ln_u, d.ln_v, d.ln_eps = 0x70000, 2, 0x80000, 0x90000, 1e-5
    got = L.gemm_desc(L.IDB_F16, [(0x10000, 320, 1, 1, 1, 0)], 0x30000, 2560, 8192, 1, 1, bias=None, residual=None, geglu=1, out=0x50000,
                      out_ld=1280, out_scale=0.0, flags=256, w_layout=1, counters=0x60000, counters_len=1 << 16, ln_stats=0x70000,
                      ln_tiles=2, ln_u=0x80000, ln_v=0x90000, ln_eps=1e-5)
    assert bytes(got) == bytes(d)


def test_gemm_desc_grouped_linear():
    d = L.GemmDesc()
    d.dtype, d.batch, d.out_h, d.out_w, d.stride, d.n, d.nsrc = L.IDB_BF16, 256, 1, 1, 1, 960, 1
    _src(d, 0, 0x10000, 320, 1, 1, 1)
    d.w, d.out, d.out_dtype, d.out_ld, d.w_layout = 0x30000, 0x50000, L.IDB_F32, 960, 1
    d.sample_bias, d.sample_bias_ld, d.out_scale, d.pad_mode = 0x60000 + 4 * 40, 1280, 0.5, 1
    d.w_groups, d.w_group_rows, d.w_group_stride = 2, 64, 960 * 320 * 2
    got = L.gemm_desc(L.IDB_BF16, [(0x10000, 320, 1, 1, 1)], 0x30000, 960, 256, 1, 1, out=0x50000, out_dtype=L.IDB_F32, w_layout=1,
                      sample_bias=0x60000 + 4 * 40, sample_bias_ld=1280, out_scale=0.5, pad_mode=1, w_groups=2, w_group_rows=64,
                      w_group_stride=960 * 320 * 2)
    assert bytes(got) == bytes(d)


def test_gemm_desc_rejects_unknown_fields_and_too_many_sources():
    with pytest.raises(TypeError, match="out_lda"):
        L.gemm_desc(L.IDB_F16, [(PTR, 320, 1, 1, 1)], PTR, 320, 64, 1, 1, out=PTR, out_lda=320)
    with pytest.raises(TypeError, match="nsrc"):                # the positional fields are not settable by name
        L.gemm_desc(L.IDB_F16, [(PTR, 320, 1, 1, 1)], PTR, 320, 64, 1, 1, nsrc=2)
    with pytest.raises(ValueError, match="at most"):
        L.gemm_desc(L.IDB_F16, [(PTR, 64, 1, 1, 1)] * (L.IDB_MAX_SRC + 1), PTR, 320, 64, 1, 1)
