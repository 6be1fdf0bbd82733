"""Host-only pin of everything idb_gemm's planner decides (no GPU call): for a fixed enumeration of descriptors — the SD-2.1-base layer
shapes at B_eff 2 / 16 / 42 / 128 in f16 and bf16, every forced tile id 0..109 crossed with split_k, and the GroupNorm-in / LayerNorm-fold
/ row-statistics / flags / fp32-output variants — the plan, the workspace size and every idb_gemm_* query must equal the recorded
fixture tests/golden/gemm_plan_table.json.gz.

idb_gemm itself is probed only where it fails before any HIP call: every probed descriptor carries a defect that idb_gemm rejects with
IDB_EINVAL right after the check under test (gn_in_gamma null after the fused-GroupNorm refusal, ln_tiles = 0 after the LayerNorm-fold
refusal, a misaligned row_stats_out after the row-statistics refusal), so it returns -2 (refused) or -1 (accepted) and never launches.
The w_groups refusal comes after the last such check and is therefore not probed here.

Regenerate (only when a planner change is intended): python tests/test_plan_table_cpu.py"""
import ctypes as C
import gzip
import io
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from faceposegenerator_amd import _lib as L  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "gemm_plan_table.json.gz")
PTR = 1 << 20          # any non-null 16-byte-aligned address: the planner never dereferences

# (name, out_h, srcs [(channels, taps, upsample)], n, stride)
CONVS = [
    ("conv_64_320", 64, [(320, 9, 0)], 320, 1),
    ("conv_32_320_640", 32, [(320, 9, 0)], 640, 1),
    ("conv_32_640", 32, [(640, 9, 0)], 640, 1),
    ("conv_16_1280", 16, [(1280, 9, 0)], 1280, 1),
    ("conv_8_1280", 8, [(1280, 9, 0)], 1280, 1),
    ("conv2_sc_32", 32, [(640, 9, 0), (320, 1, 0)], 640, 1),
    ("conv2_sc_16", 16, [(1280, 9, 0), (640, 1, 0)], 1280, 1),
    ("cat_8", 8, [(1280, 9, 0), (1280, 9, 0)], 1280, 1),
    ("cat_32", 32, [(640, 9, 0), (320, 9, 0)], 640, 1),
    ("cat_64", 64, [(320, 9, 0), (320, 9, 0)], 320, 1),
    ("conv2_cat_sc_64", 64, [(320, 9, 0), (320, 1, 0), (320, 1, 0)], 320, 1),
    ("down_64", 32, [(320, 9, 0)], 320, 2),
    ("down_16", 8, [(1280, 9, 0)], 1280, 2),
    ("up_16", 32, [(1280, 9, 1)], 1280, 1),
    ("up_32", 64, [(640, 9, 1)], 640, 1),
    ("vae_64_512", 64, [(512, 9, 0)], 512, 1),
]
LINEARS = [   # (name, rows per sample, K, n, geglu): a plain [B_eff * rows][K] matrix, or (grid=True) a 1x1 conv on the square latent grid
    ("qkv_64", 4096, 320, 960, 0),
    ("out_64", 4096, 320, 320, 0),
    ("geglu_64", 4096, 320, 2560, 1),
    ("ffout_64", 4096, 1280, 320, 0),
    ("qkv_32", 1024, 640, 1920, 0),
    ("geglu_32", 1024, 640, 5120, 1),
    ("ffout_32", 1024, 2560, 640, 0),
    ("qkv_16", 256, 1280, 3840, 0),
    ("geglu_16", 256, 1280, 10240, 1),
    ("ffout_16", 256, 5120, 1280, 0),
    ("kv_ctx", 77, 1024, 640, 0),
    ("clip_qkv", 77, 1024, 3072, 0),
    ("clip_fc2", 77, 4096, 1024, 0),
    ("temb", 1, 1280, 1280, 0),
    ("small_n", 4096, 320, 32, 0),
]
PROJ_IN = [("proj_in_64", 64, 320), ("proj_in_32", 32, 640), ("proj_in_16", 16, 1280)]
BATCHES = [2, 16, 42, 128]
DTYPES = [L.IDB_F16, L.IDB_BF16]
FORCED_SHAPES = ["conv_64_320", "conv_8_1280", "conv2_sc_32", "qkv_64", "geglu_32", "ffout_16", "proj_in_32"]
SPLITS = [0, 1, 2, 3, 5, 8]
VARIANT_SPLITS = [0, 3, 8]       # forced ids: the variants of _variants() at these split_k values, the plain descriptor at all


def _desc(shape, b, dt, grid=False):
    d = L.GemmDesc()
    d.dtype, d.batch, d.w, d.out, d.out_dtype, d.w_layout = dt, b, PTR, PTR, dt, 1
    kind, spec = shape
    if kind == "conv":
        _, oh, srcs, n, stride = spec
        d.out_h = d.out_w = oh
        d.stride, d.n, d.nsrc = stride, n, len(srcs)
        for i, (ch, taps, up) in enumerate(srcs):
            ih = (oh * stride) >> up if taps == 9 else oh
            d.src[i].ptr, d.src[i].channels, d.src[i].taps, d.src[i].in_h, d.src[i].in_w, d.src[i].upsample = PTR, ch, taps, ih, ih, up
    else:
        _, rows, k, n, geglu = spec
        side = int(round(rows ** 0.5))
        grid = grid and side * side == rows
        d.out_h = d.out_w = side if grid else 1
        d.batch = b if grid else b * rows
        d.stride, d.n, d.nsrc, d.geglu = 1, n, 1, geglu
        d.src[0].ptr, d.src[0].channels, d.src[0].taps, d.src[0].in_h, d.src[0].in_w = PTR, k, 1, d.out_h, d.out_w
    d.out_ld = d.n // 2 if d.geglu else d.n
    return d


def _gn_in(d, nsrc):
    d.gn_in_partials, d.gn_in_chunks, d.gn_in_groups, d.gn_in_eps = PTR, min(64, max(1, d.out_h * d.out_w // 64)), 32, 1e-5
    d.gn_in_beta, d.gn_in_silu, d.gn_in_nsrc = PTR, 1, nsrc
    d.gn_in_gamma = 0                  # idb_gemm probe: IDB_EINVAL right after the fusion check, before any launch


def _variants(shape, d0):
    """(suffix, mutate, probe idb_gemm) for one base descriptor."""
    kind, spec = shape
    out = [("", None, False), ("/f32", lambda d: setattr(d, "out_dtype", L.IDB_F32), False)]
    for f in (4, 16, 256):
        out.append((f"/flags{f}", lambda d, f=f: setattr(d, "flags", f), False))
    out.append(("/gnp", lambda d: (setattr(d, "gn_partials", PTR), setattr(d, "gn_groups", 32)), False))
    out.append(("/gnp_f1", lambda d: (setattr(d, "gn_partials", PTR), setattr(d, "gn_groups", 32), setattr(d, "flags", 1)), False))

    def rows(d, flags=0):
        d.row_stats_out, d.flags = PTR + 4, flags           # misaligned: IDB_EINVAL right after the refusal check
        if flags & 16:
            d.counters, d.counters_len = PTR, 1 << 30
    out.append(("/rows", rows, True))
    out.append(("/rows_f16", lambda d: rows(d, 16), True))
    if kind == "lin" or d0.nsrc == 1 and d0.src[0].taps == 1:
        def ln(d, flags=0):
            d.ln_stats, d.ln_u, d.ln_v, d.ln_eps, d.ln_tiles, d.flags = PTR, PTR, PTR, 1e-5, 0, flags   # ln_tiles 0: IDB_EINVAL after
        out.append(("/ln", ln, True))
        out.append(("/ln_f256", lambda d: ln(d, 256), True))
        out.append(("/ln_bias", lambda d: (ln(d), setattr(d, "bias", PTR)), True))
    if d0.stride == 1 and not d0.geglu and d0.out_h > 1 and all(d0.src[i].upsample == 0 for i in range(d0.nsrc)):
        out.append(("/gn", lambda d: _gn_in(d, 1), True))
        if d0.nsrc > 1:
            out.append(("/gn_all", lambda d: _gn_in(d, d0.nsrc), True))
    return out


def _shapes():
    s = {name: ("conv", (name, *rest)) for name, *rest in CONVS}
    s.update({name: ("lin", (name, *rest)) for name, *rest in LINEARS})
    s.update({name: ("conv", (name, oh, [(c, 1, 0)], c, 1)) for name, oh, c in PROJ_IN})
    return s


def _record(lib, d, probe):
    t, sk, bl = C.c_int32(), C.c_int32(), C.c_int32()
    rc = lib.idb_gemm_plan(C.byref(d), C.byref(t), C.byref(sk), C.byref(bl))
    r = [rc, t.value, sk.value, bl.value] if rc == 0 else [rc, 0, 0, 0]
    r += [lib.idb_gemm_workspace_bytes(C.byref(d)), lib.idb_gemm_fuses_groupnorm(C.byref(d)), lib.idb_gemm_folds_layernorm(C.byref(d)),
          lib.idb_gemm_emits_gn_partials(C.byref(d), 32), lib.idb_gemm_row_stats_tiles(C.byref(d))]
    if probe:
        assert d.gn_in_gamma is None if d.gn_in_partials else (d.ln_tiles == 0 if d.ln_stats else d.row_stats_out % 8 != 0)
        g = lib.idb_gemm(C.byref(d), C.c_void_p(PTR), C.c_size_t(1 << 60), None)
        assert g in (-1, -2), g        # never 0: the descriptor is invalid past the refusal checks
        r.append(g)
    return r


def table():
    lib = L.load()
    shapes = _shapes()
    res = {}

    def add(key, shape, b, dt, tile, split_k, grid=False, variants=True):
        d0 = _desc(shape, b, dt, grid)
        for suffix, mut, probe in _variants(shape, d0) if variants else [("", None, False)]:
            d = _desc(shape, b, dt, grid)
            d.tile, d.split_k = tile, split_k
            if mut:
                mut(d)
            res[key + suffix] = _record(lib, d, probe)

    for name, shape in shapes.items():
        for b in BATCHES:
            for dt in DTYPES:
                add(f"{name}/b{b}/dt{dt}", shape, b, dt, 0, 0)
                if shape[0] == "lin":
                    add(f"{name}/grid/b{b}/dt{dt}", shape, b, dt, 0, 0, grid=True)
    for name in FORCED_SHAPES:
        for tile in range(110):
            for sk in SPLITS:
                for b in (2, 128):
                    add(f"{name}/b{b}/t{tile}/sk{sk}", shapes[name], b, L.IDB_F16, tile, sk, variants=sk in VARIANT_SPLITS)
    return res


def test_plan_table_matches_the_fixture():
    with gzip.open(FIXTURE, "rt") as f:
        want = json.load(f)
    got = table()
    assert sorted(got) == sorted(want)
    diff = [k for k in want if got[k] != want[k]]
    assert not diff, [(k, want[k], got[k]) for k in diff[:20]]


if __name__ == "__main__":
    t = table()
    with open(FIXTURE, "wb") as raw, gzip.GzipFile(fileobj=raw, mode="wb", mtime=0) as gz, io.TextIOWrapper(gz) as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v, separators=(',', ':'))}" for k, v in t.items()) + "\n}\n")
    print(f"{len(t)} descriptors -> {FIXTURE}")
