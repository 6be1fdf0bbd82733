"""Every case of the weight-packing / latent-path kernel test matrix (tests/prep_matrix.py) on the device, through the C ABI, element by
element, for f16 and bf16 wherever the entry takes an operand dtype, against the criteria derived there: bit-equality (pack_conv_weight,
pack_matrix, cast_f32 against the one rounding to nearest even; both transposes; tile_weight with its zero rows; postprocess against the
definition restated in numpy float32, over the 2^21-input threshold sweep too; vae_sample's mean and logvar), membership in the set of
the two admissible roundings (pack_matrix_scaled, lora_merge_scaled at rank 0, embed_tokens), gamma_n bounds with n counted from the
kernels (lora_merge and lora_merge_scaled, ln_fold_vectors, cfg_ddpm_step) and the emulated-exp allowance (vae_sample's latents).

Every output buffer (cfg_ddpm_step's in-place latents included) lies between 64 guard elements of a NaN bit pattern and is pre-filled with
that pattern (postprocess' bytes: once with 0xA5 and once with 0x5A); after the launch the guards are unchanged, and an element the kernel
did not write fails its criterion.  The kernels that store element by element (the packers, the merges, the cast) also run once with the
destination one element past a 16-byte boundary.  A failure names the case, the worst element's index, its error and its bound.
test_summary prints the worst err / bound per kernel and dtype and which rounding the three scaled or merged packers produced.

Measured on MI355X, 206 tests, all passing (worst err / bound and its case; recorded here and in profiles/prep/README.md, never used as
thresholds):

  idb_lora_merge          f16 0.9825  33 x 64 rank 16, scale -1.75      bf16 0.9765  33 x 64 rank 16, scale 0.5
  idb_lora_merge_scaled   f16 0.9925  5 x 130 rank 3, scale -1.75       bf16 0.9783  5 x 130 rank 3, scale 0.5
                          (the rounding to T, whose term u_T |ref| a correctly rounded value attains)
  idb_ln_fold_vectors     u  f16 0.0225  6 x 65 rank 3     bf16 0.0049  96 x 200 rank 16 GEGLU;     v  f16 0.0728  bf16 0.0728  32 x 64 GEGLU
  idb_cfg_ddpm_step       latents 0.4381  (1, 4, 257) no guidance, v-prediction, noise, t 999;   x0 0.8860  (2, 4, 64) no guidance,
                          v-prediction, t 999 (n = 2; the unfused numpy emulation gives the same two figures)
  idb_vae_sample          0.4898  (1, 4, 257) with noise;   0.9743 with noise = NULL (one rounding)

Bit-equal everywhere it is asked, at both destination alignments.  Where the two admissible roundings differ: idb_pack_matrix_scaled and
idb_lora_merge_scaled at rank 0 rounded ONCE in f16 (1530 of 1530 and 386 of 386 planted elements) and TWICE, through fp32, in bf16 (the
same counts); idb_embed_tokens rounded twice in both dtypes (13 and 12 elements).  With rank > 0 no tie can be planted behind a rounded
sum; the compiled f16 merges end in the same fused multiply-add-and-convert as the f16 scaled packer, the bf16 ones in an fp32
multiply or fma and a conversion."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import matrix_common as MC  # noqa: E402
import prep_matrix as P  # noqa: E402
from faceposegenerator_amd import _lib as L  # noqa: E402

pytestmark = pytest.mark.gpu

W = MC.Worst("prep matrix")
_ROUNDING = {}          # kernel and dtype -> [elements rounded once, elements rounded through fp32] where the two differ
_EXACT = {}             # kernel and dtype -> bit-equal cases


def _exact(kernel, what, got, want, mask=None):
    """MC.same_bits, counted per kernel for the summary."""
    MC.same_bits(what, got, want, mask)
    _EXACT[kernel] = _EXACT.get(kernel, 0) + 1


def _member(kernel, what, bits, exact, dt):
    ok, bad, n_once, n_twice = P.member(bits, exact, dt)
    print(f"{what}: where the two roundings differ, {n_once} elements rounded once and {n_twice} through fp32")
    if not ok:
        once, twice = P.admissible(exact, dt)
        got = np.asarray(bits).reshape(once.shape)
        assert ok, f"{what}: element {bad} is {int(got[bad]):#06x}; one rounding gives {int(once[bad]):#06x}, two give {int(twice[bad]):#06x}"
    r = _ROUNDING.setdefault(kernel, [0, 0])
    r[0] += n_once
    r[1] += n_twice


SHIFTS = (0, 1)


# ---- the packers ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", P.DTYPES)
@pytest.mark.parametrize("shape", P.PACK_CONV_SHAPES, ids=str)
def test_pack_conv_weight(lib, shape, dt):
    cout, cin, taps = shape
    src = MC.dev(P.pack_conv_input(shape))
    for shift in SHIFTS:
        what = f"idb_pack_conv_weight {shape} {dt} shift {shift}"
        out = MC.Guarded(src.numel(), 2, shift=shift)
        L.check(lib.idb_pack_conv_weight(src.data_ptr(), out.ptr, cout, cin, taps, MC.IDB[dt], MC.stream()), what)
        torch.cuda.synchronize()
        _exact(f"idb_pack_conv_weight {dt}", what, out.raw(what), P.pack_conv_reference(shape, dt))


@pytest.mark.parametrize("dt", P.DTYPES)
@pytest.mark.parametrize("shape", P.PACK_MATRIX_SHAPES, ids=str)
def test_pack_matrix(lib, shape, dt):
    rows, cols, geglu = shape
    src = MC.dev(P.matrix_inputs(shape)[0])
    for shift in SHIFTS:
        what = f"idb_pack_matrix {shape} {dt} shift {shift}"
        out = MC.Guarded(rows * cols, 2, shift=shift)
        L.check(lib.idb_pack_matrix(src.data_ptr(), out.ptr, rows, cols, geglu, MC.IDB[dt], MC.stream()), what)
        torch.cuda.synchronize()
        _exact(f"idb_pack_matrix {dt}", what, out.raw(what), P.pack_matrix_reference(shape, dt))


@pytest.mark.parametrize("dt", P.DTYPES)
@pytest.mark.parametrize("shape", P.PACK_MATRIX_SHAPES, ids=str)
def test_pack_matrix_scaled(lib, shape, dt):
    rows, cols, geglu = shape
    src, cs = (MC.dev(v) for v in P.matrix_inputs(shape, dt))
    for shift in SHIFTS:
        what = f"idb_pack_matrix_scaled {shape} {dt} shift {shift}"
        out = MC.Guarded(rows * cols, 2, shift=shift)
        L.check(lib.idb_pack_matrix_scaled(src.data_ptr(), out.ptr, rows, cols, geglu, cs.data_ptr(), MC.IDB[dt], MC.stream()), what)
        torch.cuda.synchronize()
        _member(f"idb_pack_matrix_scaled {dt}", what, out.raw(what), P.pack_scaled_exact(shape, dt), dt)


@pytest.mark.parametrize("dt", P.DTYPES)
@pytest.mark.parametrize("case", P.lora_cases(), ids=lambda c: c.name)
def test_lora_merge(lib, case, dt):
    rows, cols, _ = case.shape
    w, a, b, cs = (MC.dev(v) for v in P.lora_inputs(case, dt))
    pa, pb = (None, None) if case.rank0 else (a.data_ptr(), b.data_ptr())
    name = "idb_lora_merge_scaled" if case.scaled else "idb_lora_merge"
    for shift in SHIFTS:
        what = f"{name} {case.name} {dt} shift {shift}"
        out = MC.Guarded(rows * cols, 2, shift=shift)
        if case.scaled:
            L.check(lib.idb_lora_merge_scaled(w.data_ptr(), pa, pb, out.ptr, rows, cols, case.rank, case.scale, cs.data_ptr(), MC.IDB[dt], MC.stream()), what)
        else:
            L.check(lib.idb_lora_merge(w.data_ptr(), pa, pb, out.ptr, rows, cols, case.rank, case.scale, MC.IDB[dt], MC.stream()), what)
        torch.cuda.synchronize()
        bits = out.raw(what)
        if case.rank0:
            _member(f"{name} rank 0 {dt}", what, bits, P.lora_exact(case, dt), dt)
        else:
            ref, bound = P.lora_reference(case, dt)
            W.judge(f"{name} {dt}", what, P.from_bits(bits, dt).reshape(ref.shape), ref, bound)


@pytest.mark.parametrize("dt", P.DTYPES)
@pytest.mark.parametrize("shape", P.LORA_SHAPES, ids=str)
def test_lora_merge_scaled_by_one_is_pack_matrix(lib, shape, dt):
    """rank 0 and a column scale of exactly 1: the product is exact, the output is idb_pack_matrix's bit for bit."""
    rows, cols, _ = shape
    what = f"idb_lora_merge_scaled {shape} {dt} rank 0, col_scale 1"
    w = MC.dev(P.lora_inputs(P.LoraCase(shape, 0.5, True, True))[0])
    ones = torch.ones(cols, dtype=torch.float32, device=MC.DEV)
    merged, packed = MC.Guarded(rows * cols, 2), MC.Guarded(rows * cols, 2)
    L.check(lib.idb_lora_merge_scaled(w.data_ptr(), None, None, merged.ptr, rows, cols, 0, -1.75, ones.data_ptr(), MC.IDB[dt], MC.stream()), what)
    L.check(lib.idb_pack_matrix(w.data_ptr(), packed.ptr, rows, cols, 0, MC.IDB[dt], MC.stream()), what)
    torch.cuda.synchronize()
    _exact(f"idb_lora_merge_scaled rank 0 {dt}", what, merged.raw(what), packed.raw(what))
    _exact(f"idb_lora_merge_scaled rank 0 {dt}", what, merged.raw(what), P.to_bits(w.cpu().numpy(), dt))


@pytest.mark.parametrize("dt", P.DTYPES)
@pytest.mark.parametrize("shape", P.TILE_SHAPES, ids=str)
def test_tile_weight(lib, shape, dt):
    n, k = shape
    what = f"idb_tile_weight {shape} {dt}"
    src = MC.dev(P.tile_input(shape), np.uint16)
    need = lib.idb_tiled_weight_bytes(n, k)
    assert need == P.tiled_bytes(n, k) and src.data_ptr() % 16 == 0
    out = MC.Guarded(need // 2, 2)
    L.check(lib.idb_tile_weight(src.data_ptr(), out.ptr, n, k, MC.IDB[dt], MC.stream()), what)
    torch.cuda.synchronize()
    _exact(f"idb_tile_weight {dt}", what, out.raw(what), P.tile_reference(shape))


@pytest.mark.parametrize("dt", P.DTYPES)
@pytest.mark.parametrize("case", P.FOLD_CASES, ids=lambda c: c.name)
def test_ln_fold_vectors(lib, case, dt):
    what = f"idb_ln_fold_vectors {case.name} {dt}"
    w, a, b, wq, beta, bias = P.fold_inputs(case, dt)
    dw, dbeta, dbias, dwq = MC.dev(w), MC.dev(beta), MC.dev(bias), MC.dev(P.to_bits(wq, dt))
    da, db = (MC.dev(a), MC.dev(b)) if case.rank else (None, None)
    u, v = MC.Guarded(case.rows), MC.Guarded(case.rows)
    L.check(lib.idb_ln_fold_vectors(dw.data_ptr(), None if case.null_a else MC.ptr(da), MC.ptr(db), case.rank, P.FOLD_SCALE, dwq.data_ptr(), dbeta.data_ptr(),
                                    dbias.data_ptr() if case.bias else None, u.ptr, v.ptr, case.rows, case.cols, case.geglu, MC.IDB[dt], MC.stream()), what)
    torch.cuda.synchronize()
    ru, bu, rv, bv = P.fold_reference(case, dt)
    W.judge(f"idb_ln_fold_vectors u {dt}", what + " u", u.f32(what), ru, bu)
    W.judge(f"idb_ln_fold_vectors v {dt}", what + " v", v.f32(what), rv, bv)


# ---- the API boundary ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", P.DTYPES)
@pytest.mark.parametrize("count", P.CAST_COUNTS)
def test_cast_f32(lib, count, dt):
    x = MC.dev(P.cast_input(count))
    want, mask = P.cast_reference(count, dt)
    for shift, fill in ((0, P.NAN16), (1, P.NAN16), (0, 0x3C00)):           # 0x3C00 is no NaN in either dtype: an unwritten NaN element shows
        what = f"idb_cast_f32 {count} {dt} shift {shift} prefill {fill:#x}"
        out = MC.Guarded(count, 2, pattern=fill, shift=shift)
        L.check(lib.idb_cast_f32(x.data_ptr(), out.ptr, count, MC.IDB[dt], MC.stream()), what)
        torch.cuda.synchronize()
        bits = out.raw(what)
        _exact(f"idb_cast_f32 {dt}", what, bits, want, mask)
        nan = np.isnan(P.from_bits(bits, dt))
        assert np.array_equal(nan, ~mask), f"{what}: a NaN input must give a NaN, and nothing else may (elements {np.flatnonzero(nan != ~mask)[:4]})"


@pytest.mark.parametrize("dt", ("f32",) + P.DTYPES)
@pytest.mark.parametrize("shape", P.TRANSPOSE_SHAPES, ids=str)
def test_nhwc_to_nchw(lib, shape, dt):
    b, hw, c = shape
    name = "idb_f32_nhwc_to_nchw" if dt == "f32" else "idb_nhwc_to_nchw_f32"
    what = f"{name} {shape} {dt}"
    x = P.transpose_input(shape, dt)
    dx = MC.dev(x) if dt == "f32" else MC.dev(x, np.uint16)
    out = MC.Guarded(x.size)
    if dt == "f32":
        L.check(lib.idb_f32_nhwc_to_nchw(dx.data_ptr(), out.ptr, b, hw, c, MC.stream()), what)
    else:
        L.check(lib.idb_nhwc_to_nchw_f32(dx.data_ptr(), out.ptr, b, hw, c, MC.IDB[dt], MC.stream()), what)
    torch.cuda.synchronize()
    _exact(f"{name} {dt}", what, out.raw(what), P.transpose_reference(shape, dt).view(np.uint32))


@pytest.mark.parametrize("dt", P.DTYPES)
@pytest.mark.parametrize("shape", P.EMBED_SHAPES, ids=str)
def test_embed_tokens(lib, shape, dt):
    batch, n_tokens, dim, vocab = shape
    what = f"idb_embed_tokens {shape} {dt}"
    ids, tok, pos = P.embed_inputs(shape, dt)
    assert ids.min() >= 0 and ids.max() < vocab
    dids, dtok, dpos = MC.dev(ids), MC.dev(tok), MC.dev(pos)
    assert dtok.data_ptr() % 16 == 0 and dpos.data_ptr() % 16 == 0
    out = MC.Guarded(ids.size * dim, 2)
    L.check(lib.idb_embed_tokens(dids.data_ptr(), dtok.data_ptr(), dpos.data_ptr(), out.ptr, batch, n_tokens, dim, MC.IDB[dt], MC.stream()), what)
    torch.cuda.synchronize()
    _member(f"idb_embed_tokens {dt}", what, out.raw(what), P.embed_exact(shape, dt), dt)


@pytest.mark.parametrize("outputs", ("both", "u8_only", "img_only"))
@pytest.mark.parametrize("name", list(P.POST_CASES))
def test_postprocess(lib, name, outputs):
    x = P.POST_CASES[name]()
    dx = MC.dev(x)
    ref_v, ref_u8 = P.post_reference(name)
    for fill in (0xA5, 0x5A):
        what = f"idb_postprocess {name} {outputs} prefill {fill:#x}"
        img = MC.Guarded(x.size) if outputs != "u8_only" else None
        u8 = MC.Guarded(x.size, 1, pattern=fill) if outputs != "img_only" else None
        L.check(lib.idb_postprocess(dx.data_ptr(), img.ptr if img else None, u8.ptr if u8 else None, x.size, MC.stream()), what)
        torch.cuda.synchronize()
        if img:
            _exact("idb_postprocess img01", what + " img01", img.raw(what), ref_v.view(np.uint32))
        if u8:
            _exact("idb_postprocess u8", what + " u8", u8.raw(what), ref_u8)


# ---- the latent path -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ("noise_all", "noise_mean_only", "noise_logvar_only", "noise_latents_only", "mode_all", "mode_latents_only"))
@pytest.mark.parametrize("shape", P.VAE_SHAPES, ids=str)
def test_vae_sample(lib, shape, mode):
    b, c, hw = shape
    what = f"idb_vae_sample {shape} {mode}"
    with_noise = mode.startswith("noise")
    moments, noise = P.vae_inputs(shape)
    dm, dn = MC.dev(moments), (MC.dev(noise) if with_noise else None)
    lat = MC.Guarded(b * c * hw)
    mean = MC.Guarded(b * c * hw) if mode.endswith(("all", "mean_only")) else None
    lv = MC.Guarded(b * c * hw) if mode.endswith(("all", "logvar_only")) else None
    L.check(lib.idb_vae_sample(dm.data_ptr(), MC.ptr(dn), P.VAE_SCALE, lat.ptr, mean.ptr if mean else None, lv.ptr if lv else None, b, c, hw, MC.stream()), what)
    torch.cuda.synchronize()
    ref, bound, rmean, rlv = P.vae_reference(shape, with_noise)
    W.judge("idb_vae_sample" + ("" if with_noise else " mode"), what, lat.f32(what).reshape(ref.shape), ref, bound)
    if mean:
        _exact("idb_vae_sample mean", what + " mean", mean.raw(what), rmean.view(np.uint32))
    if lv:
        _exact("idb_vae_sample logvar", what + " logvar", lv.raw(what), rlv.view(np.uint32))


@pytest.mark.parametrize("case", P.cfg_cases(), ids=lambda c: c.name)
def test_cfg_ddpm_step(lib, case):
    what = f"idb_cfg_ddpm_step {case.name}"
    b, c, hw = case.shape
    eps, lat, noise = P.cfg_inputs(case.shape)
    deps = MC.dev(eps if case.cfg else eps[:b])                               # without guidance the kernel is handed the one half only
    dnoise, dcoef = (MC.dev(noise) if case.noise else None), MC.dev(case.coef)
    latents = MC.Guarded(lat.size, init=lat)
    x0 = MC.Guarded(lat.size) if case.x0 else None
    L.check(lib.idb_cfg_ddpm_step(deps.data_ptr(), latents.ptr, MC.ptr(dnoise), dcoef.data_ptr(), x0.ptr if x0 else None, b, c, hw, case.cfg, case.vpred, MC.stream()), what)
    torch.cuda.synchronize()
    prev, bp, r0, b0 = P.cfg_reference(case)
    W.judge("idb_cfg_ddpm_step latents", what + " latents", latents.f32(what).reshape(prev.shape), prev, bp)
    if x0:
        W.judge("idb_cfg_ddpm_step x0", what + " x0", x0.f32(what).reshape(r0.shape), r0, b0)


def test_summary():
    W.show()
    for k in sorted(_EXACT):
        print(f"prep matrix: {k}: bit-equal in {_EXACT[k]} comparisons")
    for k in sorted(_ROUNDING):
        once, twice = _ROUNDING[k]
        kind = "one rounding" if once and not twice else "two roundings (fp32, then T)" if twice and not once else "mixed" if once else "not separated"
        print(f"prep matrix: {k}: {kind} ({once} elements equal the once-rounded value, {twice} the twice-rounded one, where they differ)")
