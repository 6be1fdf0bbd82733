"""Every case of the stem / linear / head kernel test matrix (tests/stem_matrix.py) on the device, through the C ABI, element by element
against the float64 references and the criteria derived there (stems and conv_in: gamma_(K+1+a) S max(1, |slope|) and one rounding to T;
the ArcFace stem's out2: bit-equal to the single-rounding fma of the GPU's own `out`, and `out` bit-identical with out2 = NULL;
idb_arcface_head: gamma_(K+splits+1); idb_linear_f32: gamma_(K+7) plus the emulated silu allowance; idb_pose_head: delta6 propagated through
a float64 Jacobian plus 3x the fp32 emulation's error; idb_timestep_sinusoid: 3x the fp32 emulation's error).

Every output buffer, and the head's workspace (passed at exactly its stated size), lies between 64 guard elements of a NaN bit pattern and is
pre-filled with that pattern; after the launch the guards are unchanged, and an element the kernel did not write keeps its NaN and fails
its criterion.  A failure names the case, the worst element's index, its error and its bound.  test_summary prints the worst err / bound
per kernel and dtype.  Measured on MI355X, 128 cases, all passing (worst err / bound and its case; never used as thresholds):

  idb_arcface_stem        f16 0.9801  (1, 2, 256) u8          bf16 0.9949  (1, 2, 256) f32
  idb_pose_stem           f16 0.9877  (1, 3, 511) f32         bf16 0.9952  (1, 3, 511) u8
  idb_conv_in             f16 0.9859  b2 cin1 5x7, VAE scale, pre-conv       bf16 0.9934  b3 cin3 16x17 rep 2, pre-conv
                          (the three above are the rounding to T, whose term u_T |ref| a correctly rounded value attains)
  idb_arcface_head        f16 0.0440  bf16 0.0440  (1, 64, 32), no bias; 0.0025 at (130, 512, 800), 1e-5 at K = 25088
  idb_linear_f32          0.0296  (1, 1, 1);  silu_in 0.0692  (1, 1, 1)
  idb_pose_head           R f16 0.0226  bf16 0.0194;  angles f16 0.0199  bf16 0.0178  (all at (1, 1, 8))
  idb_timestep_sinusoid   0.3333  n 5 dim 6 (|err| 2.9e-6 against a bar of 8.6e-6); 0.2652 at dim 320 (4.2e-5 against 1.6e-4)

out2 was bit-equal to the host's single-rounding fma of the stored `out`, and `out` bit-identical without out2, on all 16 ArcFace stem cases.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import matrix_common as MC  # noqa: E402
import stem_matrix as S  # noqa: E402
from faceposegenerator_amd import _lib as L  # noqa: E402

pytestmark = pytest.mark.gpu

W = MC.Worst("stem matrix")


# ---- the stems -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", S.DTYPES)
@pytest.mark.parametrize("entry", S.ENTRIES)
@pytest.mark.parametrize("shape", S.ASTEM_SHAPES, ids=str)
def test_arcface_stem(lib, shape, entry, dt):
    what = f"idb_arcface_stem {shape} {entry} {dt}"
    b, h, w = shape
    wt, bias, slope, s2, b2 = S.stem_params("arcface")
    x, dw, db, dsl, ds2, db2 = (MC.dev(v) for v in (S.stem_raw("arcface", shape, entry), wt, bias, slope, s2, b2))
    n = b * h * w * 64
    out, out2, solo = MC.Guarded(n, 2), MC.Guarded(n, 2), MC.Guarded(n, 2)
    L.check(lib.idb_arcface_stem(x.data_ptr(), int(entry == "u8"), b, h, w, dw.data_ptr(), db.data_ptr(), dsl.data_ptr(), ds2.data_ptr(), db2.data_ptr(),
                                 out.ptr, out2.ptr, MC.IDB[dt], MC.stream()), what)
    L.check(lib.idb_arcface_stem(x.data_ptr(), int(entry == "u8"), b, h, w, dw.data_ptr(), db.data_ptr(), dsl.data_ptr(), None, None,
                                 solo.ptr, None, MC.IDB[dt], MC.stream()), what)
    torch.cuda.synchronize()
    (got, bits), (got2, bits2), (_, bits_solo) = out.T(what, dt), out2.T(what, dt), solo.T(what, dt)
    ref, bound, _ = S.stem_reference("arcface", shape, entry, dt)
    W.judge(f"idb_arcface_stem {dt}", what, got.reshape(ref.shape), ref, bound)
    assert np.isfinite(got2).all(), f"{what}: out2 has elements that were not written"
    want2 = S.to_bits(S.out2_of(got.reshape(-1, 64), s2, b2, dt), dt).reshape(-1)
    diff = np.argwhere(bits2 != want2)
    assert diff.size == 0, f"{what}: out2 element {int(diff[0, 0])} is {int(bits2[diff[0, 0]]):#06x}, fma of the stored out gives {int(want2[diff[0, 0]]):#06x}"
    assert np.array_equal(bits, bits_solo), f"{what}: out differs when out2 is NULL"


@pytest.mark.parametrize("dt", S.DTYPES)
@pytest.mark.parametrize("entry", S.ENTRIES)
@pytest.mark.parametrize("shape", S.PSTEM_SHAPES, ids=str)
def test_pose_stem(lib, shape, entry, dt):
    what = f"idb_pose_stem {shape} {entry} {dt}"
    b, h, w = shape
    wt, bias, _, _, _ = S.stem_params("pose")
    x, dw, db = (MC.dev(v) for v in (S.stem_raw("pose", shape, entry), wt, bias))
    ref, bound, _ = S.stem_reference("pose", shape, entry, dt)
    assert ref.shape == (b, (h + 1) // 2, (w + 1) // 2, 64)
    out = MC.Guarded(ref.size, 2)
    L.check(lib.idb_pose_stem(x.data_ptr(), int(entry == "u8"), b, h, w, dw.data_ptr(), db.data_ptr(), out.ptr, MC.IDB[dt], MC.stream()), what)
    torch.cuda.synchronize()
    W.judge(f"idb_pose_stem {dt}", what, out.T(what, dt)[0].reshape(ref.shape), ref, bound)


# ---- idb_conv_in ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", S.DTYPES)
@pytest.mark.parametrize("case", S.conv_in_cases(), ids=lambda c: c.name)
def test_conv_in(lib, case, dt):
    what = f"idb_conv_in {case.name} {dt}"
    b, cin, h, w, cout, rep = case.shape
    x, wt, bias, pre_w, pre_b = S.conv_in_inputs(case)
    dx, dw, db = MC.dev(x), MC.dev(wt), MC.dev(bias)
    dpw, dpb = (MC.dev(pre_w), MC.dev(pre_b)) if case.pre else (None, None)
    ref, bound = S.conv_in_reference(case, dt)
    assert ref.shape == (rep, b, h, w, cout)
    out = MC.Guarded(ref.size, 2)
    L.check(lib.idb_conv_in(dx.data_ptr(), dw.data_ptr(), db.data_ptr(), out.ptr, b, rep, cin, h, w, cout, case.in_scale,
                            dpw.data_ptr() if case.pre else None, dpb.data_ptr() if case.pre else None, MC.IDB[dt], MC.stream()), what)
    torch.cuda.synchronize()
    got, bits = out.T(what, dt)
    W.judge(f"idb_conv_in {dt}", what, got.reshape(ref.shape), ref, bound)
    bits = bits.reshape(rep, -1)
    assert all(np.array_equal(bits[0], bits[r]) for r in range(rep)), f"{what}: the copies of `rep` differ"


# ---- idb_linear_f32 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", S.linear_cases(), ids=lambda c: c.name)
def test_linear_f32(lib, case):
    what = f"idb_linear_f32 {case.name}"
    m, n, k = case.shape
    x, wt, bias = S.linear_inputs(case)
    dx, dw, db = MC.dev(x), MC.dev(wt), (None if bias is None else MC.dev(bias))
    out = MC.Guarded(m * n)
    L.check(lib.idb_linear_f32(dx.data_ptr(), dw.data_ptr(), None if db is None else db.data_ptr(), out.ptr, m, n, k, int(case.silu), MC.stream()), what)
    torch.cuda.synchronize()
    ref, bound = S.linear_reference(case)
    W.judge("idb_linear_f32" + (" silu_in" if case.silu else ""), what, out.f32(what).reshape(m, n), ref, bound)


# ---- idb_arcface_head ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", S.DTYPES)
@pytest.mark.parametrize("case", S.head_cases(), ids=lambda c: c.name)
def test_arcface_head(lib, case, dt):
    what = f"idb_arcface_head {case.name} {dt}"
    m, n, k = case.shape
    x, wt, bias = S.head_inputs(case.shape, dt)
    dx, dw, db = MC.dev(S.to_bits(x, dt)), MC.dev(wt), (MC.dev(bias) if case.bias else None)
    need = lib.idb_arcface_head_workspace_bytes(m, n, k)
    assert need == S.head_workspace_bytes(m, n, k) and need % 4 == 0
    out, ws = MC.Guarded(m * n), MC.Guarded(need // 4)
    L.check(lib.idb_arcface_head(dx.data_ptr(), dw.data_ptr(), None if db is None else db.data_ptr(), out.ptr, m, n, k, MC.IDB[dt], ws.ptr, need,
                                 MC.stream()), what)
    torch.cuda.synchronize()
    ref, bound = S.head_reference(case, dt)
    W.judge(f"idb_arcface_head {dt}", what, out.f32(what).reshape(m, n), ref, bound)
    assert np.isfinite(ws.f32(what + " workspace")).all(), f"{what}: a workspace element of a slice was not written"


# ---- idb_pose_head -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", S.DTYPES)
@pytest.mark.parametrize("shape", S.PHEAD_SHAPES, ids=str)
def test_pose_head(lib, shape, dt):
    what = f"idb_pose_head {shape} {dt}"
    b, hw, c = shape
    x, wt, bias = S.phead_inputs(shape, dt)
    dx, dw, db = MC.dev(S.to_bits(x, dt)), MC.dev(wt), MC.dev(bias)
    assert dx.data_ptr() % 16 == 0
    rot, ang = MC.Guarded(b * 9), MC.Guarded(b * 3)
    L.check(lib.idb_pose_head(dx.data_ptr(), b, hw, c, dw.data_ptr(), db.data_ptr(), rot.ptr, ang.ptr, MC.IDB[dt], MC.stream()), what)
    torch.cuda.synchronize()
    r64, tol_r, a64, tol_a, _ = S.phead_reference(shape, dt)
    W.judge(f"idb_pose_head R {dt}", what + " R", rot.f32(what).reshape(b, 9), r64, tol_r)
    W.judge(f"idb_pose_head angles {dt}", what + " angles", ang.f32(what).reshape(b, 3), a64, tol_a)


# ---- idb_timestep_sinusoid -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,dim", S.SIN_SHAPES)
def test_timestep_sinusoid(lib, n, dim):
    what = f"idb_timestep_sinusoid n {n} dim {dim}"
    t = MC.dev(S.sin_inputs(n))
    out = MC.Guarded(n * dim)
    L.check(lib.idb_timestep_sinusoid(t.data_ptr(), out.ptr, n, dim, MC.stream()), what)
    torch.cuda.synchronize()
    ref, bar, emu = S.sin_bound(n, dim)
    print(f"{what}: bar {bar:.3e} (emulation {emu:.3e})")
    W.judge("idb_timestep_sinusoid", what, out.f32(what).reshape(n, dim), ref, bar)


def test_summary():
    W.show()
