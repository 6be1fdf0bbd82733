"""The CPU half of the stem / linear / head kernel test matrix (tests/stem_matrix.py), no GPU: the bf16 bit arithmetic and the
single-rounding fma against torch and exact rationals, the float64 references against torch's own float64 operators, the conditions the
input recipes must meet (distinct slopes, both PReLU branches, the hand-worked split-K geometry against the library's host-only workspace
query, a well-conditioned six-vector), the teeth of the criteria (every non-harmless defect of stem_matrix.DEFECTS fails its named case;
the unmodified fp32 emulations pass every case with err / bound <= 0.5) and every argument check of the seven entry points, which answer
before any HIP call."""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import matrix_common as MC  # noqa: E402
import stem_matrix as S  # noqa: E402

T64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float64))   # noqa: E731
STEMS = [(k, s, e, dt) for k, shapes in (("arcface", S.ASTEM_SHAPES), ("pose", S.PSTEM_SHAPES)) for s in shapes for e in S.ENTRIES for dt in S.DTYPES]
W = MC.Worst("stem matrix, fp32 emulation")


# ---- number formats ------------------------------------------------------------------------------------------------------------------
def test_bf16_bit_rounding_is_torchs_cast():
    rng = np.random.default_rng(1)
    v = np.concatenate([rng.normal(size=4096) * 10.0 ** rng.integers(-30, 30, size=4096), [0.0, -0.0, 1.0, 3.4e38 * 0.99, 1e-40, -1e-45]]).astype(np.float32)
    ties = (np.arange(0x3F80, 0x3FA0, dtype=np.uint32) << 16 | 0x8000).view(np.float32)          # exactly half way: to even
    near = (np.arange(0x3F80, 0x3FA0, dtype=np.uint32) << 16 | 0x7FFF).view(np.float32)
    v = np.concatenate([v, ties, -ties, near, (near.view(np.uint32) + 2).view(np.float32)])
    want = torch.from_numpy(v).to(torch.bfloat16)
    assert np.array_equal(S.bf16_bits(v).view(np.int16), want.view(torch.int16).numpy())
    assert np.array_equal(S.round_T(v, "bf16"), want.float().numpy())
    h = torch.from_numpy(v).clamp(-6e4, 6e4)
    assert np.array_equal(S.to_bits(h.numpy(), "f16").view(np.int16), h.to(torch.float16).view(torch.int16).numpy())
    for dt in S.DTYPES:
        bits = np.arange(0, 0x7C00, 7, dtype=np.uint16)                # finite patterns round-trip
        assert np.array_equal(S.to_bits(S.from_bits(bits, dt), dt), bits)
        g = S.from_bits(np.array([S.NAN16], np.uint16), dt)
        assert np.isnan(g).all()
    assert np.isnan(np.array([S.NAN32], np.uint32).view(np.float32)).all()


def test_fma32_rounds_once():
    """Against exact rational arithmetic, on random operands and on operands built so that rounding the float64 sum first goes wrong."""
    rng = np.random.default_rng(2)
    a = rng.normal(size=2000).astype(np.float32)
    b = rng.normal(size=2000).astype(np.float32)
    c = (rng.normal(size=2000) * 10.0 ** rng.integers(-6, 3, size=2000)).astype(np.float32)
    # a = b = 1 + 2^-12: a b = 1 + 2^-11 + 2^-24, an fp32 tie (spacing 2^-23 at 1).  c = +-2^-60 decides it, but the float64 sum drops c,
    # and rounding that sum again goes to even whatever the sign of c
    a = np.concatenate([a, np.float32([1 + 2.0 ** -12, 1 + 2.0 ** -12])])
    b = np.concatenate([b, np.float32([1 + 2.0 ** -12, 1 + 2.0 ** -12])])
    c = np.concatenate([c, np.float32([2.0 ** -60, -2.0 ** -60])])
    got = S.fma32(a, b, c)
    naive = (a.astype(np.float64) * b + c).astype(np.float32)
    for i in range(a.size):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo = np.float32(float(exact))                                   # float(Fraction) rounds correctly to float64; decide around it
        cands = {np.float32(lo), np.nextafter(lo, np.float32(np.inf)), np.nextafter(lo, np.float32(-np.inf))}
        best = min(cands, key=lambda f: (abs(Fraction(float(f)) - exact), int(np.float32(f).view(np.uint32)) & 1))
        assert got[i] == best, (i, a[i], b[i], c[i])
    assert (naive[-2:] != got[-2:]).any()                               # the crafted operands do separate the two


# ---- the references against torch, float64 -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,shape,entry,dt", STEMS, ids=lambda v: str(v).replace(" ", ""))
def test_stem_reference_is_torch_conv2d(kind, shape, entry, dt):
    wt, bias, slope, _, _ = S.stem_params(kind)
    raw = S.stem_raw(kind, shape, entry)
    if entry == "u8":
        x = torch.from_numpy(raw).float() / 255.0                      # ToTensor / the ArcFace preprocessing, in torch float32
        if kind == "arcface":
            x = (x - 0.5) / 0.5
        else:
            x = (x - torch.tensor(S.POSE_MEAN)) / torch.tensor(S.POSE_STD)
        x = x.permute(0, 3, 1, 2)
    else:
        x = torch.from_numpy(raw)
    if kind == "arcface":
        x = x.to(torch.float16 if dt == "f16" else torch.bfloat16).float()
    taps = S.stem_taps(kind, shape, entry, dt)
    assert np.array_equal(taps, x.permute(0, 2, 3, 1).numpy()), "the restated normalisation is not torch's float32 one"
    want = F.conv2d(x.double(), T64(wt.transpose(0, 3, 1, 2)), T64(bias), stride=1 if kind == "arcface" else 2, padding=1)
    want = F.prelu(want, T64(slope)) if kind == "arcface" else F.relu(want)
    ref, bound, z = S.stem_reference(kind, shape, entry, dt)
    b, h, w = shape
    assert ref.shape == ((b, h, w, 64) if kind == "arcface" else (b, (h + 1) // 2, (w + 1) // 2, 64))
    scale = (bound - np.maximum(S.U_T[dt] * np.abs(ref), S.SUB_T[dt])) / S.gamma(28)          # >= S
    assert (bound > 0).all() and (np.abs(ref - want.permute(0, 2, 3, 1).numpy()) <= 1e-12 * scale).all()


def test_stem_recipes():
    for kind in ("arcface", "pose"):
        wt, bias, slope, s2, b2 = S.stem_params(kind)
        assert len(set(slope.tolist())) == 64 and (slope > 0).any() and (slope < -1).any() and (s2 < 0).any()
    for shape in S.ASTEM_SHAPES:
        for entry in S.ENTRIES:
            for dt in S.DTYPES:
                z = S.stem_reference("arcface", shape, entry, dt)[2].reshape(-1, 64)
                if z.shape[0] >= 8:                                     # both PReLU branches on every channel
                    assert (z > 0).any(0).all() and (z < 0).any(0).all(), (shape, entry, dt)
                else:                                                   # one pixel: one output per channel, both branches across channels
                    assert (z > 0).sum() >= 16 and (z < 0).sum() >= 16, (shape, entry, dt)
                if entry == "f32":                                      # the rounding of the input to T changes it
                    assert (S.stem_taps("arcface", shape, entry, dt) != S.stem_raw("arcface", shape, entry).transpose(0, 2, 3, 1)).mean() > 0.9
    assert max(w for _, _, w in S.ASTEM_SHAPES) == 256 and max(w for _, _, w in S.PSTEM_SHAPES) == 512
    assert any(w * 8 > 256 for _, _, w in S.ASTEM_SHAPES) and any((w + 1) // 2 * 8 > 256 for _, _, w in S.PSTEM_SHAPES)
    assert any(h % 2 and w % 2 for _, h, w in S.PSTEM_SHAPES) and any(h % 2 == 0 and w % 2 == 0 for _, h, w in S.PSTEM_SHAPES)


@pytest.mark.parametrize("case", S.conv_in_cases(), ids=lambda c: c.name)
def test_conv_in_reference_is_torch_conv2d(case):
    x, wt, bias, pre_w, pre_b = S.conv_in_inputs(case)
    b, cin, h, w, cout, rep = case.shape
    v = T64(x) * case.in_scale
    if case.pre:
        v = F.conv2d(v, T64(pre_w)[:, :, None, None], T64(pre_b))
    want = F.conv2d(v, T64(wt), T64(bias), padding=1).permute(0, 2, 3, 1).numpy()
    for dt in S.DTYPES:
        ref, bound = S.conv_in_reference(case, dt)
        assert ref.shape == (rep, b, h, w, cout) and (bound > 0).all()
        scale = (bound - np.maximum(S.U_T[dt] * np.abs(ref), S.SUB_T[dt])) / S.gamma(S.conv_in_roundings(case))
        assert (np.abs(ref - want[None]) <= 1e-12 * scale).all()
    assert S.conv_in_roundings(case) == 9 * cin + 1 + case.scale + (cin + 1) * case.pre
    assert (case.in_scale == 1.0) == (case.scale == 0)


def test_conv_in_cases_cover_what_they_were_chosen_for():
    cases = S.conv_in_cases()
    assert len({c.name for c in cases}) == len(cases) == 16
    assert {c.shape[1] for c in cases if c.pre} == {1, 3, 4} and {c.shape[5] for c in cases} == {1, 2}
    b, cin, h, w, cout, rep = S.CONV_IN_SHAPES[2]
    assert h * w == 272 and rep == 2 and (256 // (h * w)) != (255 + 256) // (h * w)          # the second 256-pixel block spans two samples
    assert all(c.shape[4] % 8 == 0 for c in cases)


@pytest.mark.parametrize("case", S.linear_cases(), ids=lambda c: c.name)
def test_linear_reference_is_torch_linear(case):
    x, wt, bias = S.linear_inputs(case)
    xin = F.silu(T64(x)) if case.silu else T64(x)
    want = F.linear(xin, T64(wt), None if bias is None else T64(bias)).numpy()
    ref, bound = S.linear_reference(case)
    assert ref.shape == case.shape[:2] and (bound > 0).all()
    assert (np.abs(ref - want) <= 1e-12 * bound / S.gamma(case.shape[2] + 7)).all()
    if case.silu:
        allow, r = S.silu_allowance(x)
        assert 4 * S.U <= allow <= 64 * S.U and r < 8 * S.U, (allow, r)       # the fp32 formula itself is good to a few ulp


def test_linear_cases_cover_what_they_were_chosen_for():
    shapes = S.LINEAR_SHAPES
    assert any(n % 4 for _, n, _ in shapes) and any(k % 64 and k > 64 for _, _, k in shapes) and any(m < 8 for m, _, _ in shapes)
    assert any(m % 8 and m > 8 for m, _, _ in shapes) and any(k < 64 for _, _, k in shapes)
    assert len(S.linear_cases()) == 20


@pytest.mark.parametrize("case", S.head_cases(), ids=lambda c: c.name)
def test_head_reference_and_geometry(lib, case):
    m, n, k = case.shape
    assert S.head_slices(m, n, k) == S.HEAD_SLICES[case.shape] and sum(S.HEAD_SLICES[case.shape]) * 32 == k
    assert lib.idb_arcface_head_workspace_bytes(m, n, k) == S.head_workspace_bytes(m, n, k) == len(S.HEAD_SLICES[case.shape]) * 4 * m * n
    for dt in S.DTYPES:
        x, wt, bias = S.head_inputs(case.shape, dt)
        assert np.array_equal(S.round_T(x, dt), x)
        ref, bound = S.head_reference(case, dt)
        want = F.linear(T64(x), T64(wt), T64(bias) if case.bias else None).numpy()
        assert ref.shape == (m, n) and (np.abs(ref - want) <= 1e-12 * bound / S.gamma(k + len(S.HEAD_SLICES[case.shape]) + 1)).all()


def test_head_restatement_over_a_grid(lib):
    for m in (1, 2, 63, 64, 65, 128, 129, 256):
        for n in (64, 128, 512):
            for k in (32, 224, 256, 288, 512, 544, 800, 25088):
                assert lib.idb_arcface_head_workspace_bytes(m, n, k) == S.head_workspace_bytes(m, n, k), (m, n, k)
                assert min(S.head_slices(m, n, k)) >= 1 and sum(S.head_slices(m, n, k)) == k // 32


@pytest.mark.parametrize("shape", S.PHEAD_SHAPES, ids=str)
@pytest.mark.parametrize("dt", S.DTYPES)
def test_pose_head_reference_and_conditioning(shape, dt):
    x, wt, bias = S.phead_inputs(shape, dt)
    b, hw, c = shape
    assert x.shape == shape and np.array_equal(S.round_T(x, dt), x)
    o6, d6 = S.phead_linear_reference(shape, dt)
    want = F.linear(T64(x).mean(1), T64(wt), T64(bias)).numpy()           # the layer mean and the linear layer
    assert (np.abs(o6 - want) <= 1e-12 * d6 / S.gamma(hw + c + 12)).all()
    assert np.abs(o6 - S.phead_targets(shape)).max() < 1e-3
    a, bb = o6[:, :3], o6[:, 3:]
    na, nb = np.linalg.norm(a, axis=1), np.linalg.norm(bb, axis=1)
    angle = np.degrees(np.arccos((a * bb).sum(1) / (na * nb)))
    rot, tol_r, ang, tol_a, _ = S.phead_reference(shape, dt)
    sy = np.hypot(rot[:, 0], rot[:, 3])
    assert (na >= 0.499).all() and (na <= 2.001).all() and (nb >= 0.499).all() and (nb <= 2.001).all()
    assert (angle >= 44.9).all() and (angle <= 135.1).all() and (sy >= 0.1).all() and (np.abs(ang) <= 61).all()
    r3 = rot.reshape(-1, 3, 3)
    assert np.abs(r3 @ r3.transpose(0, 2, 1) - np.eye(3)).max() < 1e-12 and (np.linalg.det(r3) > 0.999).all()
    # float64 Gram-Schmidt against torch's: normalize, cross
    ta, tb = T64(a), T64(bb)
    tx = F.normalize(ta, dim=1)
    tz = F.normalize(torch.linalg.cross(tx, tb), dim=1)
    ty = torch.linalg.cross(tz, tx)
    assert np.abs(torch.stack([tx, ty, tz], dim=2).reshape(-1, 9).numpy() - rot).max() < 1e-14
    assert (tol_r >= S.R_FLOOR).all() and (tol_a >= S.ANG_FLOOR).all() and tol_r.max() < 1e-2 and tol_a.max() < 1.0


@pytest.mark.parametrize("n,dim", S.SIN_SHAPES)
def test_sinusoid_reference_is_the_definition(n, dim):
    ref, bar, emu = S.sin_bound(n, dim)
    t = torch.from_numpy(S.sin_inputs(n)).double()
    half = dim // 2
    freq = torch.exp(-np.log(10000.0) * torch.arange(half, dtype=torch.float64) / half)
    a = t[:, None] * freq[None]
    want = torch.cat([torch.cos(a), torch.sin(a)], dim=1).numpy()
    assert ref.shape == (n, dim) and np.abs(ref - want).max() <= 1e-12
    assert S.SIN_FLOOR <= bar <= 3e-4 and emu <= 1e-4, (bar, emu)
    assert S.sin_inputs(6).tolist() == [0.0, 1.0, 34.0, 925.0, 958.0, 999.0]


# ---- teeth ---------------------------------------------------------------------------------------------------------------------------
def test_defect_list_is_complete():
    assert set(S.DEFECT_CASES) == set(S.DEFECTS) - set(S.HARMLESS) and len(S.DEFECTS) == 20 and S.HARMLESS == ("prelu_gt",)


@pytest.mark.parametrize("defect", [d for d in S.DEFECTS if d not in S.HARMLESS])
def test_every_defect_fails_its_named_case(defect):
    assert S.defect_fails(defect), (defect, S.DEFECT_CASES[defect])


def test_harmless_defect_changes_no_value():
    for shape in S.ASTEM_SHAPES:
        for entry in S.ENTRIES:
            for dt in S.DTYPES:
                a, b = S.emulate_stem("arcface", shape, entry, dt), S.emulate_stem("arcface", shape, entry, dt, defect="prelu_gt")
                assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (shape, entry, dt)
    z = np.float32([0.0, -0.0])
    assert np.array_equal(np.where(z > 0, z, z * np.float32(-1.3)) == 0, np.where(z >= 0, z, z * np.float32(-1.3)) == 0)


@pytest.mark.parametrize("kind,shape,entry,dt", STEMS, ids=lambda v: str(v).replace(" ", ""))
def test_stem_emulation_passes(kind, shape, entry, dt):
    ref, bound, _ = S.stem_reference(kind, shape, entry, dt, e_scale=0.5)      # half the fp32 allowance, the whole rounding to T
    out, out2 = S.emulate_stem(kind, shape, entry, dt)
    res = S.check(out, ref, bound)
    assert res[0], S.describe(f"{kind} stem {shape} {entry} {dt}", res)
    W.note(f"idb_{kind}_stem {dt}", res[1])
    if kind == "arcface":
        _, _, _, s2, b2 = S.stem_params(kind)
        assert np.array_equal(out2, S.out2_of(out, s2, b2, dt)) and np.array_equal(S.round_T(out2, dt), out2)


@pytest.mark.parametrize("case", S.conv_in_cases(), ids=lambda c: c.name)
def test_conv_in_emulation_passes(case):
    for dt in S.DTYPES:
        ref, bound = S.conv_in_reference(case, dt, e_scale=0.5)                   # half the fp32 allowance, the whole rounding to T
        res = S.check(S.emulate_conv_in(case, dt), ref, bound)
        assert res[0], S.describe(f"{case.name} {dt}", res)
        W.note(f"idb_conv_in {dt}", res[1])


@pytest.mark.parametrize("case", S.linear_cases(), ids=lambda c: c.name)
def test_linear_emulation_passes(case):
    ref, bound = S.linear_reference(case)
    res = S.check(S.emulate_linear(case), ref, bound)
    assert res[0] and res[1] <= 0.5, S.describe(case.name, res)
    W.note("idb_linear_f32", res[1])


@pytest.mark.parametrize("case", S.head_cases(), ids=lambda c: c.name)
def test_head_emulation_passes(case):
    for dt in S.DTYPES:
        ref, bound = S.head_reference(case, dt)
        res = S.check(S.emulate_head(case, dt), ref, bound)
        assert res[0] and res[1] <= 0.5, S.describe(f"{case.name} {dt}", res)
        W.note(f"idb_arcface_head {dt}", res[1])


@pytest.mark.parametrize("shape", S.PHEAD_SHAPES, ids=str)
def test_pose_head_emulation_passes(shape):
    for dt in S.DTYPES:
        rot, tol_r, ang, tol_a, _ = S.phead_reference(shape, dt)
        r, a = S.emulate_phead(shape, dt)
        for name, res in (("R", S.check(r, rot, tol_r)), ("angles", S.check(a, ang, tol_a))):
            assert res[0] and res[1] <= 0.5, S.describe(f"pose head {shape} {dt} {name}", res)
            W.note(f"idb_pose_head {name} {dt}", res[1])


@pytest.mark.parametrize("n,dim", S.SIN_SHAPES)
def test_sinusoid_emulation_passes(n, dim):
    ref, bar, _ = S.sin_bound(n, dim)
    res = S.check(S.emulate_sin(n, dim), ref, bar)
    assert res[0] and res[1] <= 0.5, S.describe(f"sinusoid {n} x {dim}", res)
    W.note("idb_timestep_sinusoid", res[1])


def test_summary():
    W.show()


# ---- argument checks: every IDB_REQUIRE of the seven entry points answers before any HIP call -----------------------------------------
P = MC.P16


def test_arcface_stem_argument_checks(lib):
    ok = dict(x=P, u8=1, batch=2, h=7, w=33, wt=P, bias=P, slope=P, s2=P, b2=P, out=P, out2=P, dtype=MC.IDB["f16"])
    call = lambda a: lib.idb_arcface_stem(a["x"], a["u8"], a["batch"], a["h"], a["w"], a["wt"], a["bias"], a["slope"], a["s2"], a["b2"],   # noqa: E731
                                          a["out"], a["out2"], a["dtype"], None)
    MC.refused(lib, call, ok, MC.BAD_DTYPES, "idb_arcface_stem: dtype")
    MC.refused(lib, call, ok, [dict(x=None), dict(wt=None), dict(bias=None), dict(slope=None), dict(out=None), dict(out=P + 8), dict(out2=P + 2)],
               "idb_arcface_stem: null or unaligned")
    MC.refused(lib, call, ok, [dict(s2=None), dict(b2=None), dict(s2=None, b2=None)], "idb_arcface_stem: out2 needs")
    MC.refused(lib, call, ok, [dict(w=257), dict(w=0), dict(h=0), dict(batch=0), dict(batch=65536), dict(batch=-1)], "idb_arcface_stem: batch 1..65535")


def test_pose_stem_argument_checks(lib):
    ok = dict(x=P, u8=1, batch=2, h=4, w=6, wt=P, bias=P, out=P, dtype=MC.IDB["bf16"])
    call = lambda a: lib.idb_pose_stem(a["x"], a["u8"], a["batch"], a["h"], a["w"], a["wt"], a["bias"], a["out"], a["dtype"], None)   # noqa: E731
    MC.refused(lib, call, ok, MC.BAD_DTYPES, "idb_pose_stem: dtype")
    MC.refused(lib, call, ok, [dict(x=None), dict(wt=None), dict(bias=None), dict(out=None), dict(out=P + 4)], "idb_pose_stem: null or unaligned")
    MC.refused(lib, call, ok, [dict(w=513), dict(w=0), dict(h=0), dict(batch=0), dict(batch=65536)], "idb_pose_stem: batch 1..65535")


def test_conv_in_argument_checks(lib):
    ok = dict(x=P, wt=P, bias=P, out=P, batch=2, rep=2, cin=4, h=9, w=31, cout=16, pw=P, pb=P, dtype=MC.IDB["f16"])
    call = lambda a: lib.idb_conv_in(a["x"], a["wt"], a["bias"], a["out"], a["batch"], a["rep"], a["cin"], a["h"], a["w"], a["cout"], 1.0,   # noqa: E731
                                     a["pw"], a["pb"], a["dtype"], None)
    MC.refused(lib, call, ok, MC.BAD_DTYPES, "idb_conv_in: dtype")
    MC.refused(lib, call, ok, [dict(x=None), dict(wt=None), dict(bias=None), dict(out=None), dict(out=P + 2)], "idb_conv_in: null/unaligned")
    MC.refused(lib, call, ok, [dict(cin=5), dict(cin=0), dict(cout=12), dict(cout=0), dict(batch=0), dict(rep=0), dict(h=0), dict(w=0)],
               "idb_conv_in: unsupported dims")
    MC.refused(lib, call, ok, [dict(pb=None), dict(pw=None)], "idb_conv_in: pre_w/pre_b")


def test_linear_and_sinusoid_argument_checks(lib):
    ok = dict(x=P, w=P, y=P, m=9, n=5, k=65)
    call = lambda a: lib.idb_linear_f32(a["x"], a["w"], None, a["y"], a["m"], a["n"], a["k"], 0, None)   # noqa: E731
    MC.refused(lib, call, ok, [dict(x=None), dict(w=None), dict(y=None), dict(m=0), dict(n=0), dict(k=0), dict(m=-1)], "idb_linear_f32: bad args")
    ok = dict(t=P, out=P, n=5, dim=6)
    call = lambda a: lib.idb_timestep_sinusoid(a["t"], a["out"], a["n"], a["dim"], None)   # noqa: E731
    MC.refused(lib, call, ok, [dict(dim=7), dict(dim=1), dict(dim=0), dict(n=0), dict(t=None), dict(out=None)], "idb_timestep_sinusoid: bad args")


def test_arcface_head_argument_checks(lib):
    need = S.head_workspace_bytes(3, 64, 544)
    ok = dict(x=P, wt=P, y=P, m=3, n=64, k=544, dtype=MC.IDB["f16"], ws=P, nbytes=need)
    call = lambda a: lib.idb_arcface_head(a["x"], a["wt"], None, a["y"], a["m"], a["n"], a["k"], a["dtype"], a["ws"], a["nbytes"], None)   # noqa: E731
    MC.refused(lib, call, ok, MC.BAD_DTYPES, "idb_arcface_head: dtype")
    MC.refused(lib, call, ok, [dict(n=96), dict(n=63), dict(k=560), dict(k=31), dict(m=0), dict(n=0), dict(k=0), dict(x=None), dict(wt=None), dict(y=None)],
               "idb_arcface_head: n % 64 == 0 and k % 32 == 0")
    MC.refused(lib, call, ok, [dict(nbytes=need - 1), dict(nbytes=0), dict(ws=None), dict(ws=P + 4)], "idb_arcface_head: workspace too small")
    assert lib.idb_arcface_head_workspace_bytes(3, 96, 544) == 0 and lib.idb_arcface_head_workspace_bytes(3, 64, 560) == 0


def test_pose_head_argument_checks(lib):
    ok = dict(x=P, batch=2, hw=7, c=64, wt=P, bias=P, rot=P, ang=P, dtype=MC.IDB["bf16"])
    call = lambda a: lib.idb_pose_head(a["x"], a["batch"], a["hw"], a["c"], a["wt"], a["bias"], a["rot"], a["ang"], a["dtype"], None)   # noqa: E731
    MC.refused(lib, call, ok, MC.BAD_DTYPES, "idb_pose_head: dtype")
    MC.refused(lib, call, ok, [dict(x=None), dict(x=P + 8), dict(wt=None), dict(bias=None), dict(rot=None), dict(ang=None)], "idb_pose_head: null or unaligned")
    MC.refused(lib, call, ok, [dict(c=12), dict(c=4), dict(c=0), dict(hw=0), dict(batch=0)], "idb_pose_head: batch > 0")
