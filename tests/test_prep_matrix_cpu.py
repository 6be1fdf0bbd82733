"""The CPU half of the weight-packing / latent-path kernel test matrix (tests/prep_matrix.py), no GPU: the roundings the criteria rest on
(once to T against numpy's float64 -> float16 cast and exact rationals, truncation, the planted pairs that separate one rounding from
two), the GEGLU row order written from the header against engine._geglu_perm and the kernel's own formula, the schedule coefficients
against scheduler.step_coefficients, the references against torch's float64 operators, what the input recipes were chosen for, the fused
and unfused uint8 forms over the threshold windows, the teeth (every defect of prep_matrix.DEFECTS fails its named case; the unmodified
emulations pass every case, the bounded ones within half their allowance) and every argument check of the fourteen entry points, the
2^39-element limit included, which answer before any HIP call."""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import matrix_common as MC  # noqa: E402
import prep_matrix as P  # noqa: E402

T64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float64))   # noqa: E731
F32, F64 = np.float32, np.float64
W = MC.Worst("prep matrix, fp32 emulation")


# ---- roundings -----------------------------------------------------------------------------------------------------------------------
def test_round_exact_is_one_rounding():
    rng = np.random.default_rng(3)
    x = rng.normal(size=20000) * 10.0 ** rng.integers(-4, 4, size=20000)
    x = np.concatenate([x, [1 + 2.0 ** -11 + 2.0 ** -40, 1 + 2.0 ** -11 - 2.0 ** -40, 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 2.0 ** -25 + 2.0 ** -60, 2.0 ** -25]])
    assert np.array_equal(P.round_exact_T(x, "f16"), x.astype(np.float16).view(np.uint16))        # numpy rounds float64 to float16 once
    for dt in P.DTYPES:                                                                            # and against exact rationals
        for v in x[-6:].tolist() + x[:200].tolist():
            got = float(P.from_bits(P.round_exact_T(np.array([v]), dt), dt)[0])
            b = int(P.round_exact_T(np.array([v]), dt)[0])
            cands = [float(P.from_bits(np.array([max(b + d, 0)], np.uint16), dt)[0]) for d in (-1, 0, 1)]
            best = min(abs(Fraction(c) - Fraction(v)) for c in cands)
            assert abs(Fraction(got) - Fraction(v)) == best, (dt, v)
    odd = P.f32_odd(x)
    assert (((odd.view(np.uint32) & 1) == 1) | (odd.astype(F64) == x)).all()
    assert (np.abs(odd.astype(F64) - x) <= np.spacing(np.abs(x).astype(F32)).astype(F64)).all()


def test_truncation_never_grows():
    v = (np.random.default_rng(4).normal(size=4000) * 3).astype(F32)
    for dt in P.DTYPES:
        t = P.from_bits(P.trunc_bits(v, dt), dt)
        assert (np.abs(t) <= np.abs(v)).all() and (np.abs(v) - np.abs(t) < 2 * P.U_T[dt] * np.abs(v) + 2.0 ** -24).all()
        assert (P.trunc_bits(v, dt) != P.to_bits(v, dt)).mean() > 0.3


@pytest.mark.parametrize("dt", P.DTYPES)
@pytest.mark.parametrize("kind", ("mul", "add"))
def test_planted_pairs_separate_one_rounding_from_two(dt, kind):
    a, b = P.twice_pairs(dt, kind)
    exact = a.astype(F64) * b.astype(F64) if kind == "mul" else a.astype(F64) + b.astype(F64)
    for i in range(4):                                                    # the float64 is the exact result
        fa, fb = Fraction(float(a[i])), Fraction(float(b[i]))
        assert Fraction(float(exact[i])) == (fa * fb if kind == "mul" else fa + fb)
    once, twice = P.admissible(exact, dt)
    assert (once != twice).all() and a.dtype == F32 and b.dtype == F32


# ---- GEGLU row order -----------------------------------------------------------------------------------------------------------------
def test_geglu_rows_agree_with_the_engine_and_the_kernel():
    from faceposegenerator_amd.engine import HipEngine
    for rows in (32, 64, 96, 160, 2560):
        want = P.geglu_rows(rows)
        assert sorted(want.tolist()) == list(range(rows))
        assert np.array_equal(want, HipEngine._geglu_perm(rows).numpy())
        p = np.arange(rows)
        blk, t = p >> 5, p & 31                                           # csrc/idb_misc.hip geglu_src_row
        assert np.array_equal(want, np.where(t < 16, 16 * blk + t, rows // 2 + 16 * blk + (t - 16)))
    assert np.array_equal(P.geglu_rows(32), np.arange(32))                # one group each: the identity, so 32 rows alone test nothing
    assert not np.array_equal(P.geglu_rows(64), P.geglu_rows(64, 32)) and not np.array_equal(P.geglu_rows(96), np.arange(96))
    assert (96 // 2) % 16 == 0 and (96 // 2) % 32 != 0


# ---- recipes -------------------------------------------------------------------------------------------------------------------------
def _sizes(shapes, n=None):
    return sorted(int(np.prod(s[:n])) for s in shapes)


def test_every_family_has_one_element_a_short_block_and_a_ragged_last_block():
    for name, sizes in (("pack_conv", _sizes(P.PACK_CONV_SHAPES)), ("pack_matrix", _sizes(P.PACK_MATRIX_SHAPES, 2)), ("lora", _sizes(P.LORA_SHAPES, 2)),
                        ("transpose", _sizes(P.TRANSPOSE_SHAPES)), ("vae", _sizes(P.VAE_SHAPES)), ("cfg", _sizes(P.CFG_SHAPES)),
                        ("post", sorted(P.POST_CASES[k]().size for k in ("one", "below256", "edge257"))), ("cast", list(P.CAST_COUNTS))):
        assert sizes[0] == 1 and any(1 < s < 256 for s in sizes) and any(s > 256 and 1 <= s % 256 <= 4 for s in sizes), (name, sizes)
    assert _sizes(P.EMBED_SHAPES, 3) == [4, 48, 2772] and all(s[2] % 4 == 0 for s in P.EMBED_SHAPES)      # / 4 threads: 1, 12, 693
    chunks = [(n + 15) // 16 * (k // 64) * 128 for n, k in P.TILE_SHAPES]
    assert chunks == [128, 128, 512, 256, 6144] and all(k % 64 == 0 for _, k in P.TILE_SHAPES)
    assert all(len({co, ci, t}) == 3 for co, ci, t in P.PACK_CONV_SHAPES[1:])
    assert all(2 <= c != hw for _, c, hw in P.VAE_SHAPES[1:]) and all(b >= 2 for b, *_ in P.EMBED_SHAPES[1:])
    assert P.post_sweep_input().size == 1 << 21 == max(P.POST_CASES[k]().size for k in P.POST_CASES)


def test_matrix_and_lora_recipes():
    for shape in P.PACK_MATRIX_SHAPES:
        for dt in P.DTYPES:
            src, cs = P.matrix_inputs(shape, dt)
            assert src.dtype == F32 and cs.dtype == F32 and (len(set(cs.tolist())) == cs.size)
            once, twice = P.admissible(P.pack_scaled_exact(shape, dt), dt)
            assert (once != twice).any(), (shape, dt)                      # the summary can tell the two roundings apart
    for case in P.lora_cases():
        if case.rank0:
            for dt in P.DTYPES:
                once, twice = P.admissible(P.lora_exact(case, dt), dt)
                assert (once != twice).any()
    cases = P.lora_cases()
    assert len(cases) == 25 and {c.scale for c in cases} == {0.5, -1.75} and sum(c.rank0 for c in cases) == 5
    assert P.lora_roundings(P.LoraCase((7, 37, 4), 0.5, True)) == 8 and P.lora_roundings(P.LoraCase((7, 37, 4), 0.5, False)) == 7


def test_embed_recipe_keeps_the_sum_exact():
    for shape in P.EMBED_SHAPES:
        for dt in P.DTYPES:
            ids, tok, pos = P.embed_inputs(shape, dt)
            batch, n_tokens, dim, vocab = shape
            assert ids.min() == 0 and ids.max() == vocab - 1 and (ids.size < 3 or ids[1] == ids[2])
            ea, eb = np.frexp(tok[ids])[1], np.frexp(pos[np.arange(ids.size) % n_tokens])[1]
            assert (tok != 0).all() and (pos != 0).all() and np.abs(ea - eb).max() <= 28
            exact = P.embed_exact(shape, dt)
            for r, c in ((0, 0), (ids.size - 1, dim - 1), (ids.size // 2, 1)):
                assert Fraction(float(exact[r, c])) == Fraction(float(tok[ids[r], c])) + Fraction(float(pos[r % n_tokens, c]))
            once, twice = P.admissible(exact, dt)
            assert (once != twice).any()


def test_cast_table_holds_the_edges():
    t = P.cast_table()
    assert t.size <= 255 and np.isnan(t).sum() == 3
    f16 = lambda v: int(P.to_bits(np.array([v], F32), "f16")[0])   # noqa: E731
    bf = lambda v: int(P.to_bits(np.array([v], F32), "bf16")[0])   # noqa: E731
    with np.errstate(over="ignore"):
        assert f16(1 + 2.0 ** -11) == 0x3C00 and f16(1 + 3 * 2.0 ** -11) == 0x3C02                  # ties to even, down and up
        assert f16(2.0 ** -24) == 1 and f16(2.0 ** -25) == 0 and f16(P._nb(F32(2.0 ** -25))) == 1
        assert f16(65504.0) == 0x7BFF and f16(65519.996) == 0x7BFF and f16(65520.0) == 0x7C00
        assert bf(1 + 2.0 ** -8) == 0x3F80 and bf(1 + 3 * 2.0 ** -8) == 0x3F82 and bf(P._nb(F32(1 + 2.0 ** -8))) == 0x3F81
        assert bf(float(np.finfo(F32).max)) == 0x7F80 and bf(float(P.from_bits(np.array([0x7F7F], np.uint16), "bf16")[0])) == 0x7F7F
        assert f16(-0.0) == 0x8000 and bf(-0.0) == 0x8000 and f16(-np.inf) == 0xFC00 and bf(np.inf) == 0x7F80
    for v in (1 + 2.0 ** -11, 2.0 ** -25, 65520.0, 1 + 2.0 ** -8, float(np.finfo(F32).tiny), 1e-40, 0.0, np.inf):
        assert (t == F32(v)).any() and (t == -F32(v)).any()
    want = torch.from_numpy(t.copy())
    for dt, tt in (("f16", torch.float16), ("bf16", torch.bfloat16)):
        bits, mask = P.cast_reference(t.size, dt)
        assert np.array_equal(bits[mask].view(np.int16), want.to(tt).view(torch.int16).numpy()[mask])


def test_coefficients_are_the_schedulers():
    """float64 against the scheduler's fp32 tensor arithmetic: the table is a product of up to 1000 fp32 roundings (1000 u = 6e-5) and
    1 - abar_t / abar_(t-1) cancels down to beta_1 = 8.5e-4, where one fp32 step of the quotient (6e-8) is 7e-5 of the result."""
    from faceposegenerator_amd.scheduler import DDPMScheduler
    sched = DDPMScheduler()
    for t in P.CFG_TIMESTEPS:
        got, want = P.ddpm_coefficients(t), sched.step_coefficients(t)
        assert np.allclose(got, want, rtol=1e-3, atol=0), (t, got, want)
    assert P.ddpm_coefficients(0)[4] == 0.0 and 0.06 < P.ddpm_coefficients(999)[0] < 0.08
    cases = P.cfg_cases()
    assert len({c.name for c in cases}) == len(cases) == 31
    first = cases[:16]
    assert len({(c.cfg, c.vpred, c.noise, c.x0) for c in first}) == 16 and {c.shape for c in first} == {(2, 3, 5)}
    assert {c.t for c in first} == set(P.CFG_TIMESTEPS) and {c.g for c in first} == set(P.GUIDANCE) == {0.0, 1.0, 5.0, 7.5}
    assert P.cfg_roundings(P.CfgCase((2, 3, 5), 1, 0, True, True, 999, 7.5)) == (6, 9) and P.cfg_roundings(P.CfgCase((2, 3, 5), 0, 1, False, True, 1, 0.0)) == (2, 4)


# ---- the references against torch, float64 -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", P.lora_cases(), ids=lambda c: c.name)
def test_lora_reference_is_torch(case):
    for dt in P.DTYPES:
        w, a, b, cs = P.lora_inputs(case, dt)
        want = T64(w) + float(F32(case.scale)) * (T64(b) @ T64(a)) if case.rank else T64(w)
        if case.scaled:
            want = want * T64(cs)
        if case.rank:
            ref, bound = P.lora_reference(case, dt)
            assert (bound > 0).all() and (np.abs(ref - want.numpy()) <= 1e-12 * bound).all()
        else:
            assert np.array_equal(P.lora_exact(case, dt), want.numpy())


@pytest.mark.parametrize("case", P.FOLD_CASES, ids=lambda c: c.name)
def test_fold_reference_is_torch(case):
    for dt in P.DTYPES:
        w, a, b, wq, beta, bias = P.fold_inputs(case, dt)
        assert np.array_equal(P.round_T(wq, dt), wq) and not np.array_equal(P.fold_unrounded(case), wq)
        sr = torch.from_numpy(P.geglu_rows(case.rows)) if case.geglu else torch.arange(case.rows)
        full = T64(w) + (float(F32(P.FOLD_SCALE)) * (T64(b) @ T64(a)) if case.eff_rank else 0.0)
        want_v = full[sr] @ T64(beta) + (T64(bias) if case.bias else 0.0)
        u, bu, v, bv = P.fold_reference(case, dt)
        assert (bu > 0).all() and (bv > 0).all()
        assert (np.abs(v - want_v.numpy()) <= 1e-9 * bv).all() and (np.abs(u - T64(wq).sum(1).numpy()) <= 1e-9 * bu).all()
    lanes = (case.cols + 63) // 64
    assert P.fold_roundings(case) == (lanes + 6, lanes + 8 + (case.rank + 2 if case.rank and not case.null_a else 0))


def test_fold_cases_cover_what_they_were_chosen_for():
    c = P.FOLD_CASES
    assert [(x.rows, x.cols, x.rank, x.geglu, x.bias) for x in c[:6]] == [(1, 1, 0, 0, True), (5, 63, 0, 0, True), (6, 65, 3, 0, True), (32, 64, 0, 1, True),
                                                                          (96, 200, 16, 1, True), (7, 320, 4, 0, False)]
    assert c[6].null_a and c[6].rank == 4 and c[6].eff_rank == 0 and any(x.rows % 4 for x in c)


@pytest.mark.parametrize("case", P.cfg_cases(), ids=lambda c: c.name)
def test_cfg_reference_is_the_schedulers_step(case):
    """Against the host branch of DDPMScheduler.step's formulas restated in torch float64 on the same fp32 coefficients."""
    sa, sb, c0, cx, sigma, g = (float(v) for v in case.coef)
    eps, lat, noise = (T64(v) for v in P.cfg_inputs(case.shape))
    b, c, hw = case.shape
    eu, ec = eps[:b].permute(0, 2, 1), eps[b:].permute(0, 2, 1)
    mo = eu + g * (ec - eu) if case.cfg else eu
    x0 = sa * lat - sb * mo if case.vpred else (lat - sb * mo) / sa
    prev = c0 * x0 + cx * lat + (sigma * noise if case.noise else 0.0)
    rp, bp, r0, b0 = P.cfg_reference(case)
    assert (bp > 0).all() and (b0 > 0).all()
    assert (np.abs(rp - prev.numpy()) <= 1e-9 * bp).all() and (np.abs(r0 - x0.numpy()) <= 1e-9 * b0).all()


@pytest.mark.parametrize("shape", P.VAE_SHAPES, ids=str)
def test_vae_reference_is_the_diagonal_gaussian(shape):
    b, c, hw = shape
    m, noise = P.vae_inputs(shape)
    mean, logvar = torch.chunk(T64(m).permute(0, 2, 1), 2, dim=1)          # diffusers DiagonalGaussianDistribution on NCHW moments
    logvar = torch.clamp(logvar, -30.0, 20.0)
    std = torch.exp(0.5 * logvar)
    s = float(F32(P.VAE_SCALE))
    ref, bound, mref, lref = P.vae_reference(shape, True)
    assert (np.abs(ref - ((mean + std * T64(noise)) * s).numpy()) <= 1e-9 * bound).all() and (bound > 0).all()
    assert np.array_equal(mref.astype(F64), mean.numpy()) and np.array_equal(lref.astype(F64), logvar.numpy())
    ref, bound, _, _ = P.vae_reference(shape, False)
    assert np.array_equal(ref, (mean * s).numpy())
    lv = m[:, :, c:].reshape(-1)
    if lv.size >= 20:
        assert (lv == -30).any() and (lv == 20).any() and (lv < -30).any() and (lv > 20).any() and ((lv > -30) & (lv < 20)).any()
    allow, r = P.vae_allowance(shape)
    assert 4 * P.U <= allow <= 32 * P.U and r <= 8 * P.U, (allow, r)


def test_bit_equal_references_are_torchs():
    for shape in P.PACK_CONV_SHAPES:
        src = torch.from_numpy(P.pack_conv_input(shape))
        for dt, tt in (("f16", torch.float16), ("bf16", torch.bfloat16)):
            want = src.permute(0, 2, 1).contiguous().to(tt).view(torch.int16).numpy()
            assert np.array_equal(P.pack_conv_reference(shape, dt).view(np.int16), want)
    for shape in P.TRANSPOSE_SHAPES:
        x = P.transpose_input(shape, "f32")
        assert np.array_equal(P.transpose_reference(shape, "f32"), torch.from_numpy(x).permute(0, 2, 1).contiguous().numpy())
        for dt, tt in (("f16", torch.float16), ("bf16", torch.bfloat16)):
            xb = torch.from_numpy(P.transpose_input(shape, dt).view(np.int16)).view(tt)
            want = xb.float().permute(0, 2, 1).contiguous().numpy()
            assert np.isfinite(want).all() and np.array_equal(P.transpose_reference(shape, dt).view(np.uint32), want.view(np.uint32))
    for shape in P.TILE_SHAPES:
        n, k = shape
        ref = P.tile_reference(shape)
        assert ref.size * 2 == P.tiled_bytes(n, k) and (P.tile_input(shape) != P.NAN16).all()
        for row, col in ((0, 0), (n - 1, k - 1), (n // 2, 65 % k)):
            assert ref[row // 16, col // 64, row % 16, col % 64] == P.tile_input(shape)[row, col]
        assert (ref.transpose(0, 2, 1, 3).reshape(-1, k)[n:] == 0).all()


def test_postprocess_reference_and_the_fused_form():
    """The oracle's mul(255).add_(0.5).clamp_(0, 255).to(uint8) in torch float32 is the reference's unfused form, and the fused sum gives
    the same byte over every threshold window (2,089,215 values of v)."""
    v = P.post_window_v()
    assert v.size == 255 * 8193 == 2089215 and (np.diff(v) > 0).all()
    assert P.post_fused_differs() == 0
    for name in ("edge257", "sweep"):
        x = P.POST_CASES[name]()
        img = (torch.from_numpy(x) / 2 + 0.5).clamp(0, 1)
        want = img.mul(255).add_(0.5).clamp_(0, 255).to(torch.uint8).numpy()
        ref_v, ref_u8 = P.post_reference(name)
        assert np.array_equal(ref_v, img.numpy()) and np.array_equal(ref_u8, want)
        assert np.array_equal(P.emulate_post(name, fused=True)[1], ref_u8)
    x = P.post_sweep_input()
    assert x.size == 1 << 21 and np.unique(x).size == x.size
    reached = np.unique(P.post_v(x))
    upper = v[v >= 0.5]                                                   # spacing 2^-24 there: 2 v - 1 is an fp32, every v is reached
    assert np.isin(upper, reached).all()
    lower = v[v < 0.5]                                                    # below, only the v that some x / 2 + 0.5 rounds to
    reachable = np.unique(P.post_v((2.0 * lower.astype(F64) - 1.0).astype(F32)))
    assert np.isin(reachable[np.isin(reachable, lower)], reached).all()
    ref_u8 = P.post_reference("sweep")[1]
    assert len(np.unique(ref_u8)) == 256                                  # both sides of every threshold
    edge = P.post_edge_input()
    assert edge.size == 257 and not np.isnan(edge).any() and np.isinf(edge).sum() == 2 and (edge == 2).any() and (edge == -2).any()
    assert np.signbit(edge[edge == 0]).tolist() == [False, True]


# ---- teeth ---------------------------------------------------------------------------------------------------------------------------
def test_defect_list_is_complete():
    assert set(P.DEFECT_CASES) == set(P.DEFECTS) - set(P.HARMLESS) and len(P.DEFECTS) == 25 and P.HARMLESS == ()


@pytest.mark.parametrize("defect", [d for d in P.DEFECTS if d not in P.HARMLESS])
def test_every_defect_fails_its_named_case(defect):
    assert P.defect_fails(defect), (defect, P.DEFECT_CASES[defect])


def test_bit_equal_emulations_pass():
    for dt in P.DTYPES:
        for shape in P.PACK_CONV_SHAPES:
            assert np.array_equal(P.emulate_pack_conv(shape, dt), P.pack_conv_reference(shape, dt))
        for shape in P.PACK_MATRIX_SHAPES:
            assert np.array_equal(P.emulate_pack_matrix(shape, dt), P.pack_matrix_reference(shape, dt))
    for name in P.POST_CASES:
        for fused in (False, True):
            v, u8 = P.emulate_post(name, fused=fused)
            assert np.array_equal(v.view(np.uint32), P.post_reference(name)[0].view(np.uint32)) and np.array_equal(u8, P.post_reference(name)[1])


@pytest.mark.parametrize("dt", P.DTYPES)
def test_set_membership_accepts_both_roundings_and_nothing_else(dt):
    for shape in P.PACK_MATRIX_SHAPES:
        exact = P.pack_scaled_exact(shape, dt)
        for fused in (False, True):
            ok, bad, n_once, n_twice = P.member(P.emulate_pack_scaled(shape, dt, fused=fused), exact, dt)
            assert ok and bad is None and (n_once > 0) == fused and (n_twice > 0) == (not fused), (shape, fused)
        bits = P.emulate_pack_scaled(shape, dt).copy()
        bits.reshape(-1)[-1] ^= 2                                          # two units in the last place of T off: next to neither admissible value
        assert not P.member(bits, exact, dt)[0]
    for shape in P.EMBED_SHAPES:
        ok, bad, n_once, n_twice = P.member(P.emulate_embed(shape, dt), P.embed_exact(shape, dt), dt)
        assert ok and n_once == 0 and n_twice > 0
    for case in P.lora_cases():
        if case.rank0:
            assert P.member(P.emulate_lora(case, dt), P.lora_exact(case, dt), dt)[0]


@pytest.mark.parametrize("case", [c for c in P.lora_cases() if c.rank], ids=lambda c: c.name)
def test_lora_emulation_passes(case):
    for dt in P.DTYPES:
        ref, bound = P.lora_reference(case, dt, e_scale=0.5)                # half the fp32 allowance, the whole rounding to T
        res = P.check(P.from_bits(P.emulate_lora(case, dt), dt).reshape(ref.shape), ref, bound)
        assert res[0], P.describe(f"{case.name} {dt}", res)
        W.note(f"idb_lora_merge{'_scaled' if case.scaled else ''} {dt}", res[1])


@pytest.mark.parametrize("case", P.FOLD_CASES, ids=lambda c: c.name)
def test_fold_emulation_passes(case):
    for dt in P.DTYPES:
        u, bu, v, bv = P.fold_reference(case, dt)
        eu, ev = P.emulate_fold(case, dt)
        for name, res in (("u", P.check(eu, u, bu)), ("v", P.check(ev, v, bv))):
            assert res[0] and res[1] <= 0.5, P.describe(f"{case.name} {dt} {name}", res)
            W.note(f"idb_ln_fold_vectors {name} {dt}", res[1])


@pytest.mark.parametrize("case", P.cfg_cases(), ids=lambda c: c.name)
def test_cfg_emulation_passes(case):
    prev, bp, x0, b0 = P.cfg_reference(case)
    ep, e0 = P.emulate_cfg(case)
    rp, r0 = P.check(ep, prev, bp), P.check(e0, x0, b0)
    assert rp[0] and rp[1] <= 0.5, P.describe(f"{case.name} latents", rp)
    assert r0[0], P.describe(f"{case.name} x0", r0)                         # sharp: see the module docstring
    W.note("idb_cfg_ddpm_step latents", rp[1])
    W.note("idb_cfg_ddpm_step x0", r0[1])


@pytest.mark.parametrize("shape", P.VAE_SHAPES, ids=str)
def test_vae_emulation_passes(shape):
    for with_noise in (True, False):
        ref, bound, mean, lv = P.vae_reference(shape, with_noise)
        z, m, l2 = P.emulate_vae(shape, with_noise)
        res = P.check(z, ref, bound)
        assert res[0] and (res[1] <= 0.5 or not with_noise), P.describe(f"vae {shape} noise {with_noise}", res)      # one rounding: sharp
        assert np.array_equal(m.view(np.uint32), mean.view(np.uint32)) and np.array_equal(l2.view(np.uint32), lv.view(np.uint32))
        W.note("idb_vae_sample" + ("" if with_noise else " mode"), res[1])


def test_summary():
    W.show()


# ---- argument checks: every IDB_REQUIRE of the fourteen entry points answers before any HIP call ---------------------------------------
P16 = MC.P16
BIG = 1 << 39


def _pos(fn):
    """The entry on an argument set's values: every `ok` below lists the arguments in the entry's order."""
    return lambda a: fn(*a.values())


def test_pack_conv_weight_argument_checks(lib):
    ok = dict(src=P16, dst=P16, cout=3, cin=5, taps=9, dtype=MC.IDB["f16"], stream=None)
    f = lib.idb_pack_conv_weight
    MC.refused(lib, _pos(f), ok, MC.BAD_DTYPES + [dict(src=None), dict(dst=None), dict(cout=0), dict(cin=0), dict(taps=0), dict(cout=-1)], "idb_pack_conv_weight: bad args")
    MC.refused(lib, _pos(f), ok, [dict(cout=1 << 13, cin=1 << 13, taps=1 << 13), dict(cout=2 ** 31 - 1, cin=2 ** 31 - 1, taps=2 ** 31 - 1), dict(cout=1 << 30, cin=1 << 9, taps=1)],
             "idb_pack_conv_weight: 2^39")


def test_pack_matrix_argument_checks(lib):
    for name, scaled in (("idb_pack_matrix", False), ("idb_pack_matrix_scaled", True)):
        ok = dict(src=P16, dst=P16, rows=64, cols=5, geglu=1, **({"cs": P16} if scaled else {}), dtype=MC.IDB["bf16"], stream=None)
        f = getattr(lib, name)
        MC.refused(lib, _pos(f), ok, MC.BAD_DTYPES + [dict(src=None), dict(dst=None), dict(rows=0), dict(cols=0), dict(cols=-3)] + ([dict(cs=None)] if scaled else []),
                 f"{name}: bad args")
        MC.refused(lib, _pos(f), ok, [dict(rows=48), dict(rows=16), dict(rows=33)], f"{name}: GEGLU")
        MC.refused(lib, _pos(f), ok, [dict(rows=1 << 20, cols=1 << 19), dict(rows=BIG, cols=1, geglu=0), dict(rows=1 << 32, cols=1 << 32), dict(rows=2 ** 63 - 1, cols=2 ** 63 - 1, geglu=0)],
                 f"{name}: 2^39")


def test_lora_merge_argument_checks(lib):
    ok = dict(w=P16, a=P16, b=P16, dst=P16, rows=7, cols=37, rank=4, scale=0.5, dtype=MC.IDB["f16"], stream=None)
    f = lib.idb_lora_merge
    MC.refused(lib, _pos(f), ok, MC.BAD_DTYPES + [dict(w=None), dict(a=None), dict(b=None), dict(dst=None), dict(rows=0), dict(cols=0), dict(rank=0), dict(rank=-1)],
             "idb_lora_merge: bad args")
    MC.refused(lib, _pos(f), ok, [dict(rows=1 << 20, cols=1 << 19), dict(rows=1 << 62, cols=4)], "idb_lora_merge: 2^39")
    ok = dict(w=P16, a=P16, b=P16, dst=P16, rows=7, cols=37, rank=4, scale=0.5, cs=P16, dtype=MC.IDB["bf16"], stream=None)
    f = lib.idb_lora_merge_scaled
    MC.refused(lib, _pos(f), ok, MC.BAD_DTYPES + [dict(w=None), dict(dst=None), dict(cs=None), dict(rows=0), dict(cols=0), dict(rank=-1), dict(a=None), dict(b=None), dict(a=None, b=None)],
             "idb_lora_merge_scaled: bad args")
    MC.refused(lib, _pos(f), ok, [dict(rows=1 << 20, cols=1 << 19), dict(rows=1 << 62, cols=4, rank=0, a=None, b=None)], "idb_lora_merge_scaled: 2^39")


def test_tile_weight_argument_checks(lib):
    ok = dict(src=P16, dst=P16, n=17, k=128, dtype=MC.IDB["f16"], stream=None)
    f = lib.idb_tile_weight
    MC.refused(lib, _pos(f), ok, MC.BAD_DTYPES + [dict(src=None), dict(dst=None), dict(n=0), dict(k=0), dict(k=96), dict(k=65), dict(src=P16 + 8), dict(dst=P16 + 2)],
             "idb_tile_weight: needs operand dtype")
    MC.refused(lib, _pos(f), ok, [dict(n=1 << 33, k=64), dict(n=(1 << 33) - 15, k=64), dict(n=2 ** 63 - 1, k=64), dict(n=3, k=1 << 36)], "idb_tile_weight: 2^39")
    for n, k in P.TILE_SHAPES + ((1 << 20, 1 << 12),):
        assert lib.idb_tiled_weight_bytes(n, k) == P.tiled_bytes(n, k)
    assert lib.idb_tiled_weight_bytes(0, 64) == 0 and lib.idb_tiled_weight_bytes(5, 0) == 0


def test_ln_fold_vectors_argument_checks(lib):
    ok = dict(w=P16, a=P16, b=P16, rank=4, scale=1.0, wq=P16, beta=P16, bias=P16, u=P16, v=P16, rows=96, cols=200, geglu=1, dtype=MC.IDB["f16"], stream=None)
    f = lib.idb_ln_fold_vectors
    MC.refused(lib, _pos(f), ok, MC.BAD_DTYPES + [dict(w=None), dict(wq=None), dict(beta=None), dict(u=None), dict(v=None), dict(rows=0), dict(cols=0), dict(rank=-1), dict(rank=17),
                                             dict(b=None)], "idb_ln_fold_vectors: bad args")
    MC.refused(lib, _pos(f), ok, [dict(rows=48), dict(rows=100)], "idb_ln_fold_vectors: GEGLU")
    MC.refused(lib, _pos(f), ok, [dict(rows=1 << 20, cols=1 << 19), dict(rows=1 << 33, cols=1, geglu=0), dict(rows=1 << 62, cols=1 << 62)], "idb_ln_fold_vectors: 2^39")


def test_cfg_ddpm_step_argument_checks(lib):
    ok = dict(eps=P16, lat=P16, noise=None, coef=P16, x0=None, batch=2, c=3, hw=5, cfg=1, pred=0, stream=None)
    f = lib.idb_cfg_ddpm_step
    MC.refused(lib, _pos(f), ok, [dict(eps=None), dict(lat=None), dict(coef=None), dict(batch=0), dict(c=0), dict(hw=0), dict(hw=-5)], "idb_cfg_ddpm_step: bad args")
    MC.refused(lib, _pos(f), ok, [dict(pred=2), dict(pred=-1)], "idb_cfg_ddpm_step: prediction_type")
    MC.refused(lib, _pos(f), ok, [dict(batch=1 << 13, c=1 << 13, hw=1 << 13), dict(batch=2 ** 31 - 1, c=2 ** 31 - 1, hw=2 ** 31 - 1)], "idb_cfg_ddpm_step: 2^39")


def test_vae_sample_argument_checks(lib):
    ok = dict(m=P16, noise=None, scale=0.18215, lat=P16, mean=None, lv=None, batch=2, c=3, hw=5, stream=None)
    f = lib.idb_vae_sample
    MC.refused(lib, _pos(f), ok, [dict(m=None), dict(lat=None), dict(batch=0), dict(c=0), dict(hw=0), dict(c=-4)], "idb_vae_sample: bad args")
    MC.refused(lib, _pos(f), ok, [dict(batch=1 << 13, c=1 << 13, hw=1 << 13), dict(batch=2 ** 31 - 1, c=2 ** 31 - 1, hw=2 ** 31 - 1), dict(batch=1, c=1 << 30, hw=1)], "idb_vae_sample: 2^39")


def test_postprocess_and_cast_argument_checks(lib):
    ok = dict(x=P16, img=P16, u8=P16, count=257, stream=None)
    f = lib.idb_postprocess
    MC.refused(lib, _pos(f), ok, [dict(x=None), dict(img=None, u8=None), dict(count=0), dict(count=-1)], "idb_postprocess: bad args")
    MC.refused(lib, _pos(f), ok, [dict(count=BIG), dict(count=2 ** 63 - 1)], "idb_postprocess: 2^39")
    ok = dict(x=P16, out=P16, count=257, dtype=MC.IDB["f16"], stream=None)
    f = lib.idb_cast_f32
    MC.refused(lib, _pos(f), ok, MC.BAD_DTYPES + [dict(x=None), dict(out=None), dict(count=0), dict(count=-7)], "idb_cast_f32: bad args")
    MC.refused(lib, _pos(f), ok, [dict(count=BIG), dict(count=2 ** 63 - 1)], "idb_cast_f32: 2^39")


def test_transpose_argument_checks(lib):
    ok = dict(x=P16, out=P16, batch=2, hw=3, c=5, dtype=MC.IDB["bf16"], stream=None)
    f = lib.idb_nhwc_to_nchw_f32
    MC.refused(lib, _pos(f), ok, MC.BAD_DTYPES + [dict(x=None), dict(out=None), dict(batch=0), dict(hw=0), dict(c=0)], "idb_nhwc_to_nchw_f32: bad args")
    MC.refused(lib, _pos(f), ok, [dict(batch=1 << 13, hw=1 << 13, c=1 << 13), dict(batch=2 ** 31 - 1, hw=2 ** 31 - 1, c=2 ** 31 - 1)], "idb_nhwc_to_nchw_f32: 2^39")
    ok = dict(x=P16, out=P16, batch=2, hw=3, c=5, stream=None)
    f = lib.idb_f32_nhwc_to_nchw
    MC.refused(lib, _pos(f), ok, [dict(x=None), dict(out=None), dict(batch=0), dict(hw=0), dict(c=0)], "idb_f32_nhwc_to_nchw: bad args")
    MC.refused(lib, _pos(f), ok, [dict(batch=1 << 13, hw=1 << 13, c=1 << 13), dict(batch=2 ** 31 - 1, hw=2 ** 31 - 1, c=2 ** 31 - 1)], "idb_f32_nhwc_to_nchw: 2^39")


def test_embed_tokens_argument_checks(lib):
    ok = dict(ids=P16, tok=P16, pos=P16, out=P16, batch=2, n=3, dim=8, dtype=MC.IDB["f16"], stream=None)
    f = lib.idb_embed_tokens
    MC.refused(lib, _pos(f), ok, MC.BAD_DTYPES + [dict(ids=None), dict(tok=None), dict(pos=None), dict(out=None)], "idb_embed_tokens: bad args")
    MC.refused(lib, _pos(f), ok, [dict(batch=0), dict(n=0), dict(dim=0), dict(dim=6), dict(dim=7), dict(tok=P16 + 4), dict(pos=P16 + 8), dict(out=P16 + 2)], "idb_embed_tokens: dims/alignment")
    MC.refused(lib, _pos(f), ok, [dict(batch=1 << 13, n=1 << 13, dim=1 << 13), dict(batch=1 << 16, n=1 << 15, dim=4), dict(batch=2 ** 31 - 1, n=2 ** 31 - 1, dim=2 ** 31 - 4)],
             "idb_embed_tokens: 2^39")
