"""The harness of the per-element test matrices (tests/matrix_common.py) tested itself, no GPU: that the verdicts reject what they are
there to reject (a NaN or an infinity left in an output, an error one ulp above its bound, a shape mismatch, a differing sign of zero),
that an overwritten guard element of a Guarded buffer is reported by name and an element never written fails `check`, that the 16-bit
conversions are torch's bit for bit, and that `refused` rejects every way an argument check can be missing."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import frtail_oracle as TO  # noqa: E402
import matrix_common as MC  # noqa: E402

F32, F64 = np.float32, np.float64


def _hashed(n, salt):
    """n finite fp32 values of both signs over 2^-13 .. 2^14 from the integer hash of frtail_oracle.py."""
    i = np.arange(n) + salt
    return ((TO._h(i, 2) << 31) | ((TO._h(i + n, 27) + 114) << 23) | TO._h(i + 2 * n, 1 << 23)).astype(np.uint32).view(F32)


# ---- check, within, check_t ------------------------------------------------------------------------------------------------------------
WANT = np.array([[1.0, -2.0, 0.5], [0.0, 3.0, -1e-3]])
BOUND = np.full(WANT.shape, 1e-6)


@pytest.mark.parametrize("bad", (np.nan, np.inf, -np.inf))
def test_check_fails_a_non_finite_element_with_ratio_inf_at_its_index(bad):
    got = WANT.copy()
    got[1, 2] = bad
    for bound in (BOUND, np.full(WANT.shape, np.inf)):                   # no bound, however wide, admits it
        ok, ratio, idx, _, _ = MC.check(got, WANT, bound)
        assert not ok and ratio == np.inf and idx == (1, 2)
    with pytest.raises(AssertionError, match="the case's name"):
        MC.within("the case's name", got, WANT, BOUND)


def test_check_zero_bound_passes_only_on_equality():
    assert MC.check(WANT, WANT, 0.0)[:2] == (True, 0.0)
    got = WANT.copy()
    got[0, 1] = np.nextafter(got[0, 1], 0.0)
    ok, ratio, idx, err, bound = MC.check(got, WANT, np.zeros(WANT.shape))
    assert not ok and ratio == np.inf and idx == (0, 1) and err > 0 and bound == 0.0


def test_check_one_ulp_either_side_of_the_bound():
    want, bound = np.zeros(2), np.array([2.0 ** -20, 3e-7])              # want 0: the error is the element itself, exactly
    for i in (0, 1):
        for sign in (1.0, -1.0):
            at, above, below = (want.copy() for _ in range(3))
            at[i] = sign * bound[i]
            above[i] = sign * np.nextafter(bound[i], np.inf)
            below[i] = sign * np.nextafter(bound[i], 0.0)
            assert abs(above[i] - want[i]) > bound[i] > abs(below[i] - want[i])
            assert MC.check(at, want, bound)[:3] == (True, 1.0, (i,))
            ok, ratio, idx, _, _ = MC.check(above, want, bound)
            assert not ok and ratio > 1.0 and idx == (i,)
            ok, ratio, idx, _, _ = MC.check(below, want, bound)
            assert ok and ratio < 1.0 and idx == (i,)
            assert MC.within("below", below, want, bound) == ratio
            with pytest.raises(AssertionError, match="above: worst element"):
                MC.within("above", above, want, bound)


def test_check_shape_mismatch_empty_and_scalar_bound():
    assert MC.check(WANT.reshape(-1), WANT, BOUND)[:2] == (False, np.inf)
    assert MC.check(WANT[:1], WANT, BOUND)[0] is False
    assert MC.check(np.zeros((0, 3)), np.zeros((0, 3)), 1.0) == (True, 0.0, (), 0.0, 0.0)
    got = WANT + np.array([[0.0, 0.0, 0.0], [0.0, 0.25, 0.0]])
    assert MC.check(got, WANT, 0.5)[:3] == (True, 0.5, (1, 1)) and MC.check(got, WANT, 0.125)[:3] == (False, 2.0, (1, 1))
    assert MC.check(got, WANT, np.array([1.0, 0.125, 1.0]))[0] is False   # a row of bounds broadcasts over the rows
    assert MC.describe("x", MC.check(got, WANT, 0.5)) == "x: worst element (1, 1): |err| 2.500000e-01, bound 5.000000e-01, err / bound 0.5000"


def test_check_t_agrees_with_check():
    want = _hashed(600, 3).astype(F64).reshape(20, 30)
    bound = np.abs(want) * 2.0 ** -20
    bound[4, 5] = 0.0
    cases = {"equal": want.copy(), "inside": want + 0.75 * bound, "outside": want.copy(), "nan": want.copy(), "inf": want.copy(), "zero bound": want.copy()}
    cases["outside"][7, 7] += 3.0 * bound[7, 7]
    cases["nan"][0, 0] = np.nan
    cases["inf"][19, 29] = -np.inf
    cases["zero bound"][4, 5] = np.nextafter(want[4, 5], np.inf)
    for name, got in cases.items():
        ok, ratio = MC.check(got, want, bound)[:2]
        ok_t, ratio_t, nbad = MC.check_t(torch.from_numpy(got), torch.from_numpy(want), torch.from_numpy(bound))
        same = ratio_t == (sys.float_info.max if name == "zero bound" else ratio)      # nan_to_num's word for an inf that is no NaN
        assert ok == ok_t == (nbad == 0) == (name in ("equal", "inside")) and same, (name, ok, ratio, ok_t, ratio_t, nbad)


# ---- Guarded ---------------------------------------------------------------------------------------------------------------------------
GUARDED = [(2, None), (4, None), (8, None), (8, 0xDEADBEEFCAFEF00D), (2, 0x3C00), (1, 0xA5)]


@pytest.mark.parametrize("itemsize,pattern", GUARDED)
def test_guarded_reports_an_overwritten_guard_and_an_unwritten_element(itemsize, pattern):
    n = 37
    fresh = MC.Guarded(n, itemsize, pattern=pattern, device="cpu")
    assert fresh.ptr % 16 == 0 and fresh.ptr == fresh.buf.data_ptr() + itemsize * MC.GUARD and fresh.buf.numel() == n + 2 * MC.GUARD
    assert fresh.untouched("fresh") and fresh.raw("fresh").shape == (n,) and fresh.raw("fresh").dtype == np.dtype(f"u{itemsize}")
    want = np.dtype(f"u{itemsize}").type(MC._NAN[itemsize] if pattern is None else pattern)
    assert (fresh.raw("fresh") == want).all() and (fresh.buf.numpy().view(f"u{itemsize}") == want).all()
    for at in (n, -1, n + MC.GUARD - 1, -MC.GUARD):                      # the guard elements next to the payload and the outermost ones
        g = MC.Guarded(n, itemsize, pattern=pattern, device="cpu")
        g.buf[MC.GUARD:][at] = 0                                         # payload index `at`: a plain write inside the test's own tensor
        with pytest.raises(AssertionError, match="the buffer's name: guard elements overwritten"):
            g.raw("the buffer's name")
    g = MC.Guarded(n, itemsize, pattern=pattern, device="cpu")
    g.buf[MC.GUARD:MC.GUARD + n] = 0
    assert (g.raw("written") == 0).all() and not g.untouched("written")
    g.buf[MC.GUARD + 5] = fresh.buf[0]                                   # one element never written keeps the pattern
    assert not g.untouched("one left")
    if pattern is None:                                                  # ... which is a NaN, and fails `check` there
        got = {2: lambda: g.T("one left", "f16")[0], 4: lambda: g.f32("one left"), 8: lambda: g.f64("one left")}[itemsize]()
        assert np.isnan(got[5]) and np.isfinite(np.delete(got, 5)).all()
        assert MC.check(got, np.zeros(n), np.inf)[:3] == (False, np.inf, (5,))
        if itemsize == 2:
            assert np.isnan(g.T("one left", "bf16")[0][5])


def test_guarded_init_shift_and_views():
    vals = _hashed(9, 1)
    g = MC.Guarded(9, init=vals, device="cpu")
    MC.same_bits("init", g.f32("init"), vals)
    with pytest.raises(AssertionError, match="guard"):
        g.buf[MC.GUARD - 1] = 0
        g.raw("init")
    g = MC.Guarded(6, init=np.arange(3, dtype=F64), device="cpu")         # 4-byte words read as doubles (the BatchNorm statistics)
    assert np.array_equal(g.f64("f64"), np.arange(3.0))
    for itemsize in (2, 4):
        s = MC.Guarded(5, itemsize, device="cpu", shift=1)
        assert s.ptr % 16 == itemsize and s.untouched("shifted")
        s.buf[MC.GUARD] = 0                                              # the skipped element counts as guard
        with pytest.raises(AssertionError, match="shifted: guard"):
            s.raw("shifted")
    with pytest.raises(KeyError):
        MC.Guarded(4, 1, device="cpu")                                   # one byte has no NaN: a pattern is required


# ---- the 16-bit conversions --------------------------------------------------------------------------------------------------------------
def _ties(dt):
    """fp32 values exactly halfway between two neighbours of T, below an even and below an odd one, of both signs."""
    keep = 10 if dt == "f16" else 7                                      # explicit mantissa bits of T
    m = np.arange(0, 64, dtype=np.uint32)                                # the low mantissa bits of T: even and odd
    half = np.uint32(1 << (23 - keep - 1))
    out = []
    for e in (113, 120, 127, 130, 141):                                  # fp32 exponents that are normal in f16 as well
        bits = (np.uint32(e) << np.uint32(23)) | (m << np.uint32(23 - keep)) | half
        out += [bits, bits | np.uint32(0x80000000)]
    return np.concatenate(out).view(F32)


@pytest.mark.parametrize("dt", MC.DTYPES)
def test_to_bits_from_bits_round_T_are_torchs_conversions(dt):
    tdt = torch.float16 if dt == "f16" else torch.bfloat16
    ties = _ties(dt)
    v = np.concatenate([_hashed(4000, 7), ties, np.array([0.0, -0.0, 1.0, -1.0, 65504.0, 2.0 ** -14, 2.0 ** -24, 3 * 2.0 ** -25], F32)])
    t = torch.from_numpy(v).to(tdt)
    assert torch.isfinite(t).all()
    bits = MC.to_bits(v, dt)
    MC.same_bits(f"to_bits {dt}", bits, t.view(torch.int16).numpy())
    MC.same_bits(f"from_bits {dt}", MC.from_bits(bits, dt), t.float().numpy())
    MC.same_bits(f"round_T {dt}", MC.round_T(v.reshape(2, -1), dt), t.float().numpy().reshape(2, -1))
    MC.same_bits(f"round trip {dt}", MC.to_bits(MC.from_bits(bits, dt), dt), bits)
    r = MC.round_T(ties, dt).astype(F64)                                 # the ties went both ways: to the even neighbour each time
    assert (r > ties).any() and (r < ties).any() and (MC.to_bits(ties, dt) & 1 == 0).all()
    assert (MC.to_bits(np.array([MC.NAN32], np.uint32).view(F32), "f16") & 0x7C00 == 0x7C00).all()
    assert np.isnan(MC.from_bits(np.array([MC.NAN16], np.uint16), dt)).all()


# ---- same_bits ------------------------------------------------------------------------------------------------------------------------
def test_same_bits_is_equality_of_patterns():
    a = np.array([[0.0, 1.0, np.nan], [-np.inf, 2.5, -0.0]], F32)
    MC.same_bits("itself", a, a.copy())
    MC.same_bits("flat against shaped", a.reshape(-1), a)
    b = a.copy()
    b[0, 0] = -0.0
    with pytest.raises(AssertionError, match=r"zeros: 1 elements differ, the first at \(0, 0\): 0x80000000, expected 0x0"):
        MC.same_bits("zeros", b, a)
    c = a.copy()
    c.view(np.uint32)[0, 2] ^= 1                                         # another NaN
    with pytest.raises(AssertionError, match=r"the first at \(0, 2\)"):
        MC.same_bits("nans", c, a)
    MC.same_bits("masked", c, a, mask=~np.isnan(a))
    with pytest.raises(AssertionError, match="masked"):
        MC.same_bits("masked", b, a, mask=~np.isnan(a))
    with pytest.raises(AssertionError, match="shape"):
        MC.same_bits("shape", a.T, a)
    with pytest.raises(AssertionError, match="size"):
        MC.same_bits("size", a.reshape(-1)[:5], a)
    with pytest.raises(AssertionError, match="width"):
        MC.same_bits("width", a.astype(F64), a)
    MC.same_bits("integers", np.array([1, 0xFFFF], np.uint16), np.array([1, -1], np.int16))


# ---- refused, Worst --------------------------------------------------------------------------------------------------------------------
class _Lib:
    """A library whose one entry refuses n <= 0 the way `how` says."""

    def __init__(self, how):
        self.how, self.launches, self.msg = how, 0, b""

    def entry(self, a):
        if a["n"] > 0:
            self.launches += 1
            return 0
        self.msg = {"right": b"entry: n > 0", "other text": b"entry: bad args", "no text": b""}.get(self.how, b"entry: n > 0")
        self.launches += self.how == "launches"
        return 0 if self.how == "returns 0" else MC.EINVAL

    def idb_last_error(self):
        return self.msg

    def idb_launch_count(self):
        return self.launches


@pytest.mark.parametrize("how", ("right", "returns 0", "other text", "no text", "launches"))
def test_refused_rejects_every_way_a_check_can_be_missing(how):
    lib = _Lib(how)
    args = (lib, lib.entry, dict(n=3, p=MC.P16), [dict(n=0), dict(n=-1)], "n > 0")
    if how == "right":
        MC.refused(*args)
    else:
        with pytest.raises(AssertionError):
            MC.refused(*args)
    if how == "no text":
        with pytest.raises(AssertionError):
            MC.refused(lib, lib.entry, dict(n=3), [dict(n=0)], "")       # an empty message fails even when no text is asked for
    with pytest.raises(AssertionError):
        MC.refused(_Lib("right"), lib.entry, dict(n=3), [dict(m=0)], "n > 0")      # a variant of an argument the entry does not have
    assert MC.OFF % 16 == 4 and MC.P16 % 16 == 0


def test_worst_keeps_the_worst_and_prints_the_summary_lines():
    w = MC.Worst("x matrix", launches=True)
    w.note("k", 0.25, "case a", 2)
    w.note("k", 0.75, "case b", 2)
    w.note("k", 0.5, "case c", 2)
    w.note("a [ulp]", 1.5, "case a")
    assert list(w.lines()) == ["x matrix: a [ulp]: 0 launches, worst err / bound 1.5000 (case a)", "x matrix: k: 6 launches, worst err / bound 0.7500 (case b)"]
    w = MC.Worst("y matrix, emulation")
    w.judge("k", "case", [1.0, 2.0], [1.0, 2.5], 1.0)
    w.note("k", 0.125)
    assert list(w.lines()) == ["y matrix, emulation: k: worst err / bound 0.5000 (case)"]
    with pytest.raises(AssertionError, match="case: worst element"):
        w.judge("k", "case", [1.0, np.nan], [1.0, 2.5], 1.0)
