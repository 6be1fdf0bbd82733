"""The harness every per-element float64 test matrix shares (detect_, pair_, stem_, prep_, block_matrix.py and their test files; the
torch verdict of attn_ and norm_matrix.py): the constants, the fp32 / f16 / bf16 numerics, the element-wise verdicts, the guarded
device buffer, the worst-ratio recorder and the argument-check contract.  A case file keeps what is its family's: cases, recipes,
float64 references, emulations, defects and bound formulas.  tests/test_matrix_common_cpu.py tests this file itself.

Criteria.  u = 2^-24, gamma_n = n u / (1 - n u) (forward bound of n fp32 roundings on one term of a sum), u_T = 2^-11 (f16) or 2^-8
(bf16), sub_T = 2^-25 for f16 (below 2^-14 f16 is spaced 2^-24, so u_T |ref| is not the half-spacing there), 0 for bf16."""
import math
from typing import Tuple

import numpy as np
import torch

from faceposegenerator_amd import _lib as L

U = 2.0 ** -24
F32 = np.float32
F64 = np.float64
DTYPES = ("f16", "bf16")
U_T = {"f16": 2.0 ** -11, "bf16": 2.0 ** -8}
SUB_T = {"f16": 2.0 ** -25, "bf16": 0.0}
GUARD = 64                            # guard elements on each side of every guarded buffer
NAN32 = 0x7FC0DE7C                    # the 4-byte guards' and pre-fill's pattern: a quiet fp32 NaN with a payload, a large positive int32
NAN16 = 0x7FDE                        # 16 bits that are a NaN with a payload both as f16 and as bf16
NAN64 = 0x7FF8C0DE7C0DE7C0            # the 8-byte pattern: a quiet float64 NaN
DEV = "cuda:0"
IDB = {"f16": L.IDB_F16, "bf16": L.IDB_BF16}


# ---- numerics -----------------------------------------------------------------------------------------------------------------------
def gamma(n: int) -> float:
    return n * U / (1.0 - n * U)


def ulp32(v) -> np.ndarray:
    """fp32 spacing at |v| (v float64): 2^-149 below the normal range and at 0."""
    return np.spacing(np.abs(np.asarray(v, F64)).astype(F32)).astype(F64)


def bf16_bits(v) -> np.ndarray:
    """fp32 -> the 16 bits of the nearest bf16, ties to even, by bit arithmetic (finite inputs)."""
    b = np.ascontiguousarray(v, F32).view(np.uint32).astype(np.uint64)
    return ((b + np.uint64(0x7FFF) + ((b >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)).astype(np.uint16)


def to_bits(v, dt: str) -> np.ndarray:
    """fp32 -> uint16 bit patterns of T (round to nearest even)."""
    return np.ascontiguousarray(v, F32).astype(np.float16).view(np.uint16) if dt == "f16" else bf16_bits(v)


def from_bits(bits, dt: str) -> np.ndarray:
    """uint16 bit patterns of T -> fp32 (exact)."""
    bits = np.ascontiguousarray(bits, np.uint16)
    if dt == "f16":
        return bits.view(np.float16).astype(F32)
    return (bits.astype(np.uint32) << np.uint32(16)).view(F32)


def round_T(v, dt: str) -> np.ndarray:
    """fp32 -> fp32 holding the nearest value of T."""
    v = np.asarray(v, F32)
    return from_bits(to_bits(v, dt), dt).reshape(v.shape)


def fma32(a, b, c) -> np.ndarray:
    """fl32(a b + c) of fp32 arrays with one rounding: the exact product of two fp32 values fits a float64; the float64 sum is rounded
    to odd with the TwoSum residue, and 53 >= 2 * 24 + 2 bits make the final rounding to fp32 the rounding of the exact value."""
    a, b, c = (np.asarray(v, F32).astype(F64) for v in (a, b, c))
    p = a * b                                             # exact: 48 bits
    s = np.atleast_1d(p + c)
    p, c = np.broadcast_to(p, s.shape), np.broadcast_to(c, s.shape)
    bb = s - p
    res = (p - (s - bb)) + (c - bb)                       # TwoSum: p + c = s + res exactly
    odd = (np.ascontiguousarray(s).view(np.int64) & 1) == 1
    s = np.where((res != 0) & ~odd, np.nextafter(s, np.where(res > 0, np.inf, -np.inf)), s)      # round to odd
    return s.astype(F32)


# ---- verdicts -----------------------------------------------------------------------------------------------------------------------
def check(got, want, bound) -> Tuple[bool, float, Tuple[int, ...], float, float]:
    """(every element finite and within its bound, worst err / bound, its index, its error, its bound); a zero bound demands equality."""
    got, want = np.asarray(got, F64), np.asarray(want, F64)
    bound = np.broadcast_to(np.asarray(bound, F64), want.shape)
    if got.shape != want.shape:
        return False, np.inf, (), np.inf, 0.0
    if got.size == 0:
        return True, 0.0, (), 0.0, 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.abs(got - want)
        ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    ratio = np.where(np.isfinite(got) & np.isfinite(err), ratio, np.inf)
    i = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    ok = bool(np.all(np.isfinite(got)) and np.all(err <= bound))
    return ok, float(ratio[i]), tuple(int(v) for v in i), float(err[i]), float(bound[i])


def describe(name, res) -> str:
    ok, ratio, idx, err, bound = res
    return f"{name}: worst element {idx}: |err| {err:.6e}, bound {bound:.6e}, err / bound {ratio:.4f}"


def within(what: str, got, want, bound, show=False) -> float:
    """AssertionError naming the worst element unless `check` passes; returns worst err / bound.  `show` prints the verdict first."""
    res = check(got, want, bound)
    if show:
        print(describe(what, res))
    assert res[0], describe(what, res)
    return res[1]


def bit_equal(got, want) -> Tuple[bool, Tuple[int, ...]]:
    """fp32 arrays equal bit for bit (so -inf equals -inf and a NaN pattern only itself); the first differing index."""
    got, want = np.ascontiguousarray(got, F32), np.ascontiguousarray(want, F32)
    if got.shape != want.shape:
        return False, ()
    d = got.view(np.uint32) != want.view(np.uint32)
    return not d.any(), tuple(int(v) for v in np.argwhere(d)[0]) if d.any() else ()


def same_bits(what: str, got, want, mask=None):
    """AssertionError naming the first differing element and both patterns unless the two arrays, of one element width, are equal bit
    for bit (-0.0 is not 0.0, a NaN pattern equals only itself).  The shapes are equal, or one side is flat and of the same size; `mask`
    selects the elements that count."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype.itemsize == want.dtype.itemsize, f"{what}: {got.dtype} against {want.dtype}"
    assert got.shape == want.shape or (min(got.ndim, want.ndim) == 1 and got.size == want.size), f"{what}: {got.shape} against {want.shape}"
    shape = want.shape if got.ndim == 1 else got.shape
    bits = np.dtype(f"u{got.dtype.itemsize}")
    got, want = got.reshape(-1).view(bits), want.reshape(-1).view(bits)
    diff = np.flatnonzero((got != want) if mask is None else ((got != want) & np.asarray(mask).reshape(-1)))
    if diff.size:
        at = tuple(int(v) for v in np.unravel_index(diff[0], shape))
        raise AssertionError(f"{what}: {diff.size} elements differ, the first at {at}: {int(got[diff[0]]):#x}, expected {int(want[diff[0]]):#x}")


def check_t(out: torch.Tensor, want: torch.Tensor, bnd: torch.Tensor) -> Tuple[bool, float, int]:
    """The torch verdict: (every element finite and within its bound, worst err / bound, number of failing elements).  An element whose
    bound is 0 must be exact (its ratio is the largest double otherwise, inf for an element that is not finite); none is skipped."""
    out = out.double()
    err = (out - want).abs()
    bad = ~torch.isfinite(out) | ~(err <= bnd)
    ratio = torch.where(bnd > 0, err / bnd.clamp(min=1e-300), torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    ratio = torch.where(torch.isfinite(out), torch.nan_to_num(ratio, nan=math.inf), torch.full_like(ratio, math.inf))
    return not bool(bad.any()), float(ratio.max()), int(bad.sum())


class Worst:
    """Per key, the worst err / bound with the case it occurred in and the launches; `lines` is what a test_summary prints."""

    def __init__(self, title, ratio="err / bound", launches=False):
        self.title, self.ratio, self.launches = title, ratio, launches
        self.worst, self.count = {}, {}

    def launched(self, key, launches):
        self.count[key] = self.count.get(key, 0) + launches

    def note(self, key, ratio, where=None, launches=0):
        self.launched(key, launches)
        if key not in self.worst or ratio > self.worst[key][0]:
            self.worst[key] = (ratio, where)

    def judge(self, key, what, got, want, bound, launches=0):
        """`within`, printed, and noted under `key`."""
        self.note(key, within(what, got, want, bound, show=True), what, launches)

    def show(self):
        print("".join(line + "\n" for line in self.lines()), end="")

    def lines(self):
        for k in sorted(self.worst):
            ratio, where = self.worst[k]
            yield (f"{self.title}: {k}: " + (f"{self.count[k]} launches, " if self.launches else "") + f"worst {self.ratio} {ratio:.4f}"
                   + ("" if where is None else f" ({where})"))


# ---- the device side ----------------------------------------------------------------------------------------------------------------
def stream(device=None):
    return torch.cuda.current_stream(device).cuda_stream


def dev(a, dtype=None):
    """A host array (cast to `dtype` if given) on the device, 16-bit patterns as int16; None stays None."""
    if a is None:
        return None
    a = np.ascontiguousarray(a, dtype)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(DEV)


def ptr(t):
    return None if t is None else t.data_ptr()


_TORCH_INT = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
_NP_INT = {1: np.uint8, 2: np.int16, 4: np.int32, 8: np.int64}
_NAN = {2: NAN16, 4: NAN32, 8: NAN64}


class Guarded:
    """n elements of 1, 2, 4 or 8 bytes between GUARD elements of a bit pattern: the NaN of that width, or `pattern` (1 byte has no NaN
    and needs one).  Pre-filled with the pattern, so that an element a kernel does not write fails its criterion, or with `init` (any
    array of n elements of that width).  An output buffer, an in-place buffer, or a workspace of exactly n elements.  `ptr` is
    16-byte aligned; `shift` moves it that many elements further, and the skipped elements count as guard."""

    def __init__(self, n, itemsize=4, init=None, pattern=None, device=DEV, shift=0):
        self.n, self.itemsize, self.lo = n, itemsize, GUARD + shift
        self.bits = np.dtype(f"u{itemsize}")
        self.pattern = self.bits.type(_NAN[itemsize] if pattern is None else pattern)
        fill = int(np.array(self.pattern, self.bits).view(_NP_INT[itemsize]))           # torch's integers are signed above one byte
        self.buf = torch.full((n + 2 * GUARD + shift,), fill, dtype=_TORCH_INT[itemsize], device=device)
        if init is not None:
            self.buf[self.lo:self.lo + n] = torch.from_numpy(np.ascontiguousarray(init).reshape(-1).view(_NP_INT[itemsize])).to(device)
        assert (self.buf.data_ptr() + itemsize * GUARD) % 16 == 0
        self.ptr = self.buf.data_ptr() + itemsize * self.lo

    def raw(self, what):
        """The payload's bit patterns (unsigned), after asserting that both guards are intact."""
        host = self.buf.cpu().numpy().view(self.bits)
        assert (host[:self.lo] == self.pattern).all() and (host[self.lo + self.n:] == self.pattern).all(), f"{what}: guard elements overwritten"
        return host[self.lo:self.lo + self.n]

    def f32(self, what):
        return self.raw(what).view(F32)

    def f64(self, what):
        return self.raw(what).view(F64)

    def T(self, what, dt):
        """(fp32 values, 16-bit patterns) of a buffer of f16 or bf16 elements."""
        bits = self.raw(what)
        return from_bits(bits, dt), bits

    def untouched(self, what):
        return bool((self.raw(what) == self.pattern).all())


# ---- argument checks: an IDB_REQUIRE answers before any HIP call --------------------------------------------------------------------
EINVAL = -1
P16 = 1 << 20            # any non-null 16-byte-aligned address: none of these calls dereferences it
OFF = P16 + 4            # 4-byte aligned only
BAD_DTYPES = [dict(dtype=d) for d in (-1, 99, max(IDB.values()) + 1) if d not in IDB.values()]


def refused(lib, call, ok, variants, text):
    """Every variant of the accepted argument set `ok` (call takes the merged dict) answers IDB_EINVAL with `text` in a non-empty
    idb_last_error(), and launches nothing."""
    before = lib.idb_launch_count()
    for kw in variants:
        assert set(kw) <= set(ok), kw
        rc = call({**ok, **kw})
        msg = lib.idb_last_error()
        assert rc == EINVAL and msg and text.encode() in msg, (kw, rc, msg)
    assert lib.idb_launch_count() == before
