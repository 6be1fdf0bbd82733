"""Every case x input recipe of the norm test matrix (tests/norm_matrix.py) on the device, both dtypes, against float64 references computed
on the device from the same operand-dtype-rounded inputs, element by element.

The C ABI is called directly.  Every GroupNorm launch: the output lies between guard rows of a canary bit pattern (a NaN in both dtypes,
0x7F for e4m3) that are checked afterwards; the workspace is exactly idb_groupnorm_workspace_bytes and is filled with NaN before the call (a
partial that is loaded from a clamped index and not masked out then shows); idb_groupnorm_plan must report the geometry the case was
chosen for.  Per case and recipe: idb_groupnorm_stats alone (*chunks equals the query's, every partial against the float64 sum of its
chunk: bit-exact for the recipes with exact sums, within d 2^-24 sum |addend| otherwise); the two-launch form; the single-launch form
wherever the query says the library would take it with the engine's 4096 counters (ONE counter array for all of them, asserted zero after
every call, the result also compared with the two-launch one under twice the statistics terms); the apply-only form where hw % 64 == 0
and hw / 64 <= 64, fed (a) float64 sums rounded to fp32 and (b), where the two-launch geometry has 64-pixel chunks, what
idb_groupnorm_stats produced; idb_groupnorm_fp8 on the cases marked for it, with own statistics and with partials_in, out_inv_scale 200
(values saturate at +-448 and land in e4m3 subnormals).  LayerNorm and the in-place row softmax (its buffer between guard rows too) run
every (rows, C) / (rows, cols) x recipe.  Also: relaunch bit-equality, and one torch.cuda.graph capture + replay of a two-launch, an
apply-only and an fp8 call, bit-equal to the eager result.  test_partials_from_the_gemm feeds the apply-only form what idb_gemm's
gn_partials produced (split-K reduce, the GEMM's epilogue, and the extra statistics launch with its forced 64-pixel chunks);
test_single_launch_with_exactly_enough_counters launches the hand-off form with 2 * batch * slices counters between guard words.
Every recipe runs on every case, the >= 16 Mi-element ones included (float64 references on the device).

Worst err / criterion measured on MI355X, bf16 / f16 (test_summary prints one line per operation, dtype and recipe; recorded for the next
reader, not used as thresholds).  GroupNorm, two-launch: normal 0.996 / 0.995, offset 0.987 / 0.929, mixed_scale 0.995 / 0.991, constant_group
0.993 / 0.984, constant_offset 0.050 / 0.028, tiny_var 0.996 / 0.997, count 0.996 / 0.998, ramp 0.995 / 0.994, outlier 0.996 / 0.996; the
single-launch and apply-only forms are within 0.01 of these (the worst cases are the 40-column twin_cpg40 / big_cpg40); statistics partials at
most 0.215 of d 2^-24 sum |addend| (big_cpg60, outlier) and bit-exact on count / constant_group; partials from idb_gemm at most 0.094 (statistics
launch) / 0.016 (its own kernels) of theirs and bit-exact on count; every fp8 byte inside its interval.  LayerNorm 0.986 .. 0.998 on every recipe.  Softmax: normal 0.995 / 1.000 (f16,
300x4096: 0.9996, the output rounding), peaked 0.992 / 0.000, constant_row 0.500 / 0.484, shifted 0.995 / 0.999.  No constant was changed
for the GPU.  4016 launched combinations over both dtypes; the whole file runs in about 8 s on one MI355X.

Conditioning of the one-pass variance (test_conditioning_envelope; worst |got - ref| / (u max(|ref|, 1)) at |mean| / std = R, gamma 1, beta 0):
    elements per group      bf16: R = 1    4     16    64    256        f16: R = 1    4     16    64    256
    64 x 40 = 2560                1.00  0.99  0.99  1.01  1.16              1.00  0.99  1.00  1.51  8.48
    4096 x 10 = 40960             1.00  1.00  1.00  0.95  1.16              1.00  1.00  1.03  1.89  17.3
    262144 x 4 = 1048576          1.00  1.00  0.80  0.82  1.51              1.00  1.00  1.05  2.57  37.1
(1.00 is the output rounding alone.)  The criterion's statistics lines exceed one output ulp (2 u) from R = 64 in bf16 (2.5 / 3.1 / 15 u at
the three lengths; 0.16 / 0.2 / 0.97 u at R = 16) and from R = 64 / 64 / 16 in f16 (1.3 / 1.6 / 7.7 u at R = 16)."""
import os
import sys
import time
from collections import defaultdict

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import matrix_common as MC  # noqa: E402
import norm_matrix as NM  # noqa: E402
from faceposegenerator_amd import _lib as L  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = ("bf16", "f16")
FP8_INV_SCALE = 200.0
G = NM.GUARD_ROWS

_WORST = defaultdict(lambda: [0, 0.0, ""])        # (op, dtype, recipe) -> [launches, worst ratio, where]
_SYNC = {}
_T0 = time.time()


def _sync_counters():
    if "c" not in _SYNC:
        _SYNC["c"] = torch.zeros(NM.SYNC_LEN, dtype=torch.int32, device=DEV)
    return _SYNC["c"]


def _note(op, dtype, recipe, ratio, where):
    s = _WORST[op, dtype, recipe]
    s[0] += 1
    if ratio > s[1]:
        s[1], s[2] = ratio, where


class _Gn:
    """The device buffers of one (case, recipe, dtype)."""

    def __init__(self, lib, case, recipe, dtype, inputs=None):
        self.lib, self.case, self.dtype = lib, case, dtype
        self.x, self.gamma64, self.beta64 = inputs or NM.gn_inputs(case, recipe, dtype, DEV)
        xt = self.x.to(NM.TDT[dtype])
        self.x0 = xt[..., :case.c0].contiguous()
        self.x1 = xt[..., case.c0:].contiguous() if case.c1 else None
        self.gamma, self.beta = self.gamma64.float().contiguous(), self.beta64.float().contiguous()
        self.ws_bytes = lib.idb_groupnorm_workspace_bytes(case.batch, case.hw, case.groups)
        assert self.ws_bytes == case.batch * 64 * case.groups * 8
        self.ws = torch.empty(self.ws_bytes // 4, dtype=torch.float32, device=DEV)

    def out_buffer(self, fp8=False):
        rows = self.case.batch * self.case.hw
        return torch.full((rows + 2 * G, self.case.c), NM.CANARY8 if fp8 else NM.CANARY, dtype=torch.uint8 if fp8 else torch.int16, device=DEV)

    def launch(self, obuf, sync=None, pin=None, fp8=False):
        c = self.case
        self.ws.fill_(float("nan"))
        optr = obuf.data_ptr() + G * c.c * obuf.element_size()
        x1 = self.x1.data_ptr() if c.c1 else None
        pch = c.hw // 64 if pin is not None else 0
        if fp8:
            rc = self.lib.idb_groupnorm_fp8(self.x0.data_ptr(), c.c0, x1, c.c1, c.batch, c.hw, c.groups, c.eps, self.gamma.data_ptr(), self.beta.data_ptr(),
                                            int(c.silu), optr, FP8_INV_SCALE, NM.IDB_DT[self.dtype], self.ws.data_ptr(), self.ws_bytes,
                                            None if pin is None else pin.data_ptr(), pch, MC.stream())
        else:
            rc = self.lib.idb_groupnorm(self.x0.data_ptr(), c.c0, x1, c.c1, c.batch, c.hw, c.groups, c.eps, self.gamma.data_ptr(), self.beta.data_ptr(),
                                        int(c.silu), optr, NM.IDB_DT[self.dtype], self.ws.data_ptr(), self.ws_bytes,
                                        None if sync is None else sync.data_ptr(), 0 if sync is None else sync.numel(),
                                        None if pin is None else pin.data_ptr(), pch, MC.stream())
        L.check(rc, f"groupnorm {c.name}")

    def run(self, sync=None, pin=None, fp8=False):
        obuf = self.out_buffer(fp8)
        self.launch(obuf, sync, pin, fp8)
        torch.cuda.synchronize()
        return self.result(obuf, fp8)

    def result(self, obuf, fp8=False):
        c = self.case
        canary = NM.CANARY8 if fp8 else NM.CANARY
        assert bool((obuf[:G] == canary).all()) and bool((obuf[-G:] == canary).all()), f"{c.name} {self.dtype}: a guard row lost its canary"
        body = obuf[G:-G]
        return (body.view(NM.F8) if fp8 else body.view(NM.TDT[self.dtype])).view(c.batch, c.hw, c.c)

    def stats(self):
        import ctypes as C
        c = self.case
        part = torch.full((self.ws_bytes // 4,), float("nan"), dtype=torch.float32, device=DEV)
        chunks = C.c_int32(-1)
        L.check(self.lib.idb_groupnorm_stats(self.x0.data_ptr(), c.c0, self.x1.data_ptr() if c.c1 else None, c.c1, c.batch, c.hw, c.groups, part.data_ptr(),
                                             self.ws_bytes, C.byref(chunks), NM.IDB_DT[self.dtype], MC.stream()), f"groupnorm_stats {c.name}")
        torch.cuda.synchronize()
        return part, chunks.value


def _plans(lib, c):
    two = NM.plan(lib, c.c0, c.c1, c.batch, c.hw, c.groups)[1]
    single = NM.plan(lib, c.c0, c.c1, c.batch, c.hw, c.groups, NM.SYNC_LEN)[1]
    pin = NM.plan(lib, c.c0, c.c1, c.batch, c.hw, c.groups, 0, c.hw // 64)[1] if c.pin_ok else None
    assert (two.form, two.sw, two.chunks) == (0, c.sw, c.chunks), f"{c.name}: the plan no longer reports the geometry the case was chosen for: {two}"
    assert (single.form == 1) == c.single, f"{c.name}: single-launch eligibility changed"
    assert pin is None or pin.form == 2
    return two, single, pin


@pytest.mark.parametrize("dtype", DTYPES)
def test_groupnorm_matrix(lib, dtype):
    failures = []
    sync = _sync_counters()
    pin_stat = set()

    def judge(case, recipe, label, out, r, p, **kw):
        ok, ratio, nbad = NM.check(out, r.ref, NM.gn_bound(r, p, dtype, recipe, **kw))
        print(f"{dtype} {case.name:22s} {recipe:15s} {label:8s} worst err/criterion {ratio:.3f} bad {nbad}")
        _note("groupnorm/" + label, dtype, recipe, ratio, case.name)
        if not ok:
            failures.append(f"{case.name}/{recipe}/{label}: {nbad} of {out.numel()} elements beyond the criterion or not finite, worst ratio {ratio:.3g}")

    for case in NM.gn_cases(lib):
        two, single, pin = _plans(lib, case)
        for recipe in case.recipes:
            gn = _Gn(lib, case, recipe, dtype)
            r = NM.gn_reference(gn.x, gn.gamma64, gn.beta64, case.groups, case.eps, case.silu)
            # the statistics alone
            part, chunks = gn.stats()
            assert chunks == two.chunks, (case.name, chunks, two.chunks)
            got = part[:case.batch * chunks * case.groups * 2].view(case.batch, chunks, case.groups, 2)
            assert bool(torch.isnan(part[case.batch * chunks * case.groups * 2:]).all()), f"{case.name} {recipe}: a write beyond the {chunks} chunks reported"
            want, mag = NM.gn_partial_sums(gn.x, two, case.groups)
            if recipe in NM.EXACT_SUMS:
                if not torch.equal(got.double(), want):
                    failures.append(f"{case.name}/{recipe}/stats: {int((got.double() != want).sum())} partial sums are not the exact integers")
            else:
                ok, ratio, nbad = NM.check(got, want, NM.gn_depth(two) * NM.E24 * mag)
                _note("groupnorm/stats", dtype, recipe, ratio, case.name)
                if not ok:
                    failures.append(f"{case.name}/{recipe}/stats: {nbad} partials beyond d 2^-24 sum|addend|, worst ratio {ratio:.3g}")
            out_two = gn.run()
            judge(case, recipe, "two", out_two, r, two)
            if single.form == 1:
                out_s = gn.run(sync=sync)
                assert int(sync.abs().sum().item()) == 0, f"{case.name} {recipe}: the hand-off counters are not zero after the call"
                judge(case, recipe, "single", out_s, r, single)
                lim = NM.gn_bound(r, single, dtype, recipe, stat_factor=2.0) + NM.UNIT[dtype] * r.ref.abs()
                if not bool(((out_s.double() - out_two.double()).abs() <= lim).all()):
                    failures.append(f"{case.name}/{recipe}: single-launch and two-launch results differ beyond twice the statistics terms")
            if pin is not None:
                want64, _ = NM.gn_partial_sums(gn.x, pin, case.groups)
                judge(case, recipe, "pin_f64", gn.run(pin=want64.float().contiguous()), r, pin)
                if (two.chunks, two.chunk_len) == (pin.chunks, 64):
                    pin_stat.add(case.name)
                    judge(case, recipe, "pin_stat", gn.run(pin=part), r, pin)
            if case.fp8:
                lo, hi = NM.fp8_interval(r, two, dtype, recipe, FP8_INV_SCALE)
                for label, kw in (("fp8", {}),) + ((("fp8_pin", dict(pin=NM.gn_partial_sums(gn.x, pin, case.groups)[0].float().contiguous())),) if pin is not None else ()):
                    o8 = gn.run(fp8=True, **kw).double()
                    bad = int((~torch.isfinite(o8) | (o8 < lo) | (o8 > hi)).sum())
                    _note("groupnorm/" + label, dtype, recipe, float(bad), case.name)
                    if bad:
                        failures.append(f"{case.name}/{recipe}/{label}: {bad} bytes are not the e4m3 rounding of a value inside the criterion's interval")
                    if recipe == "normal":
                        assert bool((o8.abs() == 448).any()) and bool(((o8 != 0) & (o8.abs() < 2.0 ** -6)).any()), f"{case.name}: no saturated / subnormal e4m3 value"
            del gn, r
    assert pin_stat == set(NM.PIN_STAT_CASES), f"the cases whose idb_groupnorm_stats output serves as partials_in changed: {sorted(pin_stat)}"
    assert not failures, f"{dtype}:\n" + "\n".join(failures)


@pytest.mark.parametrize("dtype", DTYPES)
def test_partials_from_the_gemm(lib, dtype):
    """idb_gemm_desc.gn_partials: an identity 1x1 GEMM reproduces its input exactly, so its output is the recipe's tensor and the partials it
    emits (from the split-K reduce launch, from the GEMM's own epilogue, or from the extra statistics launch idb_launch_gn_stats64, which forces
    hw / 64 chunks of 64 pixels onto the slice geometry: idb_gemm_emits_gn_partials says which) are judged like idb_groupnorm_stats': bit-exact
    on `count`, else within d 2^-24 sum |addend| per partial (d from the 64-pixel-chunk geometry for the statistics launch; for the GEMM's own
    kernels, whose order is theirs, the worst any order allows: one addition per addend of the chunk, 64 * cpg), and then fed to the apply-only
    form under its criterion.  Shapes where hw / 64 differs from the two-launch chunks (norm_matrix.GEMM_PIN)."""
    import ctypes as C
    from faceposegenerator_amd import spec as S
    from faceposegenerator_amd.engine import HipEngine
    eng = HipEngine(S.TINY_UNET, S.TINY_VAE, None, None, DEV, dtype)
    failures, modes = [], defaultdict(int)
    for c, batch, side in NM.GEMM_PIN:
        case = NM.gemm_pin_case(lib, c, batch, side)
        two = NM.plan(lib, c, 0, batch, case.hw, 32)[1]
        pin = NM.plan(lib, c, 0, batch, case.hw, 32, 0, case.hw // 64)[1]
        assert (two.chunks, two.chunk_len) != (pin.chunks, 64) and pin.form == 2, (case.name, two)
        w = torch.eye(c, device=DEV).to(NM.TDT[dtype])
        for recipe in case.recipes:
            gn = _Gn(lib, case, recipe, dtype)
            r = NM.gn_reference(gn.x, gn.gamma64, gn.beta64, 32, case.eps, case.silu)
            want, mag = NM.gn_partial_sums(gn.x, pin, 32)
            for split_k in (1, 2):
                eng.arena.reset()
                prev, eng.launch_log = eng.launch_log, []
                y = eng.gemm([(gn.x0.view(batch * case.hw, c), c, 1, side, side, 0)], w, c, batch, side, side, split_k=split_k, gn_stats=32, gn_stats_always=True)
                desc, eng.launch_log = eng.launch_log[-1]["desc"], prev
                torch.cuda.synchronize()
                assert getattr(y, "_gn", None) is not None and y._gn[1] == case.hw // 64, case.name
                assert torch.equal(y.view(torch.int16), gn.x0.view(batch * case.hw, c).view(torch.int16)), f"{case.name}: the identity GEMM changed its input"
                mode = eng.lib.idb_gemm_emits_gn_partials(C.byref(desc), 32)
                modes[mode] += 1
                label = f"gemm{mode}"
                got = y._gn[0].view(batch, case.hw // 64, 32, 2)
                if recipe in NM.EXACT_SUMS:
                    if not torch.equal(got.double(), want):
                        failures.append(f"{case.name}/{recipe}/{label}: {int((got.double() != want).sum())} partial sums are not the exact integers")
                else:
                    d = NM.gn_depth(pin) if mode == 0 else 64 * case.cpg
                    ok, ratio, nbad = NM.check(got, want, d * NM.E24 * mag)
                    _note("groupnorm/stats_" + label, dtype, recipe, ratio, case.name)
                    if not ok:
                        failures.append(f"{case.name}/{recipe}/{label}: {nbad} partials beyond d 2^-24 sum|addend|, worst ratio {ratio:.3g}")
                out = gn.run(pin=got.contiguous())
                ok, ratio, nbad = NM.check(out, r.ref, NM.gn_bound(r, pin, dtype, recipe))
                _note("groupnorm/pin_" + label, dtype, recipe, ratio, case.name)
                if not ok:
                    failures.append(f"{case.name}/{recipe}/pin_{label}: {nbad} elements beyond the criterion, worst ratio {ratio:.3g}")
    print(f"{dtype}: partials came from the statistics launch {modes[0]}x, the split-K reduce {modes[1]}x, the GEMM epilogue {modes[2]}x")
    assert modes[0] >= 3 and modes[1] + modes[2] >= 1, dict(modes)
    assert not failures, f"{dtype}:\n" + "\n".join(failures)


@pytest.mark.parametrize("dtype", DTYPES)
def test_single_launch_with_exactly_enough_counters(lib, dtype):
    """The sync_len limit on the device: a counter array of exactly 2 * batch * slices ints between guard words takes the single-launch form
    (one fewer does not, by the query), leaves its counters zero and the guards untouched, and computes what the two-launch form computes."""
    case = {c.name: c for c in NM.gn_cases(lib)}["u640p320_hw1024"]
    two = NM.plan(lib, case.c0, case.c1, case.batch, case.hw, case.groups)[1]
    n = 2 * case.batch * two.slices
    p = NM.plan(lib, case.c0, case.c1, case.batch, case.hw, case.groups, n)[1]
    assert p.form == 1 and NM.plan(lib, case.c0, case.c1, case.batch, case.hw, case.groups, n - 1)[1].form == 0
    guard = 0x5A5A5A5A
    buf = torch.full((n + 8,), guard, dtype=torch.int32, device=DEV)
    buf[4:4 + n] = 0
    gn = _Gn(lib, case, "normal", dtype)
    r = NM.gn_reference(gn.x, gn.gamma64, gn.beta64, case.groups, case.eps, case.silu)
    for _ in range(2):
        out = gn.run(sync=buf[4:4 + n])
        assert bool((buf[4:4 + n] == 0).all()) and bool((buf[:4] == guard).all()) and bool((buf[4 + n:] == guard).all())
        ok, ratio, nbad = NM.check(out, r.ref, NM.gn_bound(r, p, dtype, "normal"))
        assert ok, f"{nbad} elements beyond the criterion, worst ratio {ratio}"


@pytest.mark.parametrize("dtype", DTYPES)
def test_layernorm_matrix(lib, dtype):
    failures = []
    for c in NM.LN_C:
        for rows in NM.LN_ROWS:
            for recipe in NM.LN_RECIPES:
                x, gamma, beta = NM.ln_inputs(rows, c, recipe, dtype, DEV)
                ref, bnd = NM.ln_bound(x, gamma, beta, 1e-5, dtype, recipe)
                xt, g32, b32 = x.to(NM.TDT[dtype]), gamma.float(), beta.float()
                obuf = torch.full((rows + 2 * G, c), NM.CANARY, dtype=torch.int16, device=DEV)
                L.check(lib.idb_layernorm(xt.data_ptr(), obuf.data_ptr() + G * c * 2, rows, c, 1e-5, g32.data_ptr(), b32.data_ptr(), NM.IDB_DT[dtype], MC.stream()))
                torch.cuda.synchronize()
                assert bool((obuf[:G] == NM.CANARY).all()) and bool((obuf[-G:] == NM.CANARY).all()), f"layernorm {rows}x{c}: a guard row lost its canary"
                ok, ratio, nbad = NM.check(obuf[G:-G].view(NM.TDT[dtype]), ref, bnd)
                _note("layernorm", dtype, recipe, ratio, f"{rows}x{c}")
                if not ok:
                    failures.append(f"layernorm {rows}x{c} {recipe}: {nbad} elements beyond the criterion, worst ratio {ratio:.3g}")
    assert not failures, f"{dtype}:\n" + "\n".join(failures)


@pytest.mark.parametrize("dtype", DTYPES)
def test_softmax_matrix(lib, dtype):
    failures = []
    for cols in NM.SM_COLS:
        for rows in NM.SM_ROWS:
            for recipe in NM.SM_RECIPES:
                x = NM.sm_inputs(rows, cols, recipe, dtype, DEV)
                ref, bnd = NM.sm_bound(x, dtype)
                buf = torch.full((rows + 2 * G, cols), NM.CANARY, dtype=torch.int16, device=DEV)
                buf[G:-G] = x.to(NM.TDT[dtype]).view(torch.int16)
                L.check(lib.idb_softmax_rows(buf.data_ptr() + G * cols * 2, rows, cols, NM.IDB_DT[dtype], MC.stream()))
                torch.cuda.synchronize()
                assert bool((buf[:G] == NM.CANARY).all()) and bool((buf[-G:] == NM.CANARY).all()), f"softmax {rows}x{cols}: a guard row lost its canary"
                ok, ratio, nbad = NM.check(buf[G:-G].view(NM.TDT[dtype]), ref, bnd)
                _note("softmax", dtype, recipe, ratio, f"{rows}x{cols}")
                if not ok:
                    failures.append(f"softmax {rows}x{cols} {recipe}: {nbad} elements beyond the criterion, worst ratio {ratio:.3g}")
    assert not failures, f"{dtype}:\n" + "\n".join(failures)


@pytest.mark.parametrize("dtype", DTYPES)
def test_relaunch_is_bit_identical(lib, dtype):
    by_name = {c.name: c for c in NM.gn_cases(lib)}
    sync = _sync_counters()
    for name in ("u320p640_hw576", "cpg3_hw100", "big_cpg30", "v128_hw4096"):
        case = by_name[name]
        gn = _Gn(lib, case, "normal", dtype)
        for kw in ({}, dict(sync=sync)) if case.single else ({},):
            a, b = gn.run(**kw), gn.run(**kw)
            assert torch.equal(a.view(torch.int16), b.view(torch.int16)), f"{name} {dtype} {kw and 'single'}: two launches on the same inputs differ"
    assert int(sync.abs().sum().item()) == 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_graph_replay_equals_eager(lib, dtype):
    """A two-launch, an apply-only and an fp8 call captured on a single stream, replayed into canary-refilled buffers."""
    case = {c.name: c for c in NM.gn_cases(lib)}["v128_hw4096"]
    gn = _Gn(lib, case, "normal", dtype)
    pin = NM.gn_partial_sums(gn.x, NM.plan(lib, case.c0, 0, case.batch, case.hw, case.groups, 0, case.hw // 64)[1], case.groups)[0].float().contiguous()
    variants = (dict(), dict(pin=pin), dict(fp8=True))
    bufs = [gn.out_buffer(v.get("fp8", False)) for v in variants]
    eager = []
    for v, buf in zip(variants, bufs):
        gn.launch(buf, **v)
        torch.cuda.synchronize()
        eager.append(buf.clone())
        buf.fill_(NM.CANARY8 if v.get("fp8") else NM.CANARY)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for v, buf in zip(variants, bufs):
            gn.launch(buf, **v)
    for v, buf in zip(variants, bufs):
        buf.fill_(NM.CANARY8 if v.get("fp8") else NM.CANARY)
    graph.replay()
    torch.cuda.synchronize()
    for v, buf, e in zip(variants, bufs, eager):
        assert torch.equal(buf, e), f"{dtype} {v}: the replayed graph differs from the eager launch"
        assert bool((e[G:-G] != (NM.CANARY8 if v.get("fp8") else NM.CANARY)).all())


@pytest.mark.parametrize("dtype", DTYPES)
def test_conditioning_envelope(lib, dtype):
    """The offset recipe pins the algorithm inside test_groupnorm_matrix; this records the figures for include/idb_kernels.h."""
    print()
    for case in NM.envelope_cases():
        p = NM.plan(lib, case.c0, case.c1, case.batch, case.hw, case.groups)[1]
        line = []
        for ratio in NM.ENVELOPE_R:
            gn = _Gn(lib, case, "offset", dtype, inputs=NM.envelope_inputs(case, ratio, dtype, DEV))
            r = NM.gn_reference(gn.x, gn.gamma64, gn.beta64, case.groups, case.eps, False)
            out = gn.run()
            meas, stat = NM.envelope_figures(out, r, p, dtype)
            ok, worst, nbad = NM.check(out, r.ref, NM.gn_bound(r, p, dtype, "offset"))
            assert ok, f"{case.name} {dtype} R={ratio}: {nbad} elements beyond the criterion, worst ratio {worst}"
            line.append(f"R={ratio}: {meas:.2f} u (criterion {stat:.2g} u)")
        print(f"envelope {case.name} {dtype}: " + "; ".join(line))


def test_summary(lib):
    """What the tests above launched in this process, per operation, dtype and recipe (nothing to report when they did not run)."""
    print()
    for (op, dtype, recipe), (n, worst, where) in sorted(_WORST.items()):
        print(f"norm matrix {op:18s} {dtype:4s} {recipe:15s}: {n:4d} launches, worst err / criterion {worst:.3f} ({where})")
    print(f"norm matrix: {sum(v[0] for v in _WORST.values())} launched combinations, {time.time() - _T0:.0f} s since import")
