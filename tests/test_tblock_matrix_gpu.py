"""The GPU half of the transformer block's kernel matrix (tests/tblock_matrix.py): idb_layernorm_bwd, idb_geglu_fwd, idb_geglu_bwd and
idb_adamw_clip_step_table launched on every case, recipe and dtype, each element against the float64 reference under the criteria derived
in tblock_matrix's docstring (none raised for the device), every launch repeated and compared bit for bit, every output between NaN
guards and pre-filled with NaN (an unwritten element fails, a write outside is seen), inputs checked unchanged.

Worst err / bound on MI355X (test_summary prints them; DESIGN 4.18 records them): see the table there."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import matrix_common as MC  # noqa: E402
import tblock_matrix as TM  # noqa: E402

pytestmark = pytest.mark.gpu
_WORST = MC.Worst("transformer-block kernels", launches=True)


@pytest.mark.parametrize("dt", MC.DTYPES)
def test_layernorm_bwd(lib, dt):
    for case in TM.ln_cases():
        x, dy, add, gamma = TM.ln_inputs(case, dt)
        ref = TM.ln_reference(case, x, dy, add, gamma)
        bnd = TM.ln_bound(case, ref, add, dt)
        runs = []
        for _ in range(2):
            rc, dx = TM.ln_run(lib, case, x, dy, add, gamma, dt)
            assert rc == 0, (case.name, lib.idb_last_error())
            runs.append(dx.T(f"{case.name}: dx", dt))
        MC.same_bits(f"{case.name}/{dt}: second run", runs[1][1], runs[0][1])
        got = runs[0][0].astype(np.float64).reshape(case.rows, case.c)
        _WORST.judge(f"layernorm_bwd {case.recipe:9s} {dt}", f"{case.name}/{dt}", got, ref["dx"], bnd, launches=2)


@pytest.mark.parametrize("dt", MC.DTYPES)
def test_geglu(lib, dt):
    for case in TM.geglu_cases():
        value, gate, dout = TM.geglu_inputs(case, dt)
        ref = TM.geglu_reference(value, gate, dout)
        bnd = TM.geglu_bound(ref, value, gate, dout, dt)
        runs = []
        for _ in range(2):
            rc1, rc2, out, dhg = TM.geglu_run(lib, case, value, gate, dout, dt)
            assert rc1 == 0 and rc2 == 0, (case.name, lib.idb_last_error())
            runs.append((out.T(f"{case.name}: out", dt), dhg.T(f"{case.name}: dhg", dt)))
        MC.same_bits(f"{case.name}/{dt}: out, second run", runs[1][0][1], runs[0][0][1])
        MC.same_bits(f"{case.name}/{dt}: dhg, second run", runs[1][1][1], runs[0][1][1])
        out = runs[0][0][0].astype(np.float64).reshape(case.rows, case.inner)
        dhg = runs[0][1][0].astype(np.float64).reshape(case.rows, 2 * case.inner)
        for name, got in (("out", out), ("dvalue", dhg[:, :case.inner]), ("dgate", dhg[:, case.inner:])):
            _WORST.judge(f"geglu {name:6s} {case.recipe:8s} {dt}", f"{case.name}/{dt}/{name}", got, ref[name], bnd[name], launches=2)


def test_adamw(lib):
    for case in TM.adam_cases():
        w, g, m, v = TM.adam_inputs(case)
        ow, om, ov, onorm, oskip = TM.adam_oracle(case, w, g, m, v)
        runs = []
        for _ in range(2):
            d = TM.AdamDevice(case, w, g, m, v)
            assert d.run(lib) == 0, (case.name, lib.idb_last_error())
            runs.append(d.results())
            for t, a in zip(d.g, g):
                MC.same_bits(f"{case.name}: the gradients are inputs", t.cpu().numpy(), a)
        for a, b in zip(runs[0][:3], runs[1][:3]):
            for i, (p, q) in enumerate(zip(a, b)):
                MC.same_bits(f"{case.name}: tensor {i}, second run", q, p)
        assert np.float64(runs[0][3]).tobytes() == np.float64(runs[1][3]).tobytes() and runs[0][4] == runs[1][4]
        dw, dm, dv, dnorm, dskip = runs[0]
        assert dskip == int(oskip), case.name
        if oskip:
            assert not np.isfinite(dnorm)
            for name, got, was in (("w", dw, w), ("m", dm, m), ("v", dv, v)):
                for i, (a, b) in enumerate(zip(got, was)):
                    MC.same_bits(f"{case.name}: {name}[{i}] after a skipped step", a, b)
            _WORST.note(f"adamw skipped ({case.poison})", 0.0, case.name, launches=6)
            continue
        bound = TM.adam_norm_bound(case, onorm)
        print(f"{case.name}: total_norm {dnorm!r} against {onorm!r}, |err| {abs(dnorm - onorm):.3e}, bound {bound:.3e}")
        assert abs(dnorm - onorm) <= bound
        _WORST.note("adamw norm", abs(dnorm - onorm) / bound, case.name)
        for name, got, want in (("w", dw, ow), ("m", dm, om), ("v", dv, ov)):
            ok, ratio, where = TM.adam_verdict(name, got, want)
            print(f"{case.name}: {name}: worst err / ulp {ratio:.4f} at {where}")
            assert ok, (case.name, where, ratio)
            _WORST.note(f"adamw {name} (err / ulp)", ratio, f"{case.name} {where}", launches=2)


def test_summary(lib):
    print()
    _WORST.show()
