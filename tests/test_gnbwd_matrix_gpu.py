"""The GPU half of idb_groupnorm_bwd's matrix (tests/gnbwd_matrix.py): the two kernels launched on every case in both dtypes, each element
against the float64 reference under the criterion derived in gnbwd_matrix's docstring, every launch repeated and compared bit for bit,
dx0 / dx1 and the workspace between NaN guards and pre-filled with NaN (an unwritten element fails, a write outside is seen), dy and add
checked unchanged where they are not the output.  The statistics partials come from idb_groupnorm_stats on the device, or from the host in
64-pixel chunks (a chunk count that is not the backward's own).

Worst err / bound on MI355X, bf16 / f16 (test_summary prints them; DESIGN 4.19 records them): normal 0.996 / 0.997, offset 0.952 / 0.805,
constant_group 0.990 / 0.995, one_hot 0.993 / 0.998, silu_special 0.990 / 0.971, integer exact.  No constant of the criterion was raised."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gnbwd_matrix as GM  # noqa: E402
import matrix_common as MC  # noqa: E402
import norm_matrix as NM  # noqa: E402

pytestmark = pytest.mark.gpu
_WORST = MC.Worst("groupnorm_bwd", launches=True)
PARTS = 12


@pytest.mark.parametrize("part", range(PARTS))
@pytest.mark.parametrize("dt", MC.DTYPES)
def test_groupnorm_bwd(lib, dt, part):
    for case in GM.cases()[part::PARTS]:
        inp = GM.inputs(case, dt)
        ref = GM.reference(case, inp)
        fwd = GM.forward_plan(lib, case)
        rc, own = GM.plan(lib, case.c0, case.c1, case.batch, case.hw, case.groups)
        assert rc == 0
        bnd = GM.bound(case, ref, inp, dt, NM.gn_depth(fwd), own)
        runs = []
        for _ in range(2):
            rc, dx0, dx1, stat, ws = GM.run(lib, case, inp, dt)
            assert rc == 0, (case.name, lib.idb_last_error())
            assert stat.shape[1] == (case.stat_chunks or fwd.chunks)
            sums = ws.f32(f"{case.name}: workspace")
            used = case.batch * own.chunks * case.groups * 2
            assert np.isfinite(sums[:used]).all() and np.isnan(sums[used:]).all(), f"{case.name}: pass 1 writes [batch][chunks][groups][2] and nothing else"
            runs.append((dx0.T(f"{case.name}: dx0", dt), None if dx1 is None else dx1.T(f"{case.name}: dx1", dt)))
        MC.same_bits(f"{case.name}/{dt}: dx0, second run", runs[1][0][1], runs[0][0][1])
        shape = (case.batch, case.hw)
        got0 = runs[0][0][0].astype(np.float64).reshape(shape + (case.c0,))
        got1 = None
        if case.c1:
            MC.same_bits(f"{case.name}/{dt}: dx1, second run", runs[1][1][1], runs[0][1][1])
            got1 = runs[0][1][0].astype(np.float64).reshape(shape + (case.c1,))
        ok, ratio, text = GM.judge(case, ref, bnd, got0, got1)
        print(f"{dt}: {text}")
        _WORST.note(f"{case.recipe:14s} {dt}", ratio, case.name, launches=4)
        assert ok, f"{dt}: {text}"


def test_summary(lib):
    print()
    _WORST.show()
