"""The three entries of the clipped SGD step on one tensor, bit for bit: idb_head_sgd_step (csrc/idb_head.hip, the norm met again
inside the step's launch), idb_sgd_clip_step and idb_sgd_clip_step_table with one tensor (csrc/idb_sgd.hip) are made of the same device
functions (csrc/idb_sgd.h) on the same geometry, so weights, momentum buffers and norms must be equal, not close.
Sizes, as the head's (d, c): one element (one part); 4097 elements (two parts, a ragged second); 4 196 352 elements (past 4096 x 1024:
the part cap holds and the stride loop runs twice for some threads)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import frtail_oracle as TO  # noqa: E402

from faceposegenerator_amd import _lib as L  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LR, MOM, WD, MAX_NORM = 0.1, 0.9, 5e-4, 5.0
SCALES = (4096.0, 1.0 / 4096.0)        # the gradient's scale per step: the clip active, then idle


def _hashed(n, salt):
    """n fp32 values in [-0.995, 1.005], none of them 0."""
    return torch.from_numpy(((TO._h(np.arange(n) + salt, 200) - 99.5) / 100.0).astype(np.float32)).to(DEV)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _head(lib, w, g, buf, d, c, first):
    wn = torch.empty((c, d), dtype=torch.float32, device=DEV)
    col_norm = torch.empty(c, dtype=torch.float64, device=DEV)
    bad = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    total = torch.zeros(1, dtype=torch.float64, device=DEV)
    work = torch.empty(L.IDB_HEAD_SGD_WS_BYTES, dtype=torch.uint8, device=DEV)
    L.check(lib.idb_head_sgd_step(w.data_ptr(), g.data_ptr(), buf.data_ptr(), d, c, LR, MOM, WD, MAX_NORM, int(first), wn.data_ptr(),
                                  col_norm.data_ptr(), bad.data_ptr(), total.data_ptr(), work.data_ptr(), L.IDB_HEAD_SGD_WS_BYTES, _stream()),
            "idb_head_sgd_step")
    wn2, col_norm2, bad2 = torch.empty_like(wn), torch.empty_like(col_norm), torch.full_like(bad, -1)
    L.check(lib.idb_head_pack(w.data_ptr(), d, c, wn2.data_ptr(), col_norm2.data_ptr(), bad2.data_ptr(), _stream()), "idb_head_pack")
    assert torch.equal(wn, wn2) and torch.equal(col_norm, col_norm2) and int(bad.item()) == int(bad2.item()) == 0
    return float(total.item())


def _list(lib, w, g, buf, d, c, first):
    one = lambda t: (C.c_void_p * 1)(t.data_ptr())      # noqa: E731
    total = torch.zeros(1, dtype=torch.float64, device=DEV)
    work = torch.empty(L.IDB_SGD_CLIP_WS_BYTES, dtype=torch.uint8, device=DEV)
    L.check(lib.idb_sgd_clip_step(1, one(w), one(g), one(buf), (C.c_int64 * 1)(w.numel()), LR, MOM, WD, MAX_NORM, int(first), total.data_ptr(),
                                  work.data_ptr(), L.IDB_SGD_CLIP_WS_BYTES, _stream()), "idb_sgd_clip_step")
    return float(total.item())


def _table(lib, w, g, buf, d, c, first):
    one = lambda v: torch.tensor([v], dtype=torch.int64).to(DEV)      # noqa: E731
    tw, tg, tb, tn = one(w.data_ptr()), one(g.data_ptr()), one(buf.data_ptr()), one(w.numel())
    need = lib.idb_sgd_clip_table_workspace_bytes(1)
    total = torch.zeros(1, dtype=torch.float64, device=DEV)
    work = torch.empty(need, dtype=torch.uint8, device=DEV)
    L.check(lib.idb_sgd_clip_step_table(1, tw.data_ptr(), tg.data_ptr(), tb.data_ptr(), tn.data_ptr(), LR, MOM, WD, MAX_NORM, int(first),
                                        total.data_ptr(), work.data_ptr(), need, _stream()), "idb_sgd_clip_step_table")
    return float(total.item())


@pytest.mark.parametrize("d,c", [(1, 1), (17, 241), (2049, 2048)])
def test_three_entries_one_tensor_bit_for_bit(lib, d, c):
    n = d * c
    grads = [_hashed(n, 9 + step) * scale for step, scale in enumerate(SCALES)]
    state = []
    for run in (_head, _list, _table):
        w = _hashed(n, 1).view(d, c)
        buf = torch.empty_like(w)
        norms = [run(lib, w, g, buf, d, c, step == 0) for step, g in enumerate(grads)]
        state.append((w, buf, norms))
    (wh, bh, nh), (wl, bl, nl), (wt, bt, nt) = state
    print(f"({d}, {c}): norms {nh}")
    assert nh == nl == nt and nh[0] > MAX_NORM > nh[1] > 0.0
    assert torch.equal(wh, wl) and torch.equal(wh, wt)
    assert torch.equal(bh, bl) and torch.equal(bh, bt)
    assert not torch.equal(wh, _hashed(n, 1).view(d, c))
