"""The trunk's training blocks on the GPU (faceposegenerator_amd/frtrunk.py, csrc/idb_block.hip) against the float64 oracle
(tests/frblock_oracle.py): every element of every output as a share of its derived bound.  The forward is checked from the inputs; the
backward against the oracle's backward evaluated on the GPU's own saved context, so both sides are the same function of the same stored
values and the PReLU branch of an element near 0 is the GPU's own.  Then the table form of the clipped SGD step, and the trunk's
plumbing (Trunk, BackboneSGD, train_step_full) bit for bit against the pieces chained by hand."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import frblock_oracle as BO  # noqa: E402
import frtail_oracle as TO  # noqa: E402

from faceposegenerator_amd import _lib as L  # noqa: E402
from faceposegenerator_amd import arcface as A  # noqa: E402
from faceposegenerator_amd import frhead as H  # noqa: E402
from faceposegenerator_amd import frtail  # noqa: E402
from faceposegenerator_amd import frtrunk as T  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MEASURED = {}
P = "layer1.0."


def _note(what, err, bound):
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    ratio = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))))
    key = what.split("] ")[-1]
    if key not in MEASURED or ratio > MEASURED[key][0]:
        MEASURED[key] = (ratio, float(np.max(err)))
    print(f"{what}: largest error {float(np.max(err)):.3e}, {ratio:.4f} of its bound")


def _close(what, got, want, bound):
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == np.asarray(want).shape, (what, got.shape, np.asarray(want).shape)
    err = np.abs(got - want)
    bound = np.broadcast_to(bound, err.shape)
    _note(what, err, bound)
    assert (err <= bound).all(), (what, float(err.max()), float(np.max(bound)), float((err / np.maximum(bound, 1e-300)).max()))


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _sd(prm, prefix=""):
    return {prefix + k: torch.from_numpy((BO.w_to_upstream(v) if v.ndim == 4 else v).astype(np.float32)) for k, v in prm.items()}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).astype(np.float32)).to(DEV)


@functools.lru_cache(maxsize=None)
def _case(case):
    x, prm, g = BO.case_inputs(*case)
    return x, prm, g, BO.block_forward(x, prm, case[5], bounds=True)


def _block(prm, case):
    return T.TrainBlock(_sd(prm, P), P, case[1], case[2], case[5]).to(DEV)


def _ctx_np(out):
    c = out.ctx
    return {k: (_np(v) if v is not None else None) for k, v in c.items() if k in ("c1", "c2", "cd") or k.startswith(("stat", "affine"))}


def _check_block_forward(tag, out, fw, ds):
    ctx, b = _ctx_np(out), fw["bound"]
    for k in ("c1", "c2") + (("cd",) if ds else ()):
        _close(f"{tag} {k}", ctx[k], fw[k], b[k])
    _close(f"{tag} out", _np(out.output), fw["out"], b["out"])
    for n in ("1", "2", "3") + (("d",) if ds else ()):
        _close(f"{tag} bn mean", ctx["stat" + n][0], fw["stat" + n][0], b["stat" + n][0])
        _close(f"{tag} bn invstd", ctx["stat" + n][1], fw["stat" + n][1], b["stat" + n][1])
    return ctx


def _check_running(tag, blk, running, rb):
    for k, want in running.items():
        _close(f"{tag} {k.split('.')[-1]}", _np(blk.t[P + k]), want, rb[k])


@pytest.mark.parametrize("case", BO.BLOCK_CASES, ids=lambda v: "x".join(str(i) for i in v))
def test_block_against_oracle(lib, case):
    x, prm, g, fw = _case(case)
    ds = "downsample.0.weight" in prm
    blk = _block(prm, case)
    tag = f"[{'x'.join(str(i) for i in case)}]"
    xd = _dev(x)
    out = blk(xd)
    assert out.output.dtype == torch.float32 and tuple(out.output.shape) == fw["out"].shape
    ctx = _check_block_forward(tag, out, fw, ds)
    _check_running(f"{tag} after one call", blk, fw["running"], fw["bound"]["running"])
    assert all(v == 1 for v in blk.tracked.values()) and len(blk.tracked) == (4 if ds else 3)
    grad = blk.backward(out, _dev(g))
    bw = BO.block_backward(x, prm, case[5], g, ctx, bounds=True)
    keys = [k for k in BO.BLOCK_GRADS if k in prm]
    assert list(grad.params) == [P + k for k in blk_order(prm)] and len(keys) == (12 if ds else 9)
    for k in keys:
        _close(f"{tag} d {k}", _np(grad.params[P + k]), bw[k], bw["bound"][k])
    _close(f"{tag} d input", _np(grad.input), bw["input"], bw["bound"]["input"])
    up = grad.upstream()
    assert torch.equal(up[P + "conv2.weight"], grad.params[P + "conv2.weight"].permute(0, 3, 1, 2))
    # the second call blends the running statistics once more, from the first call's fp32 values
    prm2 = dict(prm)
    prm2.update({k: _np(blk.t[P + k]) for k in fw["running"]})
    fw2 = BO.block_forward(x, prm2, case[5], bounds=True)
    blk(xd)
    _check_running(f"{tag} after two calls", blk, fw2["running"], fw2["bound"]["running"])
    sd = blk.state_dict()
    assert sd[P + "bn2.num_batches_tracked"].item() == 2 and sd[P + "conv1.weight"].shape == (case[2], case[1], 3, 3)
    assert torch.equal(sd[P + "conv1.weight"], _sd(prm)["conv1.weight"])


def blk_order(prm):
    """Upstream's model.parameters() order inside a block."""
    order = ["bn1.weight", "bn1.bias", "conv1.weight", "bn2.weight", "bn2.bias", "prelu.weight", "conv2.weight", "bn3.weight", "bn3.bias"]
    return order + (["downsample.0.weight", "downsample.1.weight", "downsample.1.bias"] if "downsample.0.weight" in prm else [])


def test_stem_against_oracle(lib):
    B, Hh, W = BO.STEM_CASE
    img, prm, g = BO.stem_inputs(B, Hh, W)
    fw = BO.stem_forward(img, prm, bounds=True)
    stem = T.TrainStem(_sd(prm)).to(DEV)
    out = stem(_dev(img))
    ctx = _ctx_np(out)
    assert torch.equal(out.ctx["x"][..., 3], torch.zeros(B, Hh, W, device=DEV)) and torch.equal(out.ctx["x"][..., :3], _dev(img).permute(0, 2, 3, 1))
    _close("[stem] c1", ctx["c1"], fw["c1"], fw["bound"]["c1"])
    _close("[stem] out", _np(out.output), fw["out"], fw["bound"]["out"])
    _close("[stem] bn mean", ctx["stat1"][0], fw["stat1"][0], fw["bound"]["stat1"][0])
    _close("[stem] bn invstd", ctx["stat1"][1], fw["stat1"][1], fw["bound"]["stat1"][1])
    for k, want in fw["running"].items():
        _close(f"[stem] {k.split('.')[-1]}", _np(stem.t[k]), want, fw["bound"]["running"][k])
    grad = stem.backward(out, _dev(g))
    bw = BO.stem_backward(img, prm, g, ctx, bounds=True)
    assert list(grad.params) == list(BO.STEM_GRADS) and grad.input is None and tuple(grad.params["conv1.weight"].shape) == (64, 3, 3, 3)
    for k in BO.STEM_GRADS:
        _close(f"[stem] d {k}", _np(grad.params[k]), bw[k], bw["bound"][k])
    assert stem.tracked == {"bn1.num_batches_tracked": 1}


def test_plans_reach_slices_and_row_tiles(lib):
    """Some case of the matrix runs wgrad in >= 2 slices and some dgrad in >= 2 row tiles (from the plan query)."""
    slices, tiles = [], []
    for (B, cin, planes, Hh, W, s) in BO.BLOCK_CASES:
        for (ci, co, k, st, h, w) in ((cin, planes, 3, 1, Hh, W), (planes, planes, 3, s, Hh, W)):
            _, sl, rt = T.conv_plan(B, h, w, ci, co, k, st)
            slices.append(sl), tiles.append(rt)
    assert max(slices) >= 2 and max(tiles) >= 2


def test_eval_mode_against_oracle(lib):
    case = BO.BLOCK_CASES[1]
    x, prm, g, _ = _case(case)
    fw = BO.block_forward(x, prm, case[5], training=False, bounds=True)
    blk = _block(prm, case).eval()
    before = {k: v.clone() for k, v in blk.t.items()}
    out = blk(_dev(x))
    _check_block_forward("[eval]", out, fw, True)
    assert all(torch.equal(before[k], blk.t[k]) for k in before) and all(v == 0 for v in blk.tracked.values())
    with pytest.raises(ValueError, match="eval-mode forward"):
        blk.backward(out, torch.zeros_like(out.output))


def test_bit_identical_repeats(lib):
    case = BO.BLOCK_CASES[1]
    x, prm, g, _ = _case(case)
    res = []
    for _ in range(2):
        blk = _block(prm, case)
        out = blk(_dev(x))
        grad = blk.backward(out, _dev(g))
        res.append((out.output, out.ctx["c1"], out.ctx["c2"], out.ctx["cd"], grad.input, grad.params, dict(blk.t)))
    a, b = res
    for i in range(5):
        assert torch.equal(a[i], b[i]), i
    for d in (5, 6):
        assert all(torch.equal(a[d][k], b[d][k]) for k in a[d])


def test_padded_taps_are_zero(lib):
    """bn1's shift is large and the input is constant per channel: after bn1 every pixel holds the same per-channel value, so conv1's
    interior is one value per output channel and the border ring differs from it exactly by the taps that fall outside, which must
    contribute 0 and not the shift.  Eval mode, so that the constant input has usable statistics."""
    case = (2, 64, 64, 8, 8, 1)
    _, prm, _ = BO.case_inputs(*case)
    assert np.abs(prm["bn1.bias"]).min() >= 0.5
    x = np.broadcast_to(((TO._h(np.arange(64) + 3, 41) - 20) / 10.0), (2, 8, 8, 64)).astype(np.float32).astype(np.float64)
    fw = BO.block_forward(x, prm, 1, training=False, bounds=True)
    wrong = BO.block_forward(x, prm, 1, training=False, omit="pad_zero")
    out = _block(prm, case).eval()(_dev(x))
    c1 = _np(out.ctx["c1"])
    _close("[padded taps] c1", c1, fw["c1"], fw["bound"]["c1"])
    _close("[padded taps] out", _np(out.output), fw["out"], fw["bound"]["out"])
    ring = np.ones((8, 8), bool)
    ring[1:-1, 1:-1] = False
    assert np.abs(c1 - wrong["c1"])[:, ring].mean() > 100 * fw["bound"]["c1"].max()
    assert np.abs(c1[:, 1:-1, 1:-1] - c1[:1, 1:2, 1:2]).max() <= 2 * fw["bound"]["c1"].max()


# ---- the table form of the clipped SGD step ----------------------------------------------------------------------------------------
def _sgd_tensors(sizes, salt):
    ws = [((TO._h(np.arange(n) + 5 * i + salt, 201) - 100) / 100.0).astype(np.float32) for i, n in enumerate(sizes)]
    return ws


def _table(ts):
    return torch.tensor([t.data_ptr() for t in ts], dtype=torch.int64).to(DEV)


def _run_table(lib, ws, gs, bufs, lr, mom, wd, max_norm, first):
    n = len(ws)
    need = lib.idb_sgd_clip_table_workspace_bytes(n)
    work = torch.empty(need, dtype=torch.uint8, device=DEV)
    total = torch.zeros(1, dtype=torch.float64, device=DEV)
    numel = torch.tensor([w.numel() for w in ws], dtype=torch.int64).to(DEV)
    tw, tg, tb = _table(ws), _table(gs), _table(bufs)
    L.check(lib.idb_sgd_clip_step_table(n, tw.data_ptr(), tg.data_ptr(), tb.data_ptr(), numel.data_ptr(), lr, mom, wd, max_norm, int(first),
                                        total.data_ptr(), work.data_ptr(), need, torch.cuda.current_stream().cuda_stream), "table")
    return float(total.item())


def _run_list(lib, ws, gs, bufs, lr, mom, wd, max_norm, first):
    n = len(ws)
    arr = lambda ts: (C.c_void_p * n)(*[t.data_ptr() for t in ts])      # noqa: E731
    numel = (C.c_int64 * n)(*[w.numel() for w in ws])
    work = torch.empty(L.IDB_SGD_CLIP_WS_BYTES, dtype=torch.uint8, device=DEV)
    total = torch.zeros(1, dtype=torch.float64, device=DEV)
    L.check(lib.idb_sgd_clip_step(n, arr(ws), arr(gs), arr(bufs), numel, lr, mom, wd, max_norm, int(first), total.data_ptr(), work.data_ptr(),
                                  L.IDB_SGD_CLIP_WS_BYTES, torch.cuda.current_stream().cuda_stream), "list")
    return float(total.item())


def test_sgd_table_equals_list_bit_for_bit(lib):
    """Five tensors (one element, odd sizes, more than one part, more than 1024 parts' worth), two steps, the clip active then idle."""
    sizes = (1, 64, 5003, 36864, 4096 * 1024 + 77)
    state = []
    for run in (_run_table, _run_list):
        ws = [torch.from_numpy(w).to(DEV) for w in _sgd_tensors(sizes, 1)]
        bufs = [torch.empty_like(w) for w in ws]
        norms = []
        for step, scale in enumerate((1.0, 1e-4)):
            gs = [torch.from_numpy(w).to(DEV) * scale for w in _sgd_tensors(sizes, 9 + step)]
            norms.append(run(lib, ws, gs, bufs, 0.1, 0.9, 5e-4, 5.0, step == 0))
        state.append((ws, bufs, norms))
    (wa, ba, na), (wb, bb, nb) = state
    assert na == nb and na[0] > 5.0 > na[1]
    for i in range(len(sizes)):
        assert torch.equal(wa[i], wb[i]) and torch.equal(ba[i], bb[i]), i


def test_sgd_table_forty_tensors_against_oracle(lib):
    sizes = tuple(1 + (37 * i) % 300 for i in range(40))
    w0 = _sgd_tensors(sizes, 2)
    ws = [torch.from_numpy(w).to(DEV) for w in w0]
    bufs = [torch.empty_like(w) for w in ws]
    ref_w, ref_b = [w.astype(np.float64) for w in w0], None
    total = sum(sizes)
    eb = [np.zeros(n) for n in sizes]
    ew = [np.zeros(n) for n in sizes]
    lr, mom, wd = 0.1, 0.9, 5e-4
    for step, scale in enumerate((0.5, 0.01, 0.3)):
        g0 = [g * np.float32(scale) for g in _sgd_tensors(sizes, 11 + step)]
        gs = [torch.from_numpy(g).to(DEV) for g in g0]
        ref_w, ref_b, ref_norm = TO.sgd_step(ref_w, [g.astype(np.float64) for g in g0], ref_b, lr, mom, wd, 5.0)
        norm = _run_table(lib, ws, gs, bufs, lr, mom, wd, 5.0, step == 0)
        assert abs(norm - ref_norm) <= (total + 8) * TO.U64 * ref_norm
        coef = min(1.0, 5.0 / (ref_norm + 1e-6))
        for i in range(len(sizes)):
            eb[i], ew[i] = TO.sgd_bound(ref_w[i], ref_b[i], eb[i], ew[i], lr, mom, wd, coef * np.abs(g0[i].astype(np.float64)), total)
            _close(f"sgd table weight, step {step + 1}", _np(ws[i]), ref_w[i], ew[i])
            _close(f"sgd table momentum, step {step + 1}", _np(bufs[i]), ref_b[i], eb[i])


def test_refusals_leave_outputs_untouched(lib):
    f32 = dict(dtype=torch.float32, device=DEV)
    x, w = torch.ones((2, 8, 8, 64), **f32), torch.ones((64, 3, 3, 64), **f32)
    out = torch.full((2, 8, 8, 64), 7.0, **f32)
    work = torch.full((1 << 20,), 7, dtype=torch.uint8, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    for bad in ((2, 8, 8, 32, 64, 3, 1), (2, 8, 8, 64, 96, 3, 1), (2, 129, 8, 64, 64, 3, 1), (1025, 8, 8, 64, 64, 3, 1), (2, 8, 8, 64, 64, 3, 3)):
        d = L.BlkConvDesc()
        d.b, d.h, d.w, d.cin, d.cout, d.ksize, d.stride = bad
        d.x, d.weight = x.data_ptr(), w.data_ptr()
        assert lib.idb_blk_conv_forward(C.byref(d), out.data_ptr(), stream) != 0
        assert lib.idb_blk_conv_dgrad(C.byref(d), x.data_ptr(), out.data_ptr(), stream) != 0
        assert lib.idb_blk_conv_wgrad(C.byref(d), x.data_ptr(), out.data_ptr(), work.data_ptr(), work.numel(), stream) != 0
    stat = torch.full((2, 64), 7.0, dtype=torch.float64, device=DEV)
    aff, rm, rv = torch.full((2, 64), 7.0, **f32), torch.full((64,), 7.0, **f32), torch.full((64,), 7.0, **f32)
    flags = torch.zeros(2, dtype=torch.int32, device=DEV)
    one = torch.ones(64, **f32)
    args = (one.data_ptr(), one.data_ptr(), rm.data_ptr(), rv.data_ptr(), stat.data_ptr(), aff.data_ptr(), flags.data_ptr(), work.data_ptr(),
            work.numel(), stream)
    assert lib.idb_blk_bn_forward(x.data_ptr(), 1, 64, 1, 1e-5, 0.1, *args) != 0          # one value per channel in training
    assert lib.idb_blk_bn_forward(x.data_ptr(), 128, 96, 1, 1e-5, 0.1, *args) != 0
    assert lib.idb_blk_bn_forward(x.data_ptr(), 128, 64, 1, 1e-5, 0.1, *args[:7], work.data_ptr(), 16, stream) != 0      # workspace too small
    torch.cuda.synchronize()
    for t in (out, stat, aff, rm, rv):
        assert bool((t == 7.0).all())
    assert bool((work == 7).all()) and not bool(flags.any())
    # the Python layer: a NaN in the input is found on the device, and the block is left as it was
    case = BO.BLOCK_CASES[0]
    xg, prm, g, _ = _case(case)
    blk = _block(prm, case)
    before = {k: v.clone() for k, v in blk.t.items()}
    bad = _dev(xg)
    bad[1, 2, 3, 5] = float("nan")
    with pytest.raises(ValueError, match="non-finite"):
        blk(bad)
    assert all(torch.equal(before[k], blk.t[k]) for k in before) and all(v == 0 for v in blk.tracked.values())
    with pytest.raises(ValueError, match="expected a float32 tensor with 64 channels"):
        blk(_dev(xg)[..., :32])
    with pytest.raises(ValueError, match="one value per channel"):
        blk(_dev(xg)[:1, :1, :1])
    out = blk(_dev(xg))
    with pytest.raises(ValueError, match="grad: expected fp32"):
        blk.backward(out, _dev(g)[:1])
    with pytest.raises(ValueError, match="not produced by this block"):
        _block(prm, case).backward(out, _dev(g))


# ---- trunk plumbing: layers [1, 1, 1, 1], B = 2, 32 x 32 images (a 2 x 2 x 512 map; the stage with n = 64) ---------------------------
LAYERS, NCLS = [1, 1, 1, 1], 5


def _trunk_sd():
    sd = A.synth_weights("r18", seed=7)
    return {k: v for k, v in sd.items() if k in T.trunk_param_shapes(LAYERS)}


def _images():
    return _dev(BO._u((2, 3, 32, 32), 77))


def _fresh(loss="CosFace", lr=0.05):
    trunk = T.Trunk(_trunk_sd(), layers=LAYERS).to(DEV)
    stage = frtail.EmbeddingStage.from_synthetic(3, ch=512, hw=4, n=64, dropout=0.4).to(DEV)
    kernel = torch.from_numpy(((TO._h(np.arange(64 * NCLS) + 13, 2001).reshape(64, NCLS) - 1000) / 1000.0 * 0.05).astype(np.float32))
    header = H.MarginHeader(kernel, loss).to(DEV)
    return trunk, stage, header, T.BackboneSGD(trunk, stage, lr), H.HeaderSGD(header, 2 * lr)


def _keep():
    return torch.from_numpy((TO._h(np.arange(2 * 2048) + 5, 10) >= 4).reshape(2, 2048))


def test_trunk_backward_equals_blocks_chained_by_hand(lib):
    trunk = T.Trunk(_trunk_sd(), layers=LAYERS).to(DEV)
    tout = trunk(_images())
    assert tuple(tout.map.shape) == (2, 2, 2, 512) and trunk.map_size(32, 32) == (2, 2) and len(tout.outs) == 5
    gm = _dev(BO._u((2, 2, 2, 512), 5))
    got = trunk.backward(tout, gm)
    want, g = {}, gm
    for blk, bo in zip(reversed(trunk.blocks), reversed(tout.outs[1:])):
        bg = blk.backward(bo, g)
        want.update(bg.params)
        g = bg.input
    want.update(trunk.stem.backward(tout.outs[0], g).params)
    assert list(got) == trunk.trainable() and sorted(got) == sorted(want) and len(got) == 4 + 4 * 12
    for k in got:
        assert torch.equal(got[k], want[k]), k
        assert tuple(got[k].shape) == tuple(trunk.tensor(k).shape) and bool(torch.isfinite(got[k]).all()) and bool((got[k] != 0).any()), k
    assert all(v == 1 for m in trunk.modules for v in m.tracked.values())


def test_train_step_full(lib):
    """One step against (1) a twin set taking the same step through the public calls chained by hand, bit for bit, and (2) the float64
    SGD applied to the GPU's own gradients, within sgd_bound."""
    one, two = _fresh(), _fresh()
    trunk, stage, header, opt_b, opt_h = two
    img, lab, keep = _images(), torch.tensor([1, 3]), _keep()
    keys = opt_b.keys
    w0 = [_np(opt_b._weight(k)) for k in keys]
    res = T.train_step_full(*one, img, lab, keep=keep)
    tout = trunk(img)
    out = stage(tout.map, keep=keep)
    hl, hg = header.loss_and_grad(out.embeddings, lab)
    grad = stage.backward(out, hg.embeddings)
    tg = trunk.backward(tout, grad.input)
    nb = opt_b.step(tg, grad)
    nh = opt_h.step(hg.kernel)
    assert (res["loss"], res["acc"], res["correct"], res["grad_norm_backbone"], res["grad_norm_header"]) == (hl.loss, hl.acc, hl.correct, nb, nh)
    assert res["grad_norm_stage"] == nb and res["grad_input"] is None and np.isfinite(res["loss"]) and nb > 0
    for k in keys:
        assert torch.equal(one[3]._weight(k), opt_b._weight(k)) and torch.equal(one[3]._buf[k], opt_b._buf[k]), k
    for ma, mb in zip(one[0].modules, trunk.modules):
        assert ma.tracked == mb.tracked and all(torch.equal(ma.t[k], mb.t[k]) for k in ma.t)
    assert all(torch.equal(one[1].t[k], stage.t[k]) for k in stage.t) and torch.equal(one[2].kernel, header.kernel)
    assert len(keys) == 4 + 4 * 12 + 5 and opt_b.steps == 1
    # the float64 step from the GPU's gradients
    gs = dict(tg)
    gs.update({"bn2.weight": grad.bn2_weight, "bn2.bias": grad.bn2_bias, "fc.weight": grad.fc_weight, "fc.bias": grad.fc_bias,
               "features.bias": grad.features_bias})
    g64 = [_np(gs[k]) for k in keys]
    ref_w, ref_b, ref_norm = TO.sgd_step(w0, g64, None, opt_b.lr, 0.9, 5e-4, 5.0)
    total = sum(w.size for w in w0)
    assert abs(nb - ref_norm) <= (total + 8) * TO.U64 * ref_norm
    coef = min(1.0, 5.0 / (ref_norm + 1e-6))
    for i, k in enumerate(keys):
        eb, ew = TO.sgd_bound(ref_w[i], ref_b[i], 0.0 * w0[i], 0.0 * w0[i], opt_b.lr, 0.9, 5e-4, coef * np.abs(g64[i]), total)
        _close("train_step_full weight", _np(opt_b._weight(k)), ref_w[i], ew)
        _close("train_step_full momentum", _np(opt_b._buf[k]), ref_b[i], eb)
        assert not np.array_equal(_np(opt_b._weight(k)), w0[i]), k
    # the optimiser's state survives a round trip in upstream's layouts
    sd = opt_b.state_dict()
    assert tuple(sd["momentum_buffers"]["layer2.0.conv1.weight"].shape) == (128, 64, 3, 3)
    again = T.BackboneSGD(trunk, stage, 0.5)
    again.load_state_dict(sd)
    assert again.lr == opt_b.lr and again.steps == 1 and all(torch.equal(again._buf[k], opt_b._buf[k]) for k in keys)
    # a second step runs with the momentum buffers
    res2 = T.train_step_full(*one, img, lab, keep=keep)
    assert np.isfinite(res2["loss"]) and one[3].steps == 2


def test_merged_state_dict_loads_into_arcface(lib):
    sd = A.synth_weights("r18", seed=5)
    trunk = T.Trunk(sd, arch="r18").to(DEV)
    stage = frtail.EmbeddingStage.from_state_dict(sd).to(DEV)
    merged = trunk.merged_state_dict(stage)
    A.check_state_dict(merged, "r18")
    net = A.ArcFace.from_state_dict(merged, "r18")
    assert net is not None and all(torch.equal(merged[k], sd[k].float()) for k in sd if not k.endswith("num_batches_tracked"))


def test_print_measured(lib):
    """The largest error of each quantity as a share of its bound (for DESIGN 4.15); run the whole file to fill it."""
    for key, (ratio, err) in sorted(MEASURED.items()):
        print(f"measured {key}: {ratio:.4f} of the bound (largest error {err:.3e})")
    assert all(r <= 1.0 for r, _ in MEASURED.values())
