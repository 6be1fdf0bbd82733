"""Every case of the MTCNN kernel test matrix (tests/detect_matrix.py) on the device, through the C ABI, element by element against the
float64 references and the criteria derived there (area: (u |q| + u |q - sub|) |mul| + u |out|; conv: gamma_(K+1) S max(1, |slope|); pool
and the suppression mask: bit equality; softmax pair: 3x the fp32 emulation's worst error in ulps of p1, at least 2 ulp; decisions equal
float64's wherever float64 is further from the threshold than the element's bound).

Every output buffer lies between 64 guard elements of a NaN bit pattern (0xDEADBEEFCAFEF00D words around the mask) that are checked after
the launch; an output element the kernel did not write keeps that NaN and fails its criterion.  Every case is launched twice into separate
buffers and the two results must be equal bit for bit.  One chained test per network walks mtcnn.PNET / RNET / ONET, the dense layer and the
heads with the seeded synthetic weights: each layer is fed the GPU's own previous output and compared with the float64 reference of that
layer on that same input, so every real layer shape gets its own bound.  A failure names the case, the worst element's index, its error
and its bound.  test_summary prints the worst err / bound per kernel (recorded in profiles/mtcnn/README.md, never used as thresholds)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import detect_matrix as D  # noqa: E402
import matrix_common as MC  # noqa: E402
from faceposegenerator_amd import _lib as L  # noqa: E402

pytestmark = pytest.mark.gpu

W = MC.Worst("detect matrix", launches=True)


def _twice(n, launch, what):
    """launch(out pointer) into two separate guarded buffers; the results must be bit-equal.  Returns the first."""
    a, b = MC.Guarded(n), MC.Guarded(n)
    launch(a.ptr)
    launch(b.ptr)
    torch.cuda.synchronize()
    ra, rb = a.f32(what), b.f32(what)
    assert np.array_equal(ra.view(np.uint32), rb.view(np.uint32)), f"{what}: a relaunch gave different bits"
    return ra


# ---- launches through the C ABI ------------------------------------------------------------------------------------------------------
def _area(lib, img_d, shape, boxes_np, oh, ow, what, sub=D.SUB, mul=D.MUL):
    b, h, w, c = shape
    n = boxes_np.shape[0]
    bx = MC.dev(boxes_np if n else np.zeros((1, 5), np.int32))

    def launch(ptr):
        L.check(lib.idb_crop_resize_area_u8(img_d.data_ptr(), b, h, w, c, bx.data_ptr(), n, ptr, oh, ow, sub, mul, MC.stream()), what)
    return _twice(n * c * oh * ow, launch, what).reshape(n, c, oh, ow)


def _conv(lib, x, wt, bias, slope, what):
    b, cin, h, w = x.shape
    cout, _, kh, kw = wt.shape
    xd, wd = MC.dev(x), MC.dev(wt)
    bd, sd = (None if bias is None else MC.dev(bias)), (None if slope is None else MC.dev(slope))

    def launch(ptr):
        L.check(lib.idb_conv2d_f32(xd.data_ptr(), wd.data_ptr(), None if bd is None else bd.data_ptr(), None if sd is None else sd.data_ptr(), ptr,
                                   b, cin, h, w, cout, kh, kw, MC.stream()), what)
    oh, ow = h - kh + 1, w - kw + 1
    return _twice(b * cout * oh * ow, launch, what).reshape(b, cout, oh, ow)


def _pool(lib, x, k, s, what):
    p, h, w = x.shape
    xd = MC.dev(x)
    oh, ow = D.pool_outputs(h, k, s), D.pool_outputs(w, k, s)

    def launch(ptr):
        L.check(lib.idb_maxpool2d_f32(xd.data_ptr(), ptr, p, h, w, k, s, MC.stream()), what)
    return _twice(p * oh * ow, launch, what).reshape(p, oh, ow)


def _softmax(lib, x, what):
    b, _, hw = x.shape
    xd = MC.dev(x)

    def launch(ptr):
        L.check(lib.idb_softmax_pairs_f32(xd.data_ptr(), ptr, b, hw, MC.stream()), what)
    return _twice(b * hw, launch, what).reshape(b, hw)


def _check_conv(got, x, wt, bias, slope, what):
    ref, bound, _ = D.conv_reference(x, wt, bias, slope)
    W.judge("idb_conv2d_f32", what, got, ref, bound, 2)


def _check_softmax(got, x, what, thr_indices=(0, 1)):
    ref, bound, bar, emu = D.sm_bound(x)
    res = D.check(got, ref, bound)
    worst_ulp = float((np.abs(got.astype(np.float64) - ref) / D.ulp32(ref)).max())
    print(f"{D.describe(what, res)}; {worst_ulp:.3f} ulp of p1, bar {bar:.3f} ulp (emulation {emu:.3f})")
    assert res[0], D.describe(what, res)
    W.note("idb_softmax_pairs_f32", res[1], what, 2)
    W.note("idb_softmax_pairs_f32 [ulp of p1]", worst_ulp, what)
    for ti in thr_indices:
        g, r, decided = D.decisions(got, ref, bound, ti)
        assert (~decided).mean() <= D.UNDECIDED_CAP, f"{what}: {int((~decided).sum())} of {decided.size} undecided at threshold {ti}"
        wrong = np.argwhere(decided & (g != r))
        assert wrong.size == 0, f"{what}: decision {ti} differs from float64 at {wrong[0].tolist()}: p = {ref[tuple(wrong[0])]!r}"


# ---- the cases -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def images():
    return {k: (MC.dev(v), v.shape) for k, v in D.area_images().items()}


@pytest.mark.parametrize("case", D.area_cases(), ids=lambda c: c.name)
def test_area(lib, images, case):
    img_d, shape = images[case.image]
    got = _area(lib, img_d, shape, case.boxes_np, case.oh, case.ow, case.name)
    ref, bound = D.area_reference(D.area_images()[case.image], case)
    W.judge("idb_crop_resize_area_u8", case.name, got, ref, bound, 2)


@pytest.mark.parametrize("case", D.conv_cases(), ids=lambda c: c.name)
def test_conv(lib, case):
    x, wt, bias, slope = D.conv_inputs(case)
    _check_conv(_conv(lib, x, wt, bias, slope, case.name), x, wt, bias, slope, case.name)


def test_pool_grid(lib):
    """All 13 x 13 x 6 (h, w, k, stride) in one pair of output buffers: the regions of the cases are separated by guard elements, every
    launch is queued, and each buffer comes back in one copy."""
    cases = D.pool_cases()
    inputs = [D.pool_inputs(*c) for c in cases]
    refs = [D.pool_reference(x, c[2], c[3]) for x, c in zip(inputs, cases)]
    xin = MC.dev(np.concatenate([x.reshape(-1) for x in inputs]))
    in_off = np.cumsum([0] + [x.size for x in inputs])
    out_off, pos = [], MC.GUARD
    for r in refs:
        out_off.append(pos)
        pos += r.size + MC.GUARD
    bufs = [torch.full((pos,), D.NAN32, dtype=torch.int32, device=MC.DEV) for _ in range(2)]
    for buf in bufs:
        for c, x, i0, o0 in zip(cases, inputs, in_off, out_off):
            L.check(lib.idb_maxpool2d_f32(xin.data_ptr() + 4 * int(i0), buf.data_ptr() + 4 * o0, x.shape[0], c[0], c[1], c[2], c[3], MC.stream()), f"pool {c}")
    torch.cuda.synchronize()
    host = [b.cpu().numpy() for b in bufs]
    assert np.array_equal(host[0], host[1]), "pool: a relaunch gave different bits"
    written = np.zeros(pos, bool)
    for c, r, o0 in zip(cases, refs, out_off):
        written[o0:o0 + r.size] = True
        MC.same_bits(f"pool (h, w, k, stride) = {c}", host[0][o0:o0 + r.size].view(np.float32).reshape(r.shape), r)
    assert (host[0][~written] == D.NAN32).all(), "pool: guard elements overwritten"
    W.note("idb_maxpool2d_f32", 0.0, "bit-equal on every case", 2 * len(cases))


@pytest.mark.parametrize("hw", D.SM_HW)
def test_softmax_pairs(lib, hw):
    x = D.sm_inputs(hw)
    _check_softmax(_softmax(lib, x, f"softmax hw {hw}"), x, f"softmax hw {hw}")


@pytest.mark.parametrize("case", D.nms_cases(), ids=lambda c: c.name)
def test_nms_mask(lib, case):
    from faceposegenerator_amd import mtcnn as M
    boxes, image, scores = D.nms_inputs(case)
    n, words = case.n, case.words
    bd, imd = MC.dev(boxes), (MC.dev(image) if case.with_image else None)
    bufs = [MC.Guarded(n * words, 8, pattern=D.WORD_GUARD) for _ in range(2)]
    for buf in bufs:
        L.check(lib.idb_nms_mask(bd.data_ptr(), MC.ptr(imd), n, case.thr, int(case.method == "Min"), int(case.plus_one), buf.ptr, MC.stream()), case.name)
    torch.cuda.synchronize()
    host = [b.raw(case.name) for b in bufs]
    assert np.array_equal(host[0], host[1]), f"{case.name}: a relaunch gave different bits"
    mask = host[0].reshape(n, words)
    want = D.nms_mask_fp32(case, boxes, image)
    diff = np.argwhere(mask != want)
    assert diff.size == 0, f"{case.name}: word {diff[0].tolist()} is {int(mask[tuple(diff[0])]):#x}, the fp32 restatement has {int(want[tuple(diff[0])]):#x}"
    assert D.left_of_diagonal_zero(mask), f"{case.name}: a bit at or left of the diagonal is set"
    # decisions against float64: equal wherever fp32 and float64 agree, and those are all but 1 %
    im = image if case.with_image else None
    b64 = D.pack_bits(D.nms_bits(boxes, im, case.thr, case.method, case.plus_one, np.float64))
    bad, pairs = D.nms_undecided(case, boxes, image)
    assert bad <= D.UNDECIDED_CAP * max(pairs, 1) and int(sum(bin(int(v)).count("1") for v in (mask ^ b64).reshape(-1))) == bad, case.name
    idxs = image if case.with_image else np.zeros(n, np.int32)
    kept = D.bnms_order(D.host_scan(mask), idxs, scores)
    assert np.array_equal(kept, M._batched_nms(boxes, scores, idxs, case.thr, case.method, case.plus_one)), f"{case.name}: the scan keeps other boxes"
    W.note("idb_nms_mask", 0.0, "bit-equal on every case", 2)


# ---- one chained walk per network ----------------------------------------------------------------------------------------------------
CHAIN = {
    "pnet": dict(image="noise3", boxes=((0, 0, 61, 0, 45), (1, 0, 61, 0, 45)), size=(14, 17), thr=0),
    "rnet": dict(image="noise3", boxes=((0, 3, 44, 2, 40), (1, 10, 61, 5, 45)), size=(24, 24), thr=1),
    "onet": dict(image="ramp3", boxes=((0, 0, 61, 0, 45), (1, 7, 50, 1, 44)), size=(48, 48), thr=1),
}


@pytest.mark.parametrize("net", ("pnet", "rnet", "onet"))
def test_chain(lib, images, net):
    from faceposegenerator_amd import mtcnn as M
    sd = {k: v.numpy().astype(np.float32) for k, v in M.synth_weights(5)[net].items()}
    cfg = CHAIN[net]
    case = D.AreaCase(f"chain_{net}_input", cfg["image"], cfg["boxes"], *cfg["size"])
    img_d, shape = images[case.image]
    x = _area(lib, img_d, shape, case.boxes_np, case.oh, case.ow, case.name)
    ref, bound = D.area_reference(D.area_images()[case.image], case)
    MC.within(case.name, x, ref, bound)
    for l in {"pnet": M.PNET, "rnet": M.RNET, "onet": M.ONET}[net]:
        if l[0] == "conv":
            what = f"chain {net} {l[1]} {x.shape}"
            wt, bias, slope = sd[f"{l[1]}.weight"], sd[f"{l[1]}.bias"], sd[f"{l[3]}.weight"]
            y = _conv(lib, x, wt, bias, slope, what)
            _check_conv(y, x, wt, bias, slope, what)
        else:
            what = f"chain {net} pool {l[1:]} {x.shape}"
            b, c, h, w = x.shape
            y = _pool(lib, x.reshape(b * c, h, w), l[1], l[2], what)
            MC.same_bits(what, y, D.pool_reference(x.reshape(b * c, h, w), l[1], l[2]))
            assert y.shape[1:] == (M.pool_out(h, l[1], l[2]), M.pool_out(w, l[1], l[2]))
            y = y.reshape(b, c, *y.shape[1:])
        x = np.ascontiguousarray(y)
    if net == "pnet":
        heads = [("conv4_1", sd["conv4_1.weight"]), ("conv4_2", sd["conv4_2.weight"])]
    else:
        dense, cout = ("dense4", 128) if net == "rnet" else ("dense5", 256)
        assert x.shape[2:] == (3, 3)
        # the dense layer as a convolution over the whole map, as MTCNN.__init__ lays it out: upstream flattens x.permute(0, 3, 2, 1)
        wt = np.ascontiguousarray(sd[f"{dense}.weight"].reshape(cout, 3, 3, x.shape[1]).transpose(0, 3, 2, 1))
        what = f"chain {net} {dense} K = {wt[0].size}"
        slope = sd[f"prelu{dense[-1]}.weight"]
        y = _conv(lib, x, wt, sd[f"{dense}.bias"], slope, what)
        _check_conv(y, x, wt, sd[f"{dense}.bias"], slope, what)
        x = y
        nxt = int(dense[-1]) + 1
        heads = [(f"dense{nxt}_{i}", sd[f"dense{nxt}_{i}.weight"].reshape(-1, cout, 1, 1)) for i in ((1, 2) if net == "rnet" else (1, 2, 3))]
    for name, wt in heads:
        what = f"chain {net} {name}"
        y = _conv(lib, x, np.ascontiguousarray(wt), sd[f"{name}.bias"], None, what)
        _check_conv(y, x, wt, sd[f"{name}.bias"], None, what)
        if name.endswith("_1"):
            logits = np.ascontiguousarray(y.reshape(y.shape[0], 2, -1))
            p = _softmax(lib, logits, f"chain {net} softmax")
            _check_softmax(p, logits, f"chain {net} softmax", (cfg["thr"],))


def test_summary():
    W.show()
