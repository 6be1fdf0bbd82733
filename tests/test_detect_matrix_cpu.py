"""The CPU half of the MTCNN kernel test matrix (tests/detect_matrix.py), no GPU: the float64 references against torch's own operators
in float64, the pooling size rule of mtcnn.py against torch's output shapes, the conditions the input recipes must meet (exact window
sums, both PReLU branches on every channel, at most 1 % undecided decisions), the teeth of the criteria (every non-harmless defect of
detect_matrix.DEFECTS fails its named case; the fp32 emulations of the unmodified kernels pass every case) and every argument check of
csrc/idb_mtcnn.hip, which answers before any HIP call."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import detect_matrix as D  # noqa: E402
import matrix_common as MC  # noqa: E402

AREA = D.area_cases()
CONV = D.conv_cases()
NMS = D.nms_cases()


# ---- the references against torch, float64 -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in AREA if c.boxes], ids=lambda c: c.name)
def test_area_reference_is_torch_area_interpolation(case):
    img = D.area_images()[case.image]
    ref, bound = D.area_reference(img, case)
    assert ref.shape == (len(case.boxes), img.shape[3], case.oh, case.ow) and np.isfinite(ref).all() and (bound > 0).all()
    for k, (i, y0, y1, x0, x1) in enumerate(case.boxes):
        assert 0 <= y0 < y1 <= img.shape[1] and 0 <= x0 < x1 <= img.shape[2] and 0 <= i < img.shape[0]
        crop = torch.from_numpy(img[i, y0:y1, x0:x1].astype(np.float64)).permute(2, 0, 1)[None]
        want = (F.interpolate(crop, size=(case.oh, case.ow), mode="area")[0].numpy() - D.SUB) * D.MUL
        assert np.abs(ref[k] - want).max() <= 1e-13, case.name


def test_area_cases_cover_what_they_were_chosen_for():
    names = {c.name for c in AREA}
    assert len(names) == len(AREA)
    assert D.pyramid_sizes(61, 45) == [(37, 28), (26, 20), (19, 14)]
    last = D.area_images()["noise3"].shape
    assert any(i == last[0] - 1 and y1 == last[1] and x1 == last[2] for c in AREA if c.image == "noise3" for i, _, y1, _, x1 in c.boxes)
    assert any(not c.boxes for c in AREA)
    assert {D.area_images()[c.image].shape[3] for c in AREA} == {1, 3, 4}
    for c in AREA:
        assert D.area_sum_exact(c), (c.name, D.area_window_pixels(c))        # 255 * window pixels < 2^24: the fp32 sum is exact
    assert max(D.area_window_pixels(c) for c in AREA) == 61 * 45


@pytest.mark.parametrize("case", CONV, ids=lambda c: c.name)
def test_conv_reference_is_torch_conv2d_prelu(case):
    x, wt, bias, slope = D.conv_inputs(case)
    ref, bound, z = D.conv_reference(x, wt, bias, slope)
    t = lambda a: None if a is None else torch.from_numpy(a.astype(np.float64))   # noqa: E731
    want = F.conv2d(t(x), t(wt), t(bias))
    if slope is not None:
        want = F.prelu(want, t(slope))
    assert ref.shape == tuple(want.shape) and ref.size == case.outputs
    assert (np.abs(ref - want.numpy()) <= 1e-12 * bound / D.gamma(case.k + 1)).all()
    if case.prelu and case.recipe == "mixed":           # both branches of PReLU on every channel
        zc = z.transpose(1, 0, 2, 3).reshape(case.cout, -1)
        assert (zc > 0).any(1).all() and (zc < 0).any(1).all(), case.name
    if case.recipe == "negative":
        assert (z < 0).all()


def test_conv_cases_cover_what_they_were_chosen_for():
    by = {c.name: c for c in CONV}
    assert len(by) == len(CONV)
    assert by["rnet_dense4_k576"].k == 576 and by["onet_dense5_k1152"].k == 1152
    assert by["outputs256"].outputs == 256 and by["outputs257"].outputs == 257
    assert any(c.kh == c.h and c.w > c.kw for c in CONV) and {(2, 3), (3, 1)} <= {(c.kh, c.kw) for c in CONV}
    assert any(not c.bias for c in CONV) and any(c.cin == 1 and c.cout == 1 for c in CONV)
    assert any(c.kh == 1 and c.prelu for c in CONV) and any(c.kh == 1 and not c.prelu for c in CONV)
    # the trunks' geometries are the ones mtcnn.py's layer lists produce from 14 x 17, 24 x 24 and 48 x 48
    from faceposegenerator_amd import mtcnn as M
    for net, layers, (h, w) in (("pnet", M.PNET, (14, 17)), ("rnet", M.RNET, (24, 24)), ("onet", M.ONET, (48, 48))):
        for l in layers:
            if l[0] == "conv":
                c = by[f"{net}_{l[1]}"]
                assert (c.cin, c.cout, c.kh, c.kw, c.h, c.w) == (l[2][0], l[2][1], l[2][2], l[2][2], h, w), c.name
                h, w = h - l[2][2] + 1, w - l[2][2] + 1
            else:
                h, w = M.pool_out(h, l[1], l[2]), M.pool_out(w, l[1], l[2])
        if net != "pnet":
            assert (h, w) == (3, 3)


def _torch_pool_shape(n, k, s):
    try:
        return F.max_pool2d(torch.zeros(1, 1, n, n, dtype=torch.float64), k, s, ceil_mode=True).shape[-1]
    except RuntimeError:
        return None


def test_pool_size_rule_is_torchs():
    """mtcnn.pool_out (what MTCNN._pool allocates) and detect_matrix.pool_outputs against torch's output shape over the whole grid; where
    torch refuses (an input smaller than the window leaves it no output) both give the one clipped window the kernel computes."""
    from faceposegenerator_amd import mtcnn as M
    refused = []
    for n in D.POOL_N:
        for k, s in D.POOL_KS:
            want = _torch_pool_shape(n, k, s)
            if want is None:
                assert n < k, (n, k, s)
                want = 1
                refused.append((n, k, s))
            assert M.pool_out(n, k, s) == want and D.pool_outputs(n, k, s) == want, (n, k, s)
    assert refused == [(1, 2, 1), (1, 3, 1), (1, 3, 2), (2, 3, 1)]       # ceil((n - k) / s) + 1 < 1; torch accepts the other n < k


def test_pool_reference_is_torch_max_pool2d():
    cases = D.pool_cases()
    assert len(cases) == 13 * 13 * 6
    for h, w, k, s in cases:
        x = D.pool_inputs(h, w, k, s)
        assert (x[0] < 0).all() and (x[2] < 0).all() and np.isinf(x[2]).any() and x.shape == (D.POOL_PLANES, h, w)
        ref = D.pool_reference(x, k, s)
        ph, pw = max(h, k), max(w, k)                    # torch refuses inputs below the window: pad with -inf, which no maximum sees
        xp = np.full((x.shape[0], ph, pw), -np.inf)
        xp[:, :h, :w] = x
        want = F.max_pool2d(torch.from_numpy(xp)[None], k, s, ceil_mode=True)[0].numpy()[:, :ref.shape[1], :ref.shape[2]]
        assert ref.shape == (x.shape[0], D.pool_outputs(h, k, s), D.pool_outputs(w, k, s))
        MC.same_bits(f"pool {(h, w, k, s)}", ref, want.astype(np.float32))


@pytest.mark.parametrize("hw", D.SM_HW)
def test_softmax_reference_is_torch_softmax(hw):
    x = D.sm_inputs(hw)
    ref, bound, bar, emu = D.sm_bound(x)
    want = torch.softmax(torch.from_numpy(x.astype(np.float64)), dim=1)[:, 1].numpy()
    assert ref.shape == (D.SM_BATCH, hw)
    assert (np.abs(ref - want) <= 4 * 2.0 ** -53 * ref + 1e-320).all()
    assert 2.0 <= bar <= 6.0 and emu < 2.0, (bar, emu)               # the fp32 formula itself is good to under 2 ulp of p1
    d = (x[:, 1].astype(np.float64) - x[:, 0]).reshape(-1)
    if hw >= 255:                                                    # the whole sweep, at all three offsets
        for v in D.SM_DELTAS:
            for sign in (1, -1):
                assert (np.abs(d - sign * v) <= max(1e-3, 1e-6 * v)).any(), (v, sign)
        assert (x[:, 0] == np.float32(1e4)).any() and (x[:, 0] == np.float32(-1e4)).any()
        assert (ref < 2.0 ** -150).any() and (ref == 1).any() and ((ref > 0) & (ref < 2.0 ** -126)).any()


# ---- the conditions on the inputs ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", D.SM_HW)
def test_softmax_undecided_share(hw):
    x = D.sm_inputs(hw)
    ref, bound, _, _ = D.sm_bound(x)
    for ti in (0, 1):
        _, r, decided = D.decisions(ref.astype(np.float32), ref, bound, ti)
        assert (~decided).mean() <= D.UNDECIDED_CAP, (hw, ti, int((~decided).sum()))
        if hw >= 255:
            assert r.any() and not r.all()


@pytest.mark.parametrize("case", NMS, ids=lambda c: c.name)
def test_nms_undecided_share_and_recipe(case):
    boxes, image, scores = D.nms_inputs(case)
    assert boxes.shape == (case.n, 4) and boxes.dtype == np.float32 and (np.diff(scores) <= 0).all()
    bad, pairs = D.nms_undecided(case, boxes, image)
    assert bad <= D.UNDECIDED_CAP * max(pairs, 1), (bad, pairs)
    mask = D.nms_mask_fp32(case, boxes, image)
    assert mask.shape == (case.n, case.words) and D.left_of_diagonal_zero(mask)
    if case.n >= 63:
        o = D._nms_overlap(boxes, case.plus_one, case.method == "Min", np.float64)
        near = np.array([o[10 + 2 * q, 11 + 2 * q] for q in range(5)]) - case.thr
        assert (np.abs(near) <= 8 * 2.0 ** -24).all() and (near > 0).any() and (near < 0).any(), near      # within a few ulp, both sides
        assert (boxes[2] == boxes[3]).all() and boxes[5, 0] == boxes[5, 2] and boxes[8, 0] == boxes[7, 2]
        assert np.isnan(o[5, 6]) == (not case.plus_one)
        bits = D.nms_bits(boxes, image if case.with_image else None, case.thr, case.method, case.plus_one)
        assert bits[2, 3] and not bits[7, 8] and bits.any(1).sum() > 5      # the duplicate goes, the touching neighbour stays
        kept = D.host_scan(mask)
        assert 0 < kept.size < case.n


def test_host_scan_keeps_what_batched_nms_keeps():
    """The greedy scan over the fp32 restatement of the mask against mtcnn._batched_nms on the same boxes."""
    from faceposegenerator_amd import mtcnn as M
    for case in NMS:
        boxes, image, scores = D.nms_inputs(case)
        idxs = image if case.with_image else np.zeros(case.n, np.int32)
        want = M._batched_nms(boxes, scores, idxs, case.thr, case.method, case.plus_one)
        got = D.bnms_order(D.host_scan(D.nms_mask_fp32(case, boxes, image)), idxs, scores)
        assert np.array_equal(got, want), case.name


# ---- teeth ---------------------------------------------------------------------------------------------------------------------------
def test_defect_list_is_complete():
    assert set(D.DEFECT_CASES) == set(D.DEFECTS) - set(D.HARMLESS) and len(D.DEFECTS) == 16 and D.HARMLESS == ("prelu_gt",)


@pytest.mark.parametrize("defect", [d for d in D.DEFECTS if d not in D.HARMLESS])
def test_every_defect_fails_its_named_case(defect):
    assert D.defect_fails(defect), (defect, D.DEFECT_CASES[defect])


def test_harmless_defect_changes_no_value():
    for case in CONV:
        args = D.conv_inputs(case)
        a, b = D.conv_reference(*args)[0], D.conv_reference(*args, defect="prelu_gt")[0]
        assert np.array_equal(a, b), case.name
    x = np.zeros((1, 1, 3, 3), np.float32)                            # an accumulator of exactly 0: 0 * slope is 0
    a, b = (D.conv_reference(x, x[:, :, :2, :2] + 1, None, np.float32([0.25]), defect=d)[0] for d in (None, "prelu_gt"))
    assert np.array_equal(a, b) and (a == 0).all()


def test_fp32_emulations_pass_every_case():
    worst = {"area": 0.0, "conv": 0.0}
    for case in AREA:
        img = D.area_images()[case.image]
        ref, bound = D.area_reference(img, case)
        res = D.check(D.emulate_area(img, case), ref, bound)
        assert res[0], D.describe(case.name, res)
        worst["area"] = max(worst["area"], res[1])
    for case in CONV:
        args = D.conv_inputs(case)
        ref, bound, _ = D.conv_reference(*args)
        res = D.check(D.emulate_conv(*args), ref, bound)
        assert res[0], D.describe(case.name, res)
        worst["conv"] = max(worst["conv"], res[1])
    for hw in D.SM_HW:
        x = D.sm_inputs(hw)
        ref, bound, _, _ = D.sm_bound(x)
        got = D.emulate_softmax(x)
        res = D.check(got, ref, bound)
        assert res[0], D.describe(f"softmax hw {hw}", res)
        for ti in (0, 1):
            g, r, decided = D.decisions(got, ref, bound, ti)
            assert (g == r)[decided].all()
    print(f"detect matrix, fp32 emulation, worst err / bound: area {worst['area']:.3f}, conv {worst['conv']:.3f}")


# ---- argument checks: every IDB_REQUIRE of idb_mtcnn.hip answers before any HIP call -------------------------------------------------
P = MC.P16


def test_area_argument_checks(lib):
    f = lib.idb_crop_resize_area_u8
    ok = dict(src=P, batch=2, h=61, w=45, c=3, boxes=P, n=2, out=P, oh=24, ow=24)
    call = lambda a: f(a["src"], a["batch"], a["h"], a["w"], a["c"], a["boxes"], a["n"], a["out"], a["oh"], a["ow"], 127.5, 0.0078125, None)   # noqa: E731
    assert call({**ok, "n": 0}) == 0                                   # nothing to do: OK, no launch
    MC.refused(lib, call, ok, (dict(src=None), dict(boxes=None), dict(out=None), dict(batch=0), dict(h=0), dict(w=0), dict(c=0), dict(n=-1), dict(oh=0),
                               dict(ow=0), dict(h=-3), dict(src=None, n=0)), "idb_crop_resize_area_u8: bad arguments")
    MC.refused(lib, call, ok, (dict(h=1 << 16, w=1 << 15), dict(n=(1 << 28) + 1)), "idb_crop_resize_area_u8: image plane or box count too large")
    MC.refused(lib, call, ok, (dict(n=1 << 28, c=4, oh=1024, ow=1024),), "idb_crop_resize_area_u8: too many outputs")


def test_conv_argument_checks(lib):
    f = lib.idb_conv2d_f32
    ok = dict(x=P, w=P, bias=None, slope=None, y=P, batch=2, cin=3, h=5, w_=7, cout=4, kh=3, kw=3)
    call = lambda a: f(a["x"], a["w"], a["bias"], a["slope"], a["y"], a["batch"], a["cin"], a["h"], a["w_"], a["cout"], a["kh"], a["kw"], None)   # noqa: E731
    MC.refused(lib, call, ok, (dict(x=None), dict(w=None), dict(y=None), dict(batch=0), dict(cin=0), dict(cout=0), dict(kh=0), dict(kw=0), dict(h=2),
                               dict(w_=2), dict(h=0), dict(batch=-1)), "idb_conv2d_f32: bad arguments")
    MC.refused(lib, call, ok, (dict(h=1 << 16, w_=1 << 15, kh=1, kw=1), dict(cin=1 << 20, h=64, w_=64, kh=64, kw=32)), "idb_conv2d_f32: plane or filter too large")
    MC.refused(lib, call, ok, (dict(batch=1 << 20, cout=1 << 20, h=32, w_=32, kh=1, kw=1),), "idb_conv2d_f32: too many outputs")


def test_pool_argument_checks(lib):
    f = lib.idb_maxpool2d_f32
    ok = dict(x=P, y=P, planes=4, h=9, w=9, k=3, s=2)
    call = lambda a: f(a["x"], a["y"], a["planes"], a["h"], a["w"], a["k"], a["s"], None)   # noqa: E731
    MC.refused(lib, call, ok, (dict(x=None), dict(y=None), dict(planes=0), dict(h=0), dict(w=0), dict(k=0), dict(s=0), dict(k=-2)), "idb_maxpool2d_f32: bad arguments")
    MC.refused(lib, call, ok, (dict(h=1 << 16, w=1 << 15), dict(h=(1 << 30) + 1, w=1), dict(h=1, w=(1 << 30) + 1), dict(k=(1 << 20) + 1), dict(s=(1 << 20) + 1)),
               "idb_maxpool2d_f32: plane, window or stride too large")
    MC.refused(lib, call, ok, (dict(planes=1 << 30, h=1 << 10, w=1 << 10, k=1, s=1),), "idb_maxpool2d_f32: too many outputs")


def test_softmax_pairs_argument_checks(lib):
    ok = dict(x=P, y=P, b=3, hw=5)
    call = lambda a: lib.idb_softmax_pairs_f32(a["x"], a["y"], a["b"], a["hw"], None)   # noqa: E731
    MC.refused(lib, call, ok, (dict(x=None), dict(y=None), dict(b=0), dict(hw=0), dict(b=-1)), "idb_softmax_pairs_f32: bad arguments")
    MC.refused(lib, call, ok, (dict(b=1 << 30, hw=1 << 30),), "idb_softmax_pairs_f32: too many outputs")


def test_nms_mask_argument_checks(lib):
    ok = dict(boxes=P, image=P, n=5, mask=P)
    call = lambda a: lib.idb_nms_mask(a["boxes"], a["image"], a["n"], 0.5, 0, 0, a["mask"], None)   # noqa: E731
    MC.refused(lib, call, ok, (dict(boxes=None), dict(mask=None), dict(image=None, n=0), dict(n=-1), dict(n=(1 << 20) + 1)), "idb_nms_mask: bad arguments")
