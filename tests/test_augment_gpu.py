"""The FR-training input stage on the MI355X: idb_randaug against Pillow itself (tests/randaug_oracle.py part (a)).  Every comparison
is array_equal / torch.equal: there is no tolerance anywhere."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import randaug_oracle as R  # noqa: E402

from faceposegenerator_amd import augment as A  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = [(112, 112), (24, 40), (33, 17), (128, 128), (8, 8)]     # (h, w)


def _special(h, w, seed=0):
    """uniform-random, narrow-range, constant, one constant channel"""
    u = np.random.default_rng(seed + h * 1000 + w).integers(0, 256, (h, w, 3), dtype=np.uint8)
    one = u.copy()
    one[..., 2] = 9
    return [u, (u // 3 + 40).astype(np.uint8), np.full_like(u, 77), one]


def _cases():
    """(op index, bin, neg) for every op, bin 1..30 and, for the signed ops, both signs"""
    out = []
    for o, name in enumerate(A.OPS):
        for b in range(1, 31):
            for neg in ((False, True) if name in A.SIGNED else (False,)):
                out.append((o, b, neg))
    return out


def _report(got, ref, cases):
    """'' if equal, else op, bin, sign and the first differing pixel of the first differing image"""
    if got.shape != ref.shape:
        return f"shape {got.shape} vs {ref.shape}"
    bad = np.nonzero((got != ref).reshape(got.shape[0], -1).any(axis=1))[0]
    if len(bad) == 0:
        return ""
    i = int(bad[0])
    y, x, c = (int(v) for v in np.argwhere(got[i] != ref[i])[0])
    o, b, neg = cases[i]
    return (f"{len(bad)} of {got.shape[0]} images differ; first: image {i} op {A.OPS[o]} bin {b} neg {neg}, pixel (y={y}, x={x}, c={c}) "
            f"got {got[i, y, x, c]} ref {ref[i, y, x, c]}")


@pytest.mark.parametrize("h,w", SIZES)
def test_every_op_bin_and_sign_equals_pillow(lib, h, w):
    cases = _cases()
    base = _special(h, w)[:2]
    pick = np.random.default_rng(1).integers(0, 2, len(cases))
    x = np.stack([base[k] for k in pick])
    plan = A.make_plan(np.zeros(len(cases)), [[c[0]] for c in cases], [[c[1]] for c in cases], [[c[2]] for c in cases])
    ref = np.stack([R.pil_op(x[i], A.OPS[o], R.magnitude_of(A.OPS[o], b, neg, w)) for i, (o, b, neg) in enumerate(cases)])
    got = A.apply(x, plan, "u8", device=DEV)
    assert got.dtype == torch.uint8 and tuple(got.shape) == x.shape and got.is_cuda
    msg = _report(got.cpu().numpy(), ref, cases)
    assert not msg, f"{h}x{w}: {msg}"


@pytest.mark.parametrize("op", ["AutoContrast", "Equalize", "Contrast"])
def test_special_images(lib, op):
    o = A.OPS.index(op)
    for h, w in [(112, 112), (33, 17)]:
        imgs = _special(h, w, seed=5)
        cases = [(o, 7, bool(i & 1)) if op in A.SIGNED else (o, 7, False) for i in range(len(imgs))]
        plan = A.make_plan(np.zeros(len(imgs)), [[c[0]] for c in cases], [[c[1]] for c in cases], [[c[2]] for c in cases])
        ref = np.stack([R.pil_op(im, op, R.magnitude_of(op, b, neg, w)) for im, (_, b, neg) in zip(imgs, cases)])
        got = A.apply(np.stack(imgs), plan, "u8", device=DEV).cpu().numpy()
        msg = _report(got, ref, cases)
        assert not msg, f"{op} {h}x{w}: {msg}"


def test_flip_alone(lib):
    for h, w in SIZES:
        x = np.stack(_special(h, w, seed=2))
        flip = np.array([1, 0, 1, 1], bool)
        plan = A.make_plan(flip, np.zeros((4, 0)), np.zeros((4, 0)))
        ref = np.stack([R.pil_flip(im) if f else im for im, f in zip(x, flip)])
        u8, fl = A.apply(x, plan, "both", device=DEV)
        assert np.array_equal(u8.cpu().numpy(), ref), (h, w)
        want = torch.stack([R.to_tensor_normalize(im) for im in ref])
        assert torch.equal(fl.cpu(), want), (h, w)


def _seeded_chain(x, num_ops, magnitude, flip_p, seed):
    """the oracle chain on the global generators seeded with ``seed`` (restored afterwards)"""
    t_state, n_state = torch.get_rng_state(), np.random.get_state()
    try:
        torch.manual_seed(seed)
        np.random.seed(seed)
        return R.chain(x, num_ops, magnitude, flip_p)
    finally:
        torch.set_rng_state(t_state)
        np.random.set_state(n_state)


def test_ra_4_16_end_to_end(lib):
    n, seed = 64, 20
    x = np.random.default_rng(3).integers(0, 256, (n, 112, 112, 3), dtype=np.uint8)
    x[1::2] = x[1::2] // 2 + 30                                 # half of them narrow-range
    ref_u8, ref_f, _, trace = _seeded_chain(x, 4, 16, 0.5, seed)
    plan = A.RandAugment(4, 16).plan(n, torch.Generator().manual_seed(seed), np.random.RandomState(seed))
    cases = [trace[4 * i] for i in range(n)]
    x_before = x.copy()
    u8, fl = A.apply(x, plan, "both", device=DEV)
    assert u8.dtype == torch.uint8 and tuple(u8.shape) == (n, 112, 112, 3) and u8.device == torch.device(DEV)
    assert fl.dtype == torch.float32 and tuple(fl.shape) == (n, 3, 112, 112) and fl.device == torch.device(DEV)
    msg = _report(u8.cpu().numpy(), ref_u8, cases)
    assert not msg, f"chain {plan.op.tolist()}: {msg} (the op named is the first of the image's four)"
    assert torch.equal(fl.cpu(), ref_f)
    assert np.array_equal(x, x_before)
    # a device tensor gives the same, is left unchanged, and each single output equals its half of "both"
    xd = torch.from_numpy(x).to(DEV)
    u8d, fld = A.apply(xd, plan, "both")
    assert torch.equal(u8d, u8) and torch.equal(fld, fl) and torch.equal(xd.cpu(), torch.from_numpy(x_before))
    assert torch.equal(A.apply(xd, plan, "u8"), u8) and torch.equal(A.apply(torch.from_numpy(x), plan, "float", device=DEV), fl)
    # the policy's batch transform: same generators, same tensor
    t = A.get_conventional_aug_policy("ra_4_16")
    out = t(xd, torch.Generator().manual_seed(seed), np.random.RandomState(seed))
    assert out.dtype == torch.float32 and torch.equal(out, fl)


@pytest.mark.parametrize("num_ops", [0, 1, 4])
@pytest.mark.parametrize("n", [1, 300])
def test_num_ops_and_batch_sizes(lib, num_ops, n):
    h, w, seed = 24, 40, 100 + num_ops + n
    x = np.random.default_rng(n).integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    ref_u8, ref_f, _, _ = _seeded_chain(x, num_ops, 16, 0.5, seed)
    plan = A.RandAugment(num_ops, 16).plan(n, torch.Generator().manual_seed(seed), np.random.RandomState(seed))
    assert plan.num_ops == num_ops
    u8, fl = A.apply(x, plan, "both", device=DEV)
    assert np.array_equal(u8.cpu().numpy(), ref_u8) and torch.equal(fl.cpu(), ref_f)
    u8b, flb = A.apply(x, plan, "both", device=DEV)               # a second run: bit-identical
    assert torch.equal(u8b, u8) and torch.equal(flb, fl)


def test_refusals(lib):
    plan = A.make_plan([0], np.zeros((1, 0)), np.zeros((1, 0)))
    with pytest.raises(ValueError, match="49152"):
        A.apply(torch.zeros((1, 129, 128, 3), dtype=torch.uint8, device=DEV), plan)
    with pytest.raises(ValueError, match="uint8"):
        A.apply(torch.zeros((1, 16, 16, 3), dtype=torch.float32, device=DEV), plan)
    with pytest.raises(ValueError, match="contiguous"):
        A.apply(torch.zeros((1, 16, 3, 16), dtype=torch.uint8, device=DEV).permute(0, 1, 3, 2), plan)
    with pytest.raises(ValueError, match="uint8 RGB"):
        A.apply(torch.zeros((1, 16, 16, 4), dtype=torch.uint8, device=DEV), plan)
    x = torch.zeros((1, 129, 128, 3), dtype=torch.uint8, device=DEV)      # the library itself: unsupported, nothing launched
    o = torch.empty((1, 129, 128, 3), dtype=torch.uint8, device=DEV)
    assert lib.idb_randaug(x.data_ptr(), 1, 129, 128, None, None, None, None, 0, o.data_ptr(), None, None) == -2
