"""The FR-training input stage without a GPU: the integer / float32 restatements that csrc/idb_augment.hip transcribes equal Pillow
itself, image for image (tests/randaug_oracle.py parts (b) and (a)); ``plan()`` reproduces the reference's draws from private
generators; the magnitude tables, the host's fixed-point matrices, the policy names and idb_randaug's argument checks."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import randaug_oracle as R  # noqa: E402

from faceposegenerator_amd import augment as A  # noqa: E402

SIZES = [(112, 112), (24, 40), (33, 17)]                         # (h, w)


def _images(h, w):
    """uniform-random, narrow-range, constant, and one with a single constant channel (the identity branches of AutoContrast / Equalize)"""
    u = np.random.default_rng(h * 1000 + w).integers(0, 256, (h, w, 3), dtype=np.uint8)
    one = u.copy()
    one[..., 2] = 9
    return {"uniform": u, "narrow": (u // 3 + 40).astype(np.uint8), "constant": np.full_like(u, 77), "one-constant-channel": one}


def _first_diff(got, ref):
    d = np.argwhere(got != ref)
    if len(d) == 0:
        return "shape" if got.shape != ref.shape else "none"
    y, x, c = (int(v) for v in d[0])
    return f"{len(d)} bytes differ, first at (y={y}, x={x}, c={c}): got {got[y, x, c]} ref {ref[y, x, c]}"


@pytest.mark.parametrize("op", A.OPS)
def test_restatement_equals_pillow(op):
    signed = op in A.SIGNED
    scalar = op in ("Identity", "AutoContrast", "Equalize", "Grayscale")
    for h, w in SIZES:
        for kind, x in _images(h, w).items():
            for b in ([1] if scalar else range(1, 31)):
                for neg in ((False, True) if signed else (False,)):
                    m = R.magnitude_of(op, b, neg, w)
                    ref, got = R.pil_op(x, op, m), R.np_op(x, op, m)
                    assert np.array_equal(got, ref), f"{op} bin {b} neg {neg} {h}x{w} {kind}: {_first_diff(got, ref)}"


def test_flip_restatement_equals_pillow():
    for h, w in SIZES:
        for x in _images(h, w).values():
            assert np.array_equal(R.np_flip(x), R.pil_flip(x))


def test_autocontrast_lut_for_every_lo_hi_pair():
    """The oracle's LUT equals ImageOps.autocontrast on a two-value image for all 32 640 pairs lo < hi (the double arithmetic the
    kernel repeats: scale = 255 / (hi - lo), offset = -lo scale, int(i scale + offset) clipped)."""
    from PIL import Image, ImageOps
    ramp = np.arange(256, dtype=np.uint8)
    for lo in range(0, 255, 17):                                  # Pillow itself on a sample of pairs: the LUT is applied to lo..hi
        for hi in range(lo + 1, 256, 13):
            x = np.clip(ramp, lo, hi).reshape(16, 16)
            ref = np.array(ImageOps.autocontrast(Image.fromarray(x)))
            assert np.array_equal(R.autocontrast_lut(lo, hi)[x], ref), (lo, hi)
    for lo in range(255):                                         # every pair: ends pinned, monotone
        for hi in range(lo + 1, 256):
            lut = R.autocontrast_lut(lo, hi)
            assert lut[lo] == 0 and lut[hi] >= 254 and np.all(np.diff(lut.astype(np.int32)) >= 0), (lo, hi)


@pytest.mark.parametrize("num_ops,magnitude", [(4, 16), (2, 9), (1, 9)])
@pytest.mark.parametrize("flip_p", [0.5, None])
def test_plan_reproduces_the_reference_draws(num_ops, magnitude, flip_p):
    n, seed = 24, 1234 + num_ops
    x = np.random.default_rng(0).integers(0, 256, (n, 16, 16, 3), dtype=np.uint8)
    t_state, n_state = torch.get_rng_state(), np.random.get_state()
    try:
        torch.manual_seed(seed)
        np.random.seed(seed)
        _, _, flips, trace = R.chain(x, num_ops, magnitude, flip_p)
    finally:
        torch.set_rng_state(t_state)
        np.random.set_state(n_state)
    before_t, before_n = torch.get_rng_state().clone(), np.random.get_state()
    plan = A.RandAugment(num_ops, magnitude).plan(n, torch.Generator().manual_seed(seed), np.random.RandomState(seed), flip_p)
    assert torch.equal(torch.get_rng_state(), before_t)
    after_n = np.random.get_state()
    assert before_n[0] == after_n[0] and np.array_equal(before_n[1], after_n[1]) and before_n[2:] == after_n[2:]
    assert plan.flip.shape == (n,) and plan.op.shape == plan.bin.shape == plan.neg.shape == (n, num_ops)
    assert plan.flip.tolist() == (flips if flip_p is not None else [False] * n)
    assert [tuple(t) for t in zip(plan.op.reshape(-1).tolist(), plan.bin.reshape(-1).tolist(), plan.neg.reshape(-1).tolist())] == trace
    assert 1 <= plan.bin.min() and plan.bin.max() <= magnitude
    assert not plan.neg[~np.isin(plan.op, [A.OPS.index(o) for o in A.SIGNED])].any()


def test_tables_known_answers():
    assert A.OPS == R.OPS == list(R.augmentation_space(31, [112, 112]).keys())
    assert A.SIGNED == ("ShearX", "TranslateX", "Rotate", "Brightness", "Color", "Contrast", "Sharpness")
    t = A.magnitude_tables(112)
    ref = R.augmentation_space(31, [112, 64])
    assert list(t) == A.OPS
    for k in A.OPS:
        assert torch.equal(t[k][0], ref[k][0]) and t[k][1] == ref[k][1] == (k in A.SIGNED)
    assert int(t["Posterize"][0][16]) == 6
    assert float(t["Solarize"][0][16]) == 119.0
    assert int(float(t["TranslateX"][0][16])) == 27
    assert float(t["Rotate"][0][30]) == 30.0 and t["Identity"][0].ndim == 0


def test_host_fixed_point_matrices_equal_the_oracle():
    for h, w in SIZES + [(128, 128), (8, 8)]:
        ia, fa = A.slot_tables(h, w)
        assert ia.shape == (13, 31, 2, 6) and ia.dtype == np.int32 and fa.shape == (13, 31, 2) and fa.dtype == np.float32
        for o, op in enumerate(A.OPS):
            for b in range(1, 31):
                for s in range(2):
                    m = R.magnitude_of(op, b, bool(s), w)
                    if op in ("ShearX", "TranslateX", "Rotate"):
                        want = R.fixed_affine(R.geometry_matrix(op, m, w, h))
                        assert ia[o, b, s].tolist() == want == A.affine_fixed(op, m, w, h), (op, b, s, h, w)
                    elif op in ("Brightness", "Color", "Contrast", "Sharpness"):
                        assert fa[o, b, s] == np.float32(1.0 + m)
                    elif op == "Posterize":
                        assert ia[o, b, s, 0] == (0xFF << (8 - int(m))) & 0xFF and ia[o, b, s, 1:].tolist() == [0] * 5
                    elif op == "Solarize":
                        assert fa[o, b, s] == np.float32(m) and float(fa[o, b, s]) == m
                    else:
                        assert not ia[o, b, s].any() and fa[o, b, s] == 0
    plan = A.make_plan([0, 1], [[1, 9], [4, 0]], [[3, 16], [30, 1]], [[True, False], [False, False]])
    sop, sia, sfa = A.slot_args(plan, 24, 40)
    ia, fa = A.slot_tables(24, 40)
    assert sop.tolist() == [[1, 9], [4, 0]] and sia.shape == (2, 2, 6) and sfa.shape == (2, 2)
    assert sia[0, 0].tolist() == ia[1, 3, 1].tolist() and sfa[0, 1] == fa[9, 16, 0] == np.float32(119.0) and sfa[1, 0] == fa[4, 30, 0]


def test_policy_names():
    def shape(t):
        return (t.flip_p, t.randaug.num_ops, t.randaug.magnitude)
    for name in ("hf", "GAN_HF", "nogan_hf"):
        assert shape(A.get_conventional_aug_policy(name))[:2] == (0.5, 0)
    for name in ("ra_4_16", "gan_ra_4_16", "NoGAN_RA_4_16"):
        assert shape(A.get_conventional_aug_policy(name)) == (0.5, 4, 16)
    assert shape(A.get_conventional_aug_policy("num_mag_exp", num_ops=2, mag=9)) == (0.5, 2, 9)
    assert shape(A.get_conventional_aug_policy("aug_operation_exp", operation="Rotate")) == (0.5, 1, 9)
    assert shape(A.get_conventional_aug_policy("totensor"))[:2] == (None, 0)
    for name in ("moco", "faa_casia", "faa_imgnet", "mag_totensor", "nonsense"):
        with pytest.raises(ValueError, match="ra_4_16"):
            A.get_conventional_aug_policy(name)


def test_apply_refuses_bad_batches_before_the_library():
    plan = A.make_plan([0], np.zeros((1, 0)), np.zeros((1, 0)))
    for bad in (np.zeros((1, 129, 128, 3), np.uint8), np.zeros((1, 16, 16, 3), np.float32), np.zeros((1, 16, 16, 4), np.uint8),
                np.zeros((1, 4, 16, 3), np.uint8), torch.zeros((1, 16, 3, 16), dtype=torch.uint8).permute(0, 1, 3, 2)):
        with pytest.raises(ValueError):
            A.apply(bad, plan)
    with pytest.raises(ValueError):
        A.apply(np.zeros((2, 16, 16, 3), np.uint8), plan)
    with pytest.raises(ValueError):
        A.make_plan([0], [[13]], [[1]])


def test_invalid_arguments_are_rejected_without_gpu(lib):
    # argument validation happens before any HIP call, so it is testable on CPU (any non-null address will do)
    p = 0x1000
    assert lib.idb_randaug(p, 1, 129, 128, p, p, p, p, 1, p, p, None) == -2
    assert b"49152" in lib.idb_last_error()
    assert lib.idb_randaug(p, 1, 112, 112, p, p, p, p, -1, p, p, None) == -1
    assert b"num_ops" in lib.idb_last_error()
    assert lib.idb_randaug(p, 1, 112, 112, p, p, p, p, 1, None, None, None) == -1
    assert b"no output" in lib.idb_last_error()
    assert lib.idb_randaug(p, 1, 7, 112, p, p, p, p, 1, p, p, None) == -1
    assert b">= 8" in lib.idb_last_error()
    assert lib.idb_randaug(p, 1, 112, 112, p, None, p, p, 1, p, p, None) == -1
    assert lib.idb_randaug(None, 1, 112, 112, p, p, p, p, 1, p, p, None) == -1
    assert lib.idb_randaug(p, 0, 112, 112, p, p, p, p, 1, p, p, None) == -1
