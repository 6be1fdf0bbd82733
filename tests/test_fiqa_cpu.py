"""CR-FIQA host side (no GPU): the resize tables and the integer restatement of tests/fiqa_oracle.py against their known answers and
against unrounded float64 bilinear interpolation, the weight layout, the script's and the notebook's host policy, and the argument
checks of the two new C entry points."""
import os
import random
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fiqa_oracle as Q  # noqa: E402

from faceposegenerator_amd import arcface as A  # noqa: E402
from faceposegenerator_amd import fiqa as F  # noqa: E402

# (H, W, dh, dw): identity, both axes shrinking, enlarging, the workload, a squashed non-square image, the 2x box, one pixel, two rows
SHAPES = [(7, 7, 7, 7), (5, 9, 3, 4), (13, 11, 112, 112), (512, 512, 112, 112), (200, 300, 112, 112), (8, 8, 4, 4), (1, 1, 3, 3),
          (2, 3, 112, 112)]


def _images(H, W, B=2, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (B, H, W, 3), dtype=np.uint8)


# ---- resize tables and oracle ------------------------------------------------------------------------------------------------------
def test_coef_tables_known_answer():
    o, c = F.coef_tables(6, 4)
    assert o.dtype == np.int32 and c.dtype == np.int16
    assert o.tolist() == [0, 1, 3, 4]
    assert c.tolist() == [[1536, 512], [512, 1536], [1536, 512], [512, 1536]]


@pytest.mark.parametrize("H,W,dh,dw", SHAPES)
def test_coef_tables_invariants_and_oracle_tables(H, W, dh, dw):
    for s, d in ((H, dh), (W, dw), (112, 512), (3, 1000)):
        o, c = F.coef_tables(s, d)
        assert o.shape == (d,) and c.shape == (d, 2)
        assert (c.astype(np.int64).sum(axis=1) == 2048).all()
        assert o.min() >= 0 and o.max() <= s - 1
        assert (c[o == s - 1, 1] == 0).all()                    # the clamped second tap carries no weight
        oo, oc = Q.coef_table(s, d)
        assert np.array_equal(o, oo) and np.array_equal(c, oc)


def test_coef_tables_refuse_empty_axes():
    with pytest.raises(ValueError):
        F.coef_tables(0, 4)
    with pytest.raises(ValueError):
        F.coef_tables(4, 0)


def test_oracle_known_answers():
    for H, W in ((7, 7), (1, 1), (5, 9)):
        x = _images(H, W)
        assert np.array_equal(Q.resize(x, H, W), x)                                      # identity sizes return the source
    for H, W, dh, dw in SHAPES:
        assert (Q.resize(np.full((1, H, W, 3), 255, np.uint8), dh, dw) == 255).all()    # a constant image stays constant
    row = np.array([0, 0, 0, 200, 200, 200], np.uint8)[None, None, :, None].repeat(3, axis=3)
    assert Q.resize(row, 1, 4)[0, 0, :, 0].tolist() == [0, 0, 200, 200]
    # the 2x2 box rule (a + b + c + d + 2) >> 2 on a hand-written block: (1 + 2 + 3 + 5 + 2) >> 2 = 3, (255 + 255 + 255 + 254 + 2) >> 2 = 255,
    # (0 + 0 + 0 + 1 + 2) >> 2 = 0, (0 + 1 + 1 + 0 + 2) >> 2 = 1
    x = np.zeros((1, 8, 8, 3), np.uint8)
    x[0, 0:2, 0:2, 0] = [[1, 2], [3, 5]]
    x[0, 0:2, 2:4, 0] = [[255, 255], [255, 254]]
    x[0, 2:4, 0:2, 0] = [[0, 0], [0, 1]]
    x[0, 2:4, 2:4, 0] = [[0, 1], [1, 0]]
    y = Q.resize(x, 4, 4)
    assert y.shape == (1, 4, 4, 3) and y[0, 0:2, 0:2, 0].tolist() == [[3, 255], [0, 1]] and not y[..., 1:].any()


@pytest.mark.parametrize("H,W,dh,dw", SHAPES)
def test_oracle_is_within_one_grey_level_of_float64_bilinear(H, W, dh, dw):
    x = _images(H, W)
    y = Q.resize(x, dh, dw).astype(np.float64)
    if H == 2 * dh and W == 2 * dw:                     # the box path is no bilinear interpolation at these centres' rounding: compare the mean
        box = x.astype(np.float64).reshape(2, dh, 2, dw, 2, 3).mean(axis=(2, 4))
        err = np.abs(y - box).max()
        print(f"{H}x{W} -> {dh}x{dw}: max |oracle - box mean| = {err:.4f}")
        assert err <= 0.5
        return
    err = np.abs(y - Q.bilinear_f64(x, dh, dw)).max()
    print(f"{H}x{W} -> {dh}x{dw}: max |oracle - float64 bilinear| = {err:.4f}")
    assert err < 1.0


# ---- weights -----------------------------------------------------------------------------------------------------------------------
def test_param_shapes_add_exactly_the_quality_head():
    for arch in ("r18", "r50", "r100"):
        a, q = A.param_shapes(arch), F.param_shapes(arch)
        assert list(q)[:len(a)] == list(a) and all(q[k] == a[k] for k in a)
        assert {k: q[k] for k in q if k not in a} == {"qs.weight": (1, 512), "qs.bias": (1,)}
    with pytest.raises(ValueError):
        F.param_shapes("r200")


def test_state_dict_checks():
    sd = F.synth_weights("r18", 0)
    assert sd["qs.weight"].shape == (1, 512) and abs(sd["qs.bias"].item() - 2.0) < 0.5
    F.check_state_dict(sd, "r18")
    with pytest.raises(ValueError, match="qs"):
        F.FaceQuality.from_state_dict({k: v for k, v in sd.items() if not k.startswith("qs.")}, "r18")
    se = dict(sd)
    se["layer1.0.se_block.fc1.weight"] = torch.zeros(4, 64, 1, 1)
    with pytest.raises(ValueError, match="se_block"):
        F.FaceQuality.from_state_dict(se, "r18")
    fw = F.fold_weights(sd, "r18")
    assert fw["qs.w"].shape == (512,) and fw["qs.b"].shape == (1,) and fw["qs.w"].dtype == torch.float32
    assert set(fw) - {"qs.w", "qs.b"} == set(A.fold_weights({k: v for k, v in sd.items() if not k.startswith("qs.")}, "r18"))


def test_network_refuses_the_cpu_and_a_call_before_placement():
    m = F.FaceQuality.from_synthetic("r18")
    with pytest.raises(ValueError):
        m.to("cpu")
    with pytest.raises(RuntimeError):
        m.get_batch_feature(np.zeros((1, 4, 4, 3), np.uint8))


# ---- host policy -------------------------------------------------------------------------------------------------------------------
def test_natural_keys_sort():
    names = ["10.png", "2.png", "1_b.png", "1_a.png"]
    assert sorted(names, key=F.natural_keys) == ["1_a.png", "1_b.png", "2.png", "10.png"]
    assert F.natural_keys("img12_3.png") == ["img", 12, "_", 3, ".png"]


def test_list_images_is_listdir_in_natural_order(tmp_path):
    for n in ("10.png", "2.png", "1_b.png", "1_a.png"):
        (tmp_path / n).write_bytes(b"")
    assert F.list_images(str(tmp_path)) == [os.path.join(str(tmp_path), n) for n in ("1_a.png", "1_b.png", "2.png", "10.png")]


def test_sample_paths_reproduces_the_seeded_draw_and_leaves_the_global_state():
    names = [f"{i}.png" for i in range(25)]
    state = random.getstate()
    try:
        random.seed(7)
        want = random.sample(names, 10)
    finally:
        random.setstate(state)
    assert F.sample_paths(names, n=10, seed=7) == want
    assert random.getstate() == state
    assert F.sample_paths(names[:10], n=10) == names[:10] and F.sample_paths(names[:3], n=10) == names[:3]
    assert F.sample_paths(names) == names                                                # the default n = 10000
    assert random.getstate() == state


def test_scores_round_trip(tmp_path):
    q = np.array([[2.1234567], [1.0], [0.1], [-3.5e-7], [2.0000002]], dtype=np.float32)
    paths = [f"/data/set/{i}.png" for i in range(5)]
    out = str(tmp_path / "scores.txt")
    F.write_scores(out, paths, torch.from_numpy(q))
    lines = open(out).read().split("\n")
    assert lines[-1] == "" and lines[:-1] == [p + " " + str(s) for p, s in zip(paths, q[:, 0])]
    got = F.read_scores(out)
    assert got == [float(str(s)) for s in q[:, 0]]
    assert np.array_equal(np.asarray(got, dtype=np.float32), q[:, 0])                    # str(np.float32) round-trips the value
    with pytest.raises(ValueError):
        F.write_scores(out, paths[:2], q)


def test_quality_summary_matches_pandas():
    import pandas as pd
    for seed, n in ((0, 1000), (1, 7), (2, 2)):
        v = (2.1 + 0.15 * np.random.default_rng(seed).standard_normal(n)).astype(np.float32).astype(np.float64).tolist()
        df = pd.DataFrame({"score": v})
        want = {"mean": float(np.round(df["score"].mean(), 3)), "std": float(np.round(df["score"].std(), 3))}
        assert F.quality_summary(v) == want
    one = F.quality_summary([2.5])
    assert one["mean"] == 2.5 and np.isnan(one["std"]) and np.isnan(pd.DataFrame({"s": [2.5]})["s"].std())


def test_load_image_rgb_decodes_png_exactly(tmp_path):
    from PIL import Image
    x = _images(5, 7, B=1)[0]
    Image.fromarray(x).save(str(tmp_path / "a.png"))
    assert np.array_equal(F.load_image_rgb(str(tmp_path / "a.png")), x)
    Image.fromarray(x[..., 0]).save(str(tmp_path / "g.png"))                             # greyscale -> three equal channels
    assert np.array_equal(F.load_image_rgb(str(tmp_path / "g.png")), x[..., :1].repeat(3, axis=2))


# ---- ABI ---------------------------------------------------------------------------------------------------------------------------
def test_library_refuses_bad_arguments_before_any_hip_call(lib):
    p = 0x1000
    assert lib.idb_resize_linear_u8(None, 1, 8, 8, p, p, p, p, 4, 4, 0, p, None) == -1
    assert b"null" in lib.idb_last_error()
    assert lib.idb_resize_linear_u8(p, 1, 8, 8, p, None, p, p, 4, 4, 0, p, None) == -1
    assert b"null" in lib.idb_last_error()
    assert lib.idb_resize_linear_u8(p, 1, 8, 8, p, p + 2, p, p, 4, 4, 0, p, None) == -1
    assert b"aligned" in lib.idb_last_error()
    for b, h, w, dh, dw in ((0, 8, 8, 4, 4), (65536, 8, 8, 4, 4), (1, 0, 8, 4, 4), (1, 8, 0, 4, 4), (1, 8, 8, 0, 4), (1, 8, 8, 4, 0),
                            (1, 32769, 8, 4, 4), (1, 8, 8, 4, 32769)):
        assert lib.idb_resize_linear_u8(p, b, h, w, p, p, p, p, dh, dw, 1, p, None) == -1
        assert b"32768" in lib.idb_last_error()
    assert lib.idb_fiqa_tail(p, None, p, 4, 512, p, p, None) == -1
    assert b"null" in lib.idb_last_error()
    assert lib.idb_fiqa_tail(p, p, p, 4, 512, p, None, None) == -1
    assert lib.idb_fiqa_tail(p, p + 1, p, 4, 512, p, p, None) == -1
    assert b"unaligned" in lib.idb_last_error()
    for b, d in ((0, 512), ((1 << 30) + 1, 512), (4, 0), (4, 8193)):
        assert lib.idb_fiqa_tail(p, p, p, b, d, p, p, None) == -1
        assert b"8192" in lib.idb_last_error()
