"""ArcFace IResNet on CPU: state-dict layout against the known answers, the strict loader, the exactness of the weight folding the
engine uploads (evaluated by plain torch in the engine's NHWC order, border ring and head separately), the stability of the synthetic
fixture, and the host-side refusals of the new idb_gemm descriptor fields (no GPU call is made)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import arcface_oracle as O  # noqa: E402

from faceposegenerator_amd import _lib  # noqa: E402
from faceposegenerator_amd import arcface as A  # noqa: E402


def _n_params(arch):
    return sum(int(np.prod(s)) for k, s in A.param_shapes(arch).items() if not k.endswith(("running_mean", "running_var", "num_batches_tracked")))


@pytest.mark.parametrize("arch,params,entries", [("r100", 65_156_160, 925), ("r50", 43_590_848, 475)])
def test_known_answers(arch, params, entries):
    assert _n_params(arch) == params
    assert len(A.param_shapes(arch)) == entries


def test_state_dict_key_names():
    keys = A.param_shapes("r18")
    for k in ("conv1.weight", "bn1.num_batches_tracked", "prelu.weight", "layer1.0.downsample.0.weight", "layer1.0.downsample.1.running_var",
              "layer4.1.conv2.weight", "layer2.1.prelu.weight", "bn2.bias", "fc.weight", "fc.bias", "features.running_mean"):
        assert k in keys, k
    assert "layer1.1.downsample.0.weight" not in keys
    assert keys["fc.weight"] == (512, 25088)


def test_loader_is_strict():
    sd = A.synth_weights("r18", 1)
    A.ArcFace.from_state_dict(sd, "r18")                                  # complete: accepted
    no_nbt = {k: v for k, v in sd.items() if not k.endswith("num_batches_tracked")}
    A.ArcFace.from_state_dict(no_nbt, "r18")                              # num_batches_tracked is optional
    bad = dict(sd)
    del bad["layer2.0.bn3.running_mean"]
    with pytest.raises(ValueError, match="layer2.0.bn3.running_mean"):
        A.ArcFace.from_state_dict(bad, "r18")
    bad = dict(sd)
    bad["layer9.0.conv1.weight"] = torch.zeros(1)
    with pytest.raises(ValueError, match="layer9.0.conv1.weight"):
        A.ArcFace.from_state_dict(bad, "r18")
    bad = dict(sd)
    bad["layer3.1.conv2.weight"] = torch.zeros(256, 256, 1, 1)
    with pytest.raises(ValueError, match="layer3.1.conv2.weight"):
        A.ArcFace.from_state_dict(bad, "r18")
    with pytest.raises(ValueError):
        A.ArcFace.from_state_dict(sd, "r18", torch.float32)


def test_from_pretrained_reads_a_local_pth(tmp_path):
    sd = A.synth_weights("r18", 2)
    p = tmp_path / "backbone.pth"
    torch.save(sd, p)
    m = A.ArcFace.from_pretrained(str(p), arch="r18")
    assert torch.equal(m._fw["fc.w"], A.fold_weights(sd, "r18")["fc.w"])


def test_synth_fixture_has_the_required_ranges():
    sd = A.synth_weights("r50", 0)
    for k, v in sd.items():
        if k.endswith("running_var"):
            assert 0.5 <= v.min() and v.max() <= 2.0, k
        if "prelu" in k:
            assert 0.05 <= v.min() and v.max() <= 0.4, k
        if k.endswith(".bias") and not k.startswith("fc"):
            assert v.abs().min() > 0, k
        if k.startswith("layer") and k.endswith("bn1.bias"):
            assert 0.5 <= v.abs().min() and v.abs().max() <= 2.0, k


@pytest.fixture(scope="module", params=["r50", "r100"])
def folded_run(request):
    arch = request.param
    torch.manual_seed(0)
    sd = A.synth_weights(arch, 0)
    x = torch.rand(2, 3, 112, 112, generator=torch.Generator().manual_seed(1)) * 2 - 1
    ref_st, got_st = [], []
    ref = O.forward(sd, arch, x, None, ref_st)
    got = O.run_folded(A.fold_weights(sd, arch), arch, x, got_st)
    return arch, sd, ref, got, ref_st, got_st


def _rel(a, b):
    return ((a - b).norm() / b.norm()).item()


def test_fold_equals_restatement_on_border_ring_and_interior(folded_run):
    """The folded weights, run by plain torch in NHWC with the second-output bn1, equal the unfolded fp32 restatement on the border ring
    of every stage (where a bn1 shift folded into a bias would be wrong) and in the interior."""
    _, _, _, _, ref_st, got_st = folded_run
    for r, g in zip(ref_st, got_st):
        g = g.permute(0, 3, 1, 2)
        ring = torch.ones(r.shape[-2:], dtype=torch.bool)
        ring[1:-1, 1:-1] = False
        assert _rel(g[..., ring], r[..., ring]) <= 1e-5, r.shape
        assert _rel(g[..., ~ring], r[..., ~ring]) <= 1e-5, r.shape


def test_fold_equals_restatement_on_the_head(folded_run):
    """The head matrix (bn2 + fc + features, columns permuted to NHWC) on the restatement's own layer4 output, in flattened order."""
    arch, sd, ref, got, ref_st, _ = folded_run
    fw = A.fold_weights(sd, arch)
    x4 = ref_st[-1]
    head_nhwc = x4.permute(0, 2, 3, 1).reshape(x4.shape[0], -1) @ fw["fc.w"].t() + fw["fc.b"]
    assert _rel(head_nhwc, O.head(sd, x4)) <= 1e-5
    assert _rel(got, ref) <= 1e-5


def test_a_folded_bn1_bias_would_be_wrong_on_the_border(folded_run):
    """Why the engine carries bn1 as a second output: folding bn1's shift into conv1's bias is exact in the interior only."""
    arch, sd, *_ = folded_run
    x = torch.randn(1, 512, 7, 7)
    k = "layer4.1"
    exact = F.conv2d(F.batch_norm(x, sd[f"{k}.bn1.running_mean"], sd[f"{k}.bn1.running_var"], sd[f"{k}.bn1.weight"], sd[f"{k}.bn1.bias"],
                                  False, 0.0, 1e-5), sd[f"{k}.conv1.weight"], None, 1, 1)
    a, b = A._affine(sd, f"{k}.bn1")
    w = sd[f"{k}.conv1.weight"].double()
    folded = F.conv2d(x.double(), w * a[None, :, None, None], torch.einsum("ocyx,c->o", w, b), 1, 1).float()
    ring = torch.ones(7, 7, dtype=torch.bool)
    ring[1:-1, 1:-1] = False
    assert _rel(folded[..., ~ring], exact[..., ~ring]) < 1e-5
    assert _rel(folded[..., ring], exact[..., ring]) > 1e-2


def test_fixture_activations_stay_in_range(folded_run):
    _, _, ref, _, ref_st, _ = folded_run
    for s in ref_st:
        assert 0.1 <= s.std().item() <= 10.0
    assert torch.isfinite(ref).all()


def test_emulated_autocast_error_is_small():
    """The rounding the GPU tolerances are sized from: r50 with every stored activation rounded to f16 / bf16."""
    sd = A.synth_weights("r50", 0)
    x = torch.rand(2, 3, 112, 112, generator=torch.Generator().manual_seed(1)) * 2 - 1
    ref = O.forward(sd, "r50", x)
    for dt, bound in ((torch.float16, 4e-3), (torch.bfloat16, 3e-2)):
        e = O.forward(sd, "r50", x, dt)
        assert ((e - ref).norm(dim=1) / ref.norm(dim=1)).max().item() < bound, dt


# ---- host-side refusals of the new descriptor fields (argument checks run before any HIP call) ---------------------------------------
def _desc(stride=1, taps=9, in_hw=8, out_hw=8, nsrc=1):
    d = _lib.GemmDesc()
    d.dtype, d.batch, d.out_h, d.out_w, d.stride, d.n, d.nsrc = _lib.IDB_F16, 1, out_hw, out_hw, stride, 64, nsrc
    d.src[0].ptr, d.src[0].channels, d.src[0].taps, d.src[0].in_h, d.src[0].in_w = 0x1000, 64, taps, in_hw, in_hw
    d.w, d.out, d.out_dtype, d.out_ld = 0x2000, 0x3000, _lib.IDB_F16, 64
    return d


def test_prelu_without_slope_is_refused(lib):
    d = _desc()
    d.act = 2
    assert lib.idb_gemm_plan(C.byref(d), None, None, None) == -1
    assert b"act_slope" in lib.idb_last_error()
    d.act_slope = 0x4000
    assert lib.idb_gemm_plan(C.byref(d), None, None, None) == 0
    d.residual = 0x5000                                                 # PReLU + residual: refused like GELU + residual
    assert lib.idb_gemm_plan(C.byref(d), None, None, None) == -1


def test_prelu_plans_split_k(lib):
    d = _desc()
    d.act, d.act_slope = 2, 0x4000
    for sk in (0, 1):
        d.split_k = sk
        tile, split, blocks = C.c_int32(), C.c_int32(), C.c_int32()
        assert lib.idb_gemm_plan(C.byref(d), C.byref(tile), C.byref(split), C.byref(blocks)) == 0
        assert split.value >= 2                                          # the reduce launch applies the PReLU
    d.act, d.act_slope = 0, None
    d.split_k = 0
    split = C.c_int32()
    assert lib.idb_gemm_plan(C.byref(d), None, C.byref(split), None) == 0


def test_strided_1x1_source(lib):
    # a 1x1 source on the 16x16 input grid of a stride-2 GEMM (8x8 output) reads pixel (2 oy, 2 ox): accepted
    d = _desc(stride=2, taps=9, in_hw=16, out_hw=8, nsrc=2)
    d.src[1].ptr, d.src[1].channels, d.src[1].taps, d.src[1].in_h, d.src[1].in_w = 0x6000, 64, 1, 16, 16
    assert lib.idb_gemm_plan(C.byref(d), None, None, None) == 0
    d.src[1].in_h = d.src[1].in_w = 15                                   # ceil(15 / 2) = 8: odd inputs too
    assert lib.idb_gemm_plan(C.byref(d), None, None, None) == 0
    d.src[1].in_h = d.src[1].in_w = 18
    assert lib.idb_gemm_plan(C.byref(d), None, None, None) == -1
    # the same source in a stride-1 GEMM: refused
    d = _desc(stride=1, taps=9, in_hw=8, out_hw=8, nsrc=2)
    d.src[1].ptr, d.src[1].channels, d.src[1].taps, d.src[1].in_h, d.src[1].in_w = 0x6000, 64, 1, 16, 16
    assert lib.idb_gemm_plan(C.byref(d), None, None, None) == -1
    assert b"output grid" in lib.idb_last_error()


def test_out2_needs_scale_and_shift(lib):
    d = _desc()
    d.out2 = 0x7000
    assert lib.idb_gemm_plan(C.byref(d), None, None, None) == -1
    assert b"out2" in lib.idb_last_error()
    d.out2_scale = 0x8000
    assert lib.idb_gemm_plan(C.byref(d), None, None, None) == -1
    d.out2_shift = 0x9000
    assert lib.idb_gemm_plan(C.byref(d), None, None, None) == 0
    d.out2 = None                                                        # scale / shift without the output: refused too
    assert lib.idb_gemm_plan(C.byref(d), None, None, None) == -1


def test_stem_and_head_argument_checks(lib):
    assert lib.idb_arcface_stem(None, 1, 1, 112, 112, None, None, None, None, None, None, None, _lib.IDB_F16, None) == -1
    assert lib.idb_arcface_head_workspace_bytes(4, 512, 25088) > 0
    assert lib.idb_arcface_head_workspace_bytes(4, 500, 25088) == 0
    assert lib.idb_arcface_head(0x1000, 0x2000, None, 0x3000, 4, 512, 25088, _lib.IDB_F16, None, 0, None) == -1


def test_call_needs_a_device():
    m = A.ArcFace.from_synthetic("r18", 0)
    with pytest.raises(RuntimeError):
        m(torch.zeros(1, 3, 112, 112))
    with pytest.raises(ValueError):
        m.to("cpu")
