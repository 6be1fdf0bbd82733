"""The embedding stage without a GPU: the float64 oracle (tests/frtail_oracle.py) against stock torch modules under float64 autograd and
against a recording of the reference's own IResNet class (tests/golden/frtail_reference.*, written by
tests/golden/make_frtail_reference.py), the SGD oracle against torch.optim.SGD + clip_grad_norm_, the C ABI's refusals, the Python
refusals and bookkeeping, and the preconditions on every input the GPU file checks."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import frtail_oracle as TO  # noqa: E402

from faceposegenerator_amd import _lib as L  # noqa: E402
from faceposegenerator_amd import frtail as T  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GRADS = ("bn2.weight", "bn2.bias", "fc.weight", "fc.bias", "features.bias", "input")


def _rel(got, want):
    return float(np.abs(np.asarray(got) - np.asarray(want)).max() / max(float(np.abs(np.asarray(want)).max()), 1e-300))


def _torch_stage(prm, ch, hw, n, eps=1e-5):
    bn2, fc, feat = nn.BatchNorm2d(ch, eps=eps).double(), nn.Linear(ch * hw, n).double(), nn.BatchNorm1d(n, eps=eps).double()
    with torch.no_grad():
        for mod, name in ((bn2, "bn2"), (feat, "features")):
            mod.weight.copy_(torch.from_numpy(prm[f"{name}.weight"]))
            mod.bias.copy_(torch.from_numpy(prm[f"{name}.bias"]))
            mod.running_mean.copy_(torch.from_numpy(prm[f"{name}.running_mean"]))
            mod.running_var.copy_(torch.from_numpy(prm[f"{name}.running_var"]))
        fc.weight.copy_(torch.from_numpy(TO.to_upstream(prm["fc.weight"], ch, hw)))
        fc.bias.copy_(torch.from_numpy(prm["fc.bias"]))
    feat.weight.requires_grad = False
    return bn2, fc, feat


@pytest.mark.parametrize("renorm", [False, True])
@pytest.mark.parametrize("B,ch,hw,n", [(2, 64, 1, 64), (5, 64, 4, 64), (37, 64, 49, 64)])
def test_oracle_equals_float64_autograd(B, ch, hw, n, renorm):
    p = 0.4
    x, prm, keep, g = TO.case_inputs(B, ch, hw, n, p)
    bn2, fc, feat = _torch_stage(prm, ch, hw, n)
    side = int(round(hw ** 0.5)) if int(round(hw ** 0.5)) ** 2 == hw else 1
    xt = torch.from_numpy(TO.to_upstream(x, ch, hw)).view(B, ch, side, hw // side).requires_grad_(True)
    kt = torch.from_numpy(TO.to_upstream(keep, ch, hw)).double()
    y = bn2(xt).flatten(1) * kt / (1 - p)
    features = F.normalize(feat(fc(y)))
    if renorm:                                                # the loop's three literal lines
        norm = torch.norm(features, 2, 1, True)
        output = torch.div(features, norm)
    else:
        output = features
    output.backward(torch.from_numpy(g).double())
    fw = TO.forward(x, prm, keep, p)
    bw = TO.backward(x, prm, keep, p, g, fw, renormalised=renorm)
    tol = 1e-12
    assert _rel(fw["emb"], features.detach().numpy()) <= tol
    want = {"bn2.weight": bn2.weight.grad, "bn2.bias": bn2.bias.grad, "fc.weight": torch.from_numpy(TO.to_device(fc.weight.grad.numpy(), ch, hw)),
            "fc.bias": fc.bias.grad, "features.bias": feat.bias.grad,
            "input": torch.from_numpy(TO.to_device(xt.grad.reshape(B, ch * hw).numpy(), ch, hw))}
    for k in GRADS:
        scale = max(float(want[k].abs().max()), float(np.abs(bw["fc.weight"]).max()) if k == "fc.bias" else 0.0)
        assert float(np.abs(bw[k] - want[k].numpy()).max()) <= tol * scale, k      # d fc.bias is 0 up to rounding: relative to d fc.weight
    assert feat.weight.grad is None
    got = fw["running"]
    for mod, name in ((bn2, "bn2"), (feat, "features")):
        assert _rel(got[f"{name}.running_mean"], mod.running_mean.numpy()) <= tol
        assert _rel(got[f"{name}.running_var"], mod.running_var.numpy()) <= tol
    # eval mode
    for m in (bn2, feat):
        m.eval()
    with torch.no_grad():
        ev = F.normalize(feat(fc(bn2(xt).flatten(1))))
    prm_now = dict(prm)
    prm_now.update(got)
    assert _rel(TO.forward(x, prm_now, None, p, training=False)["emb"], ev.numpy()) <= tol


def test_oracle_equals_reference_recording():
    """The reference's iresnet18(num_features=64, dropout=0.4) in float64 train mode, its layer4 output replaced by the formula tensor
    below, its stage parameters set from case_inputs, the dropout mask captured from the dropout module's output."""
    meta = json.load(open(os.path.join(GOLD, "frtail_reference.json")))
    rec = np.load(os.path.join(GOLD, "frtail_reference.npz"))
    B, ch, hw, n, p = meta["B"], meta["ch"], meta["hw"], meta["n"], meta["p"]
    assert (B, ch, hw, n, p) == (4, 512, 49, 64, 0.4) and meta["features_weight_requires_grad"] is False
    x, prm, _, g = TO.case_inputs(B, ch, hw, n, p)
    K = ch * hw
    keep = TO.to_device(np.unpackbits(rec["keep_bits"])[:B * K].reshape(B, K), ch, hw)
    assert 0.5 <= keep.mean() <= 0.7
    fw = TO.forward(x, prm, keep, p)
    bw = TO.backward(x, prm, keep, p, g, fw)
    tol = 1e-12
    assert _rel(fw["emb"], rec["embeddings"]) <= tol
    for k in ("bn2.weight", "bn2.bias", "features.bias"):
        assert _rel(bw[k], rec[f"grad.{k}"]) <= tol, k
    wg = TO.to_upstream(bw["fc.weight"], ch, hw)
    assert float(np.abs(bw["fc.bias"] - rec["grad.fc.bias"]).max()) <= tol * float(np.abs(wg).max())
    xg = TO.to_upstream(bw["input"], ch, hw)
    st = meta["stride"]
    for name, a in (("fc.weight", wg), ("input", xg)):
        assert _rel(a.sum(1), rec[f"grad.{name}.rowsum"]) <= 1e-11, name
        assert _rel(a.sum(0), rec[f"grad.{name}.colsum"]) <= 1e-11, name
        assert _rel(a.reshape(-1)[::st], rec[f"grad.{name}.sample"]) <= tol, name
    for k, v in fw["running"].items():
        assert _rel(v, rec[f"running.{k}"]) <= tol, k
    assert meta["num_batches_tracked"] == {"bn2": 1, "features": 1}


def test_sgd_oracle_equals_torch():
    shapes = [(8,), (8,), (6, 40), (6,), (6,)]
    ws = [((TO._h(np.arange(int(np.prod(s))) + 5 * i, 201) - 100) / 100.0).reshape(s) for i, s in enumerate(shapes)]
    params = [nn.Parameter(torch.from_numpy(w.copy())) for w in ws]
    opt = torch.optim.SGD(params, lr=0.1, momentum=0.9, weight_decay=5e-4)
    bufs, norms = None, []
    for step, scale in enumerate((3.0, 2.0, 0.01)):
        gs = [((TO._h(np.arange(w.size) + 7 * i + step, 301) - 150) / 150.0).reshape(w.shape) * scale for i, w in enumerate(ws)]
        for prm, gg in zip(params, gs):
            prm.grad = torch.from_numpy(gg.copy())
        ref_norm = float(torch.nn.utils.clip_grad_norm_(params, 5.0))
        opt.step()
        ws, bufs, norm = TO.sgd_step(ws, gs, bufs, 0.1, 0.9, 5e-4, 5.0)
        norms.append(norm)
        assert abs(norm - ref_norm) <= 1e-12 * ref_norm
        for w, b, prm in zip(ws, bufs, params):
            assert _rel(w, prm.detach().numpy()) <= 1e-12 and _rel(b, opt.state[prm]["momentum_buffer"].numpy()) <= 1e-12
    assert norms[0] > 5 and norms[2] < 5                       # the clip active, and idle


# ---- the C ABI without a GPU ---------------------------------------------------------------------------------------------------------
def _err(lib):
    return lib.idb_last_error().decode()


def _desc(**kw):
    d = L.TailDesc()
    d.b, d.ch, d.hw, d.n, d.x_dtype, d.training, d.p, d.eps2, d.eps1, d.momentum = 4, 64, 49, 64, L.IDB_F32, 1, 0.4, 1e-5, 1e-5, 0.1
    for k in ("x", "bn2_weight", "bn2_bias", "bn2_mean", "bn2_var", "fc_weight", "fc_bias", "feat_weight", "feat_bias", "feat_mean", "feat_var"):
        setattr(d, k, 4096)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_abi_symbols_and_refusals(lib):
    for name in ("idb_tail_workspace_bytes", "idb_tail_forward", "idb_tail_backward", "idb_sgd_clip_step"):
        assert name in L.EXPORTS and hasattr(lib, name)
    ks, rt = C.c_int32(0), C.c_int32(0)
    need = lib.idb_tail_workspace_bytes(128, 512, 49, 512, C.byref(ks), C.byref(rt))
    assert need > 0 and ks.value > 1 and rt.value == 1
    assert lib.idb_tail_workspace_bytes(130, 64, 1, 64, C.byref(ks), C.byref(rt)) > 0 and (ks.value, rt.value) == (1, 2)
    for bad in ((0, 64, 49, 64), (1025, 64, 49, 64), (4, 96, 49, 64), (4, 4096, 49, 64), (4, 64, 0, 64), (4, 64, 65, 64), (4, 64, 49, 32),
                (4, 64, 49, 2048)):
        assert lib.idb_tail_workspace_bytes(*bad, None, None) == 0, bad
    P, big = 4096, 1 << 40

    def fwd(d, ws=P, nbytes=big, out=P, affine=P):
        return lib.idb_tail_forward(C.byref(d) if d is not None else None, out, P, P, affine, P, P, P, P, ws, nbytes, None)

    def bwd(d, renorm=0, g=P, dw=P):
        return lib.idb_tail_backward(C.byref(d), g, P, P, P, P, P, P, P, renorm, P, P, dw, P, P, None, P, big, None)

    cases = [(lambda: fwd(None), "null descriptor"), (lambda: fwd(_desc(b=0)), "b in 1"), (lambda: fwd(_desc(ch=96)), "ch % 64"),
             (lambda: fwd(_desc(x_dtype=7)), "x_dtype"), (lambda: fwd(_desc(training=2)), "training must"),
             (lambda: fwd(_desc(b=1)), "batch of one"), (lambda: fwd(_desc(p=1.0)), "dropout p"), (lambda: fwd(_desc(p=-0.1)), "dropout p"),
             (lambda: fwd(_desc(eps2=-1.0)), "eps in"), (lambda: fwd(_desc(momentum=2.0)), "eps in"), (lambda: fwd(_desc(x=None)), "null pointer"),
             (lambda: fwd(_desc(fc_weight=4100)), "16-byte aligned"), (lambda: fwd(_desc(keep=4097)), "4-byte aligned"),
             (lambda: fwd(_desc(training=0, keep=P)), "keep-mask in eval"), (lambda: fwd(_desc(), ws=None), "workspace"),
             (lambda: fwd(_desc(), nbytes=16), "workspace"), (lambda: fwd(_desc(), out=None), "null output"),
             (lambda: fwd(_desc(), affine=4100), "affine 16-byte"), (lambda: bwd(_desc(training=0, b=4)), "eval mode"),
             (lambda: bwd(_desc(), g=None), "null input"), (lambda: bwd(_desc(), dw=None), "null output"),
             (lambda: bwd(_desc(), renorm=2), "renormalised must")]
    for call, msg in cases:
        assert call() == -1 and msg in _err(lib), (msg, _err(lib))
    n = 2
    arr = (C.c_void_p * n)(P, P)
    numel = (C.c_int64 * n)(16, 16)

    wts, bufs = (C.c_void_p * n)(2 * P, 3 * P), (C.c_void_p * n)(4 * P, 5 * P)

    def sgd(count=n, w=wts, numel=numel, lr=0.1, mom=0.9, wd=5e-4, mx=5.0, ws=P, nbytes=L.IDB_SGD_CLIP_WS_BYTES, total=P, buf=bufs):
        return lib.idb_sgd_clip_step(count, w, arr, buf, numel, lr, mom, wd, mx, 1, total, ws, nbytes, None)

    for call, msg in [(lambda: sgd(count=0), "1..8 tensors"), (lambda: sgd(count=9), "1..8 tensors"), (lambda: sgd(total=None), "null pointer"),
                      (lambda: sgd(lr=-1.0), "lr in"), (lambda: sgd(mom=1.0), "lr in"), (lambda: sgd(mx=0.0), "lr in"),
                      (lambda: sgd(nbytes=8), "workspace"), (lambda: sgd(w=(C.c_void_p * n)(2 * P, None)), "tensor 1: null"),
                      (lambda: sgd(numel=(C.c_int64 * n)(16, 0)), "tensor 1: 1..2^32"), (lambda: sgd(total=P + 4), "total_norm 8-byte"),
                      (lambda: sgd(w=(C.c_void_p * n)(2 * P, 2 * P)), "tensors 0 and 1 share a weight or momentum buffer"),
                      (lambda: sgd(buf=(C.c_void_p * n)(4 * P, 2 * P)), "tensors 0 and 1 share"),
                      (lambda: sgd(buf=wts), "tensor 0: weight and momentum buffer are the same")]:
        assert call() == -1 and msg in _err(lib), (msg, _err(lib))


# ---- Python refusals and bookkeeping -------------------------------------------------------------------------------------------------
def _sd(ch=64, hw=4, n=64):
    _, prm, _, _ = TO.case_inputs(2, ch, hw, n)
    sd = {k: torch.from_numpy(v.astype(np.float32)) for k, v in prm.items()}
    sd["fc.weight"] = torch.from_numpy(TO.to_upstream(prm["fc.weight"], ch, hw).astype(np.float32))
    return sd


def test_python_refusals():
    sd = _sd()
    with pytest.raises(ValueError, match=r"lacks \['bn2.running_var', 'fc.bias'\]"):
        T.EmbeddingStage.from_state_dict({k: v for k, v in sd.items() if k not in ("fc.bias", "bn2.running_var")})
    with pytest.raises(NotImplementedError, match="SE or bottleneck"):
        T.EmbeddingStage.from_state_dict(dict(sd, **{"layer1.0.se.fc1.weight": torch.zeros(1)}))
    with pytest.raises(NotImplementedError, match="SE or bottleneck"):
        T.EmbeddingStage.from_state_dict(dict(sd, **{"layer1.0.conv3.weight": torch.zeros(1)}))
    with pytest.raises(ValueError, match="does not fit"):
        T.EmbeddingStage.from_state_dict(dict(sd, **{"fc.weight": torch.zeros(64, 100)}))
    with pytest.raises(ValueError, match="dropout in"):
        T.EmbeddingStage.from_state_dict(sd, dropout=1.0)
    with pytest.raises(ValueError, match=r"bn2.bias expected \(64,\)"):
        T.EmbeddingStage.from_state_dict(dict(sd, **{"bn2.bias": torch.zeros(3)}))
    stage = T.EmbeddingStage.from_state_dict(sd)
    with pytest.raises(ValueError, match="no CPU fallback"):
        stage.to("cpu")
    with pytest.raises(L.IdbError, match="not on a device"):
        stage(torch.zeros(2, 2, 2, 64))
    with pytest.raises(L.IdbError, match="not on a device"):
        T.StageSGD(stage, 0.1).step(T.StageGrad(*[torch.zeros(1)] * 5, None, 4, 64))
    with pytest.raises(TypeError, match="must be an EmbeddingStage"):
        T.StageSGD(object(), 0.1)
    with pytest.raises(ValueError, match="lr in"):
        T.StageSGD(stage, -1.0)
    with pytest.raises(ValueError, match="without"):
        T.StageSGD(stage, 0.1).load_state_dict({"lr": 0.1})
    with pytest.raises(ValueError, match="exactly after the first step"):
        T.StageSGD(stage, 0.1).load_state_dict(dict(T.StageSGD(stage, 0.1).state_dict(), steps=2))
    with pytest.raises(TypeError, match="EmbeddingStage and the StageSGD"):
        T.train_step(stage, None, None, None, None, None)
    with pytest.raises(NotImplementedError, match="ReduceLROnPlateau"):
        T.learning_rate(0, auto_schedule=True)

    class Trunk:
        training = True
    with pytest.raises(NotImplementedError, match="trunk in training mode"):
        T.train_step_images(Trunk(), stage, None, None, None, None, None)
    stage.device = torch.device("cuda:0")                     # the remaining checks come before any device call
    for bad, msg in ((torch.zeros(2, 2, 2, 64, dtype=torch.float64), "float16, bfloat16 or float32"), (torch.zeros(2, 3, 2, 64), "NHWC"),
                     (torch.zeros(2, 2, 2, 32), "NHWC"), (torch.zeros(2, 2, 2, 64), "no CPU fallback")):
        with pytest.raises(ValueError, match=msg):
            stage(bad)
    big = torch.zeros(1025, 2, 2, 64)
    with pytest.raises(ValueError, match="batch 1025: expected 1..1024"):
        stage(big)
    with pytest.raises(ValueError, match="batch of one in training mode"):
        stage(torch.zeros(1, 2, 2, 64))
    with pytest.raises(ValueError, match=r"keep: expected bool or uint8 \[2, 256\]"):
        stage(torch.zeros(2, 2, 2, 64), keep=torch.ones(2, 255, dtype=torch.uint8))
    with pytest.raises(ValueError, match="keep: expected bool or uint8"):
        stage(torch.zeros(2, 2, 2, 64), keep=np.ones((2, 256), dtype=np.float32))
    with pytest.raises(ValueError, match="keep: a dropout mask in eval mode"):
        stage.eval()(torch.zeros(2, 2, 2, 64), keep=torch.ones(2, 256, dtype=torch.bool))
    stage.train()
    # backward's checks come before any device call too
    ctx = dict(stage=stage, training=True, b=2)
    with pytest.raises(ValueError, match=r"grad_embeddings: expected fp32 \[2, 64\]"):
        stage.backward(T.StageOut(None, None, ctx), torch.zeros(2, 63))
    with pytest.raises(ValueError, match="grad_embeddings: expected fp32"):
        stage.backward(T.StageOut(None, None, ctx), torch.zeros(2, 64, dtype=torch.float64))
    with pytest.raises(ValueError, match="eval-mode forward"):
        stage.backward(T.StageOut(None, None, dict(ctx, training=False)), torch.zeros(2, 64))
    with pytest.raises(ValueError, match="not produced by this stage"):
        T.EmbeddingStage.from_state_dict(sd).backward(T.StageOut(None, None, ctx), torch.zeros(2, 64))
    good = T.StageGrad(torch.zeros(64), torch.zeros(64), torch.zeros(64, 256), torch.zeros(64), torch.zeros(64), None, 4, 64)
    opt = T.StageSGD(stage, 0.1)
    with pytest.raises(ValueError, match=r"gradient of bn2.weight expected fp32 \(64,\) on cuda:0"):
        opt.step(good)                                        # on the CPU while the stage claims a device; shapes: the GPU file
    with pytest.raises(TypeError, match="expected the StageGrad"):
        opt.step(torch.zeros(3))
    stage.device = None
    with pytest.raises(ValueError, match=r"merged_into: fc.bias is \(3,\) in the backbone, \(64,\) here"):
        stage.merged_into(dict(sd, **{"fc.bias": torch.zeros(3)}))
    for bad in (dict(epoch=-1), dict(epoch=0, batch_size=0), dict(epoch=0, world=0)):
        with pytest.raises(ValueError, match="learning_rate: expected epoch >= 0"):
            T.learning_rate(**bad)
    with pytest.raises(ValueError, match="momentum_buffers expected"):
        T.StageSGD(stage, 0.1).load_state_dict(dict(T.StageSGD(stage, 0.1).state_dict(), steps=1, momentum_buffers={"fc.bias": torch.zeros(64)}))
    with pytest.raises(ValueError, match=r"momentum buffer bn2.weight expected \(64,\)"):
        T.StageSGD(stage, 0.1).load_state_dict(dict(T.StageSGD(stage, 0.1).state_dict(), steps=1,
                                                    momentum_buffers={k: torch.zeros(3) for k in T.TRAINABLE}))
    odd = dict(sd, **{k: torch.ones(96) for k in sd if k.startswith("bn2.")}, **{"fc.weight": torch.zeros(64, 96 * 4)})
    with pytest.raises(ValueError, match=r"ch 96 \(% 64 == 0"):
        T.EmbeddingStage.from_state_dict(odd)
    with pytest.raises(ValueError, match="eps in"):
        T.EmbeddingStage.from_state_dict(sd, eps=-1.0)


def test_state_dict_round_trips():
    sd = _sd()
    stage = T.EmbeddingStage.from_state_dict(sd)
    out = stage.state_dict()
    assert list(out) == list(T.STAGE_KEYS) and out["bn2.num_batches_tracked"].item() == 0
    for k, v in sd.items():
        assert torch.equal(out[k], v), k
    assert torch.equal(stage.t["fc.weight"].view(64, 4, 64)[5, 3, 7], sd["fc.weight"].view(64, 64, 4)[5, 7, 3])
    full = dict(sd, **{"conv1.weight": torch.ones(2, 2)})
    stage.t["fc.bias"] += 1.0
    stage.tracked["bn2"] = 3
    merged = stage.merged_into(full)
    assert torch.equal(merged["conv1.weight"], full["conv1.weight"]) and torch.equal(merged["fc.bias"], sd["fc.bias"] + 1.0)
    assert "bn2.num_batches_tracked" not in merged            # the backbone dict had none
    merged = stage.merged_into(dict(full, **{"bn2.num_batches_tracked": torch.tensor(0)}))
    assert merged["bn2.num_batches_tracked"].item() == 3
    again = T.EmbeddingStage.from_state_dict(merged)
    assert all(torch.equal(again.t[k], stage.t[k]) for k in stage.t) and again.tracked["bn2"] == 3
    with pytest.raises(ValueError, match="lacks"):
        stage.merged_into({"conv1.weight": torch.ones(1)})
    syn = T.EmbeddingStage.from_synthetic(3, ch=64, hw=4, n=64)
    assert syn.t["fc.weight"].shape == (64, 256) and torch.equal(syn.t["features.weight"], torch.ones(64)) and syn.training
    assert not syn.eval().training and syn.train().training
    up = torch.arange(2 * 12.0).view(2, 12)
    assert torch.equal(T.to_upstream_order(T.to_device_order(up, 3, 4), 3, 4), up)
    assert np.array_equal(T.to_device_order(up, 3, 4).numpy(), TO.to_device(up.numpy(), 3, 4))


def test_learning_rate():
    def by_hand(epoch):                                       # the config's function, evaluated by hand
        return 0.1 ** len([m for m in [22, 30, 35] if m - 1 <= epoch])
    want = {0: 1.0, 20: 1.0, 21: 0.1, 29: 0.1 ** 2, 34: 0.1 ** 3, 35: 0.1 ** 3}
    for epoch, factor in want.items():
        assert by_hand(epoch) == pytest.approx(factor, rel=1e-15)
        assert T.learning_rate(epoch) == 0.1 / 512 * 128 * 1 * by_hand(epoch)
    assert T.learning_rate(0, base=0.2, batch_size=256, world=2) == 0.2 / 512 * 256 * 2


# ---- preconditions on every input the GPU file checks --------------------------------------------------------------------------------
@pytest.mark.parametrize("B,ch,hw,n,p", TO.gpu_cases(), ids=lambda v: str(v))
def test_gpu_inputs_are_well_conditioned_and_bounds_see_every_term(B, ch, hw, n, p):
    x, prm, keep, g = TO.case_inputs(B, ch, hw, n, p)
    fw = TO.forward(x, prm, keep, p)
    # (a) no near-constant channel or feature
    xr = x.reshape(B * hw, ch)
    assert xr.std(0).min() >= 1e-2 * np.sqrt((xr ** 2).mean())
    assert fw["z"].std(0).min() >= 1e-2 * np.sqrt((fw["z"] ** 2).mean())
    # (b) the kept share
    if p > 0:
        assert 0.5 <= keep.mean() <= 0.7 and 0.5 <= keep.mean(1).min() and keep.mean(1).max() <= 0.7
    else:
        assert keep.all()
    # (c) every term is visible at 4x the bound somewhere
    fb = TO.forward_bounds(x, prm, fw)
    bw = TO.backward(x, prm, keep, p, g, fw)
    bb = TO.backward_bounds(x, prm, fw, bw)

    def seen_bwd(term, renorm=False, base=bw, bound=bb):
        alt = TO.backward(x, prm, keep, p, g, fw, renormalised=renorm, omit=term)
        return any((np.abs(alt[k] - base[k]) > 4 * bound[k]).any() for k in GRADS)

    # without a mask g_y = g_z W and sum_b g_z = 0 (the BatchNorm1d backward), so the bn2 mean term is 0 and can show only at p > 0
    terms = ["bn2_xhat_term", "bn1_mean_term", "bn1_zhat_term", "projection"]
    if p > 0:
        terms += ["bn2_mean_term", "mask_bwd", "mask_scale"]
    for term in terms:
        assert seen_bwd(term), term
    # the second projection can show in no gradient: on unit rows it is the projection I - e e^T once more, and a projection is
    # idempotent, so the loop's norm / div lines change the cotangent only through the rounding of |e| (asserted here instead)
    bwr = TO.backward(x, prm, keep, p, g, fw, renormalised=True)
    alt = TO.backward(x, prm, keep, p, g, fw, renormalised=True, omit="second_projection")
    assert all(np.abs(alt[k] - bwr[k]).max() <= 1e-12 * max(np.abs(bwr["fc.weight"]).max(), np.abs(bwr[k]).max()) for k in GRADS)
    for term in ("unbiased", "momentum"):
        alt = TO.forward(x, prm, keep, p, omit=term)["running"]
        assert any((np.abs(alt[k] - fw["running"][k]) > 4 * fb["running"][k]).any() for k in alt), term
    alt = TO.forward(x, prm, keep, p, omit="fc_bias")
    assert (np.abs(alt["z"] - fw["z"]) > 4 * fb["z"]).any()
    if p > 0:
        alt = TO.forward(x, prm, keep, p, omit="mask_scale")
        assert (np.abs(alt["z"] - fw["z"]) > 4 * fb["z"]).any()


def test_free_running_float64_loop_lowers_its_loss():
    """The loop test_frtail_gpu.test_train_step runs on the GPU, here free-running in float64: five CosFace steps lower the loss."""
    import frhead_grad_oracle as GO
    B, ch, hw, n, p, Cn, lr = 37, 64, 49, 64, 0.4, 33, 0.05
    x, prm, keep, g = TO.case_inputs(B, ch, hw, n, p)
    labels = (TO._h(np.arange(B) + 3, Cn)).astype(np.int64)
    kernel = ((TO._h(np.arange(n * Cn) + 13, 2001).reshape(n, Cn) - 1000) / 1000.0 * 0.05).astype(np.float32).astype(np.float64)
    names = list(T.TRAINABLE)
    bufs = hbuf = None
    losses = []
    for _ in range(5):
        fw = TO.forward(x, prm, keep, p)
        hb = GO.backward("CosFace", fw["emb"], kernel, labels)
        bw = TO.backward(x, prm, keep, p, hb["d_emb"], fw)
        losses.append(hb["loss"])
        ws, bufs, _ = TO.sgd_step([prm[k] for k in names], [bw[k] for k in names], bufs, lr)
        prm = dict(prm, **dict(zip(names, ws)), **fw["running"])
        (kernel,), hbuf, _ = TO.sgd_step([kernel], [hb["d_kernel"]], hbuf, lr)
    assert losses[-1] < losses[0], losses
