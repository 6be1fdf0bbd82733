"""The FR loss head without a GPU: the float64 oracle (tests/frhead_oracle.py) against outputs recorded from the reference's own CosFace,
ArcFace, AdaFace and CrossEntropyLoss (tests/golden/frhead_reference.*, run on the CPU in float64 and in fp32), the module's host
arithmetic (dataset_labels, multi_class_acc, the AverageMeter averaging, the header-file loaders) against the same recordings, every
refusal before any HIP call, the C ABI's own argument checks, and the preconditions of the GPU test's cases.

Float64 recordings, u = 2^-53.  Both sides evaluate one expression in double with different summation orders.  The fp32 operands and
their products are exact in double; a column or row norm is within (D / 2 + 1) u relative, the dot product of the D products within
(D - 1) u sum |a b| <= (D - 1) u, so a cosine is within (2 D + 8) u on either side and (4 D + 16) u =: e between the two.  CosFace is
linear in it: s e.  ArcFace and AdaFace go through acos, whose slope is 1 / sqrt(1 - c^2); the recorded cosines stay within |c| <= 0.999
(asserted), where the slope is at most 22.4: s (22.4 e + 16 u) with a few u for acos and cos themselves.  The log-sum-exp is 1-Lipschitz
in the maximum norm, the per-sample loss subtracts one more logit, the mean over B adds nothing: twice the logit bound, plus
(C + B + 16) u relative for the sums of C exponentials and B losses, taken on |loss| <= 4 s.

fp32 recordings, u = 2^-24.  Upstream rounds every normalised component (relative (D / 2 + 2) u with fp32 norms), sums D products in
some order, (D + 2) u, and rounds acos, cos and the scale: a cosine within (2 D + 6) u, a logit within s ((2 D + 6) u k + 8 u) with
k = 1 / sqrt(1 - c_max^2) for ArcFace / AdaFace (c_max from the oracle's own cosines) and 1 for CosFace; the fp32 log-softmax adds a
few u of |lse| <= 4 s.
"""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest
import torch

import frhead_oracle as O
from faceposegenerator_amd import _lib
from faceposegenerator_amd import frhead as H

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
REF = np.load(os.path.join(GOLD, "frhead_reference.npz"))
META = json.load(open(os.path.join(GOLD, "frhead_reference.json")))
IDS = [c[0] for c in O.CASES]
SLOPE = 1 / math.sqrt(1 - 0.999 ** 2)


def _case(name):
    _, loss, B, Cn, D, seed = next(c for c in O.CASES if c[0] == name)
    emb, kernel, labels, norms = O.inputs(loss, B, Cn, D, seed)
    kw = dict(norms=norms, t_alpha=0.3 if name.endswith("_ema") else 1.0) if loss == "AdaFace" else {}
    th, extras = O.thetas(loss, emb, kernel, labels, **kw)
    return loss, B, Cn, D, emb, kernel, labels, norms, th, extras


@pytest.mark.parametrize("name", IDS)
def test_inputs_are_the_recorded_inputs(name):
    loss, B, Cn, D, emb, kernel, labels, norms, _, _ = _case(name)
    want = REF[name + "_checksum"]
    got = [emb.astype(np.float64).sum(), kernel.astype(np.float64).sum(), labels.sum(), norms.astype(np.float64).sum()]
    assert np.allclose(got, want, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("name", IDS)
def test_oracle_matches_the_float64_recording(name):
    loss, B, Cn, D, emb, kernel, labels, norms, th, extras = _case(name)
    assert np.abs(th).max() <= 0.999 * O.S                    # |c| <= 0.999: the slope of acos is bounded as the docstring says
    e = (4 * D + 16) * O.U64
    bound = O.S * e if loss == "CosFace" else O.S * (SLOPE * e + 16 * O.U64)
    err = np.abs(th - REF[name + "_thetas_f64"]).max()
    assert err <= bound, (err, bound)
    loss_v, per, lse = O.cross_entropy(th, labels)
    assert abs(loss_v - float(REF[name + "_loss_f64"])) <= 2 * bound + (Cn + B + 16) * O.U64 * 4 * O.S
    assert np.array_equal(O.argmax(th), REF[name + "_pred_f64"])
    assert O.multi_class_acc(O.argmax(th), labels) == float(REF[name + "_acc_f64"])
    assert 0.0 < float(REF[name + "_acc_f64"]) < 100.0        # a fixture that is all right or all wrong tests no argmax
    if loss == "AdaFace":
        got = np.array([extras["batch_mean"], extras["batch_std"]])
        assert np.abs(got - REF[name + "_buffers_f64"]).max() <= (B + 8) * O.U64 * 100


@pytest.mark.parametrize("name", IDS)
def test_oracle_is_within_fp32_rounding_of_the_fp32_recording(name):
    loss, B, Cn, D, emb, kernel, labels, norms, th, extras = _case(name)
    cmax = np.abs(th).max() / O.S + 0.01
    k = 1.0 if loss == "CosFace" else 1 / math.sqrt(1 - cmax ** 2)
    bound = O.S * ((2 * D + 6) * O.U32 * k + 8 * O.U32)
    err = np.abs(th - REF[name + "_thetas_f32"].astype(np.float64)).max()
    assert err <= bound, (err, bound)
    loss_v = O.cross_entropy(th, labels)[0]
    assert abs(loss_v - float(REF[name + "_loss_f32"])) <= 2 * bound + 8 * O.U32 * 4 * O.S
    if loss == "AdaFace":                                     # fp32 buffers: the mean and std of B fp32 values of at most 100
        got = np.array([extras["batch_mean"], extras["batch_std"]])
        assert np.abs(got - REF[name + "_buffers_f32"]).max() <= (B + 8) * O.U32 * 100


@pytest.mark.parametrize("loss", ["CosFace", "ArcFace", "AdaFace"])
def test_oracle_at_the_clamps(loss):
    """Columns along and against an embedding (cosine +-1, where ArcFace's acos has no slope bound): the clamp decides, and the error
    of acos at the clamp is that of a square root, (pi / 2) sqrt(2 e)."""
    emb, kernel, labels, norms = (REF[f"clamp_{loss}_{k}"] for k in ("emb", "kernel", "labels", "norms"))
    th, _ = O.thetas(loss, emb, kernel, labels, **(dict(norms=norms) if loss == "AdaFace" else {}))
    bound = O.S * (math.pi / 2 * math.sqrt(2 * (4 * 16 + 16) * O.U64) + 16 * O.U64)
    assert np.abs(th - REF[f"clamp_{loss}_thetas_f64"]).max() <= bound
    assert abs(O.cross_entropy(th, labels)[0] - float(REF[f"clamp_{loss}_loss_f64"])) <= 2 * bound
    if loss == "AdaFace":                                     # the clamp applies to every entry, not only to the target
        assert abs(th[1, 1] + O.S * (1 - O.EPS)) <= 1e-9 and abs(th[2, 2] - O.S * (1 - O.EPS)) <= 1e-9


def test_host_arithmetic_against_the_recordings():
    labels, classes = H.dataset_labels(META["names"])
    assert labels.tolist() == META["labels"] and classes == META["classes"]
    assert O.dataset_labels(META["names"])[0].tolist() == META["labels"]
    for correct, batch, acc in META["multi_class_acc"]:
        assert H.multi_class_acc(correct, batch) == acc
        assert O.multi_class_acc([1] * correct + [0] * (batch - correct), [1] * batch) == acc
    m = META["meter"]
    got = H.average_meters(m["losses"], m["accs"])
    assert (got["loss"], got["top1"], got["steps"]) == (m["loss_avg"], m["acc_avg"], len(m["losses"]))
    assert (O.average_meter(m["losses"]), O.average_meter(m["accs"])) == (m["loss_avg"], m["acc_avg"])
    with pytest.raises(ValueError):
        H.dataset_labels(["a_1.png"])
    with pytest.raises(ValueError):
        H.dataset_labels([])
    with pytest.raises(ValueError):
        H.average_meters([], [])


def test_validate_averages_the_steps_as_the_meters_do(monkeypatch):
    m = META["meter"]
    steps = iter([{"loss": lv, "acc": av} for lv, av in zip(m["losses"], m["accs"])])
    monkeypatch.setattr(H, "step_metrics", lambda *a, **k: next(steps))
    got = H.validate(None, None, [(None, None)] * len(m["losses"]))
    assert got == {"loss": m["loss_avg"], "top1": m["acc_avg"], "steps": len(m["losses"])}


@pytest.mark.parametrize("loss", ["CosFace", "AdaFace"])
def test_header_files_load(loss, tmp_path):
    """The header file is written here, with the keys, shapes and dtypes the reference's header.state_dict() was recorded to have
    (kernel fp32 [in, out]; AdaFace also t, batch_mean, batch_std, fp32 [1]) and the recorded values."""
    sd = {"kernel": torch.from_numpy(REF[f"header_{loss}_kernel"])}
    if loss == "AdaFace":
        sd.update({k: torch.tensor(META["header_AdaFace"][k], dtype=torch.float32) for k in ("t", "batch_mean", "batch_std")})
    assert sorted(sd) == META[f"header_{loss}_keys"]
    path = str(tmp_path / "1000_header.pth")
    torch.save(sd, path)
    hd = H.MarginHeader.from_pretrained(path, loss)
    assert sorted(torch.load(path, weights_only=True)) == META[f"header_{loss}_keys"]
    assert np.array_equal(hd.kernel.numpy(), REF[f"header_{loss}_kernel"]) and (hd.in_features, hd.out_features) == (16, 9)
    assert (hd.s, hd.m) == (64.0, O.DEFAULT_M[loss]) and (hd.h, hd.t_alpha) == (0.333, 1.0)
    if loss == "AdaFace":
        want = META["header_AdaFace"]
        assert (hd.t, hd.batch_mean, hd.batch_std) == (want["t"][0], want["batch_mean"][0], want["batch_std"][0])
        assert hd.batch_mean != 20.0                           # the recording moved the buffers off their defaults
        sd = hd.state_dict()
        again = H.MarginHeader.from_state_dict(sd, "AdaFace")
        assert (again.batch_mean, again.batch_std) == (hd.batch_mean, hd.batch_std)
        with pytest.raises(ValueError):
            H.MarginHeader.from_state_dict({"kernel": sd["kernel"]}, "AdaFace")
    with pytest.raises(ValueError):
        H.MarginHeader.from_state_dict({"weight": hd.kernel}, loss)
    syn = H.MarginHeader.from_synthetic(64, 301, 3, "ArcFace")
    assert tuple(syn.kernel.shape) == (64, 301) and syn.m == 0.50 and 0.008 < float(syn.kernel.std()) < 0.012


# ---- refusals, all before any HIP call (these tests run without a GPU, where a HIP call would fail in another way) -------------------
def test_python_refusals():
    for name in ("ElasticCosFace", "NonLinearHeader"):
        with pytest.raises(NotImplementedError, match=name):
            H.MarginHeader.from_synthetic(8, 4, 0, name)
        with pytest.raises(NotImplementedError, match=name):
            H.MarginHeader.from_pretrained("/nonexistent/header.pth", name)
    with pytest.raises(ValueError, match="expected one of"):
        H.MarginHeader.from_synthetic(8, 4, 0, "SphereFace")
    k = torch.randn(8, 4)
    k[:, 2] = 0
    with pytest.raises(ValueError, match="zero or non-finite column"):
        H.MarginHeader(k, "CosFace")
    with pytest.raises(ValueError, match="in_features"):
        H.MarginHeader(torch.randn(4097, 2), "CosFace")
    hd = H.MarginHeader.from_synthetic(8, 4, 0, "CosFace")
    e = torch.randn(3, 8)
    for bad in ([0, 1, -1], [0, 4, 1]):
        with pytest.raises(ValueError, match="label"):
            hd.loss(e, torch.tensor(bad))
        with pytest.raises(ValueError, match="label"):
            hd(e, torch.tensor(bad))
    with pytest.raises(ValueError, match="label"):
        hd.loss(e, torch.tensor([0, 1]))
    with pytest.raises(ValueError, match="embeddings"):
        hd.loss(torch.randn(3, 7), torch.tensor([0, 1, 2]))
    with pytest.raises(ValueError, match="CosFace and ArcFace take"):
        hd.loss(e, torch.tensor([0, 1, 2]), norms=torch.ones(3))
    ada = H.MarginHeader.from_synthetic(8, 4, 0, "AdaFace")
    with pytest.raises(ValueError, match="at least 2"):
        ada.loss(e[:1], torch.tensor([0]), norms=torch.ones(1))
    with pytest.raises(ValueError, match="AdaFace takes"):
        ada.loss(e, torch.tensor([0, 1, 2]))
    with pytest.raises(_lib.IdbError, match="not on a device"):       # valid arguments, but never packed: no silent CPU path
        hd.loss(e, torch.tensor([0, 1, 2]))
    with pytest.raises(ValueError, match="HIP device"):
        hd.to("cpu")

    class Training:
        training = True

    with pytest.raises(NotImplementedError, match="training mode"):
        H.step_metrics(Training(), hd, None, None)
    with pytest.raises(NotImplementedError, match="training mode"):
        H.step_metrics(object(), hd, None, None, training=True)


def _desc(**kw):
    d = _lib.HeadDesc()
    d.kind, d.b, d.d, d.c, d.s, d.m, d.h, d.t_alpha = 0, 4, 8, 5, 64.0, 0.35, 0.333, 1.0
    for f in ("emb", "norms", "label", "kernel", "wn", "col_norm", "ada_state"):
        setattr(d, f, 0x1000)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_abi_symbols_and_refusals(lib):
    for name in ("idb_head_pack", "idb_head_workspace_bytes", "idb_head_loss", "idb_head_logits"):
        assert hasattr(lib, name) and name in _lib.EXPORTS
    ws = 0x1000
    cases = [(dict(kind=3), b"loss kind"), (dict(b=0), b"b in 1.."), (dict(b=65537), b"b in 1.."), (dict(d=4097), b"d in 1.."),
             (dict(c=(1 << 20) + 1), b"c in 1.."), (dict(c=0), b"c in 1.."), (dict(kind=2, b=1), b"AdaFace needs b >= 2"),
             (dict(wn=None), b"not packed"), (dict(col_norm=None), b"not packed"), (dict(label=None), b"null pointer"),
             (dict(kind=2, norms=None), b"AdaFace needs norms"), (dict(s=0.0), b"s in"), (dict(t_alpha=1.5), b"t_alpha")]
    for kw, text in cases:
        d = _desc(**kw)
        assert lib.idb_head_loss(C.byref(d), ws, ws, ws, ws, ws, 1 << 30, None) == -1, kw
        assert text in lib.idb_last_error(), (kw, lib.idb_last_error())
        assert lib.idb_head_logits(C.byref(d), ws, ws, ws, 1 << 30, None) == -1, kw
        assert text in lib.idb_last_error(), (kw, lib.idb_last_error())
    d = _desc()
    assert lib.idb_head_loss(C.byref(d), ws, ws, ws, ws, ws, 16, None) == -1 and b"workspace" in lib.idb_last_error()
    assert lib.idb_head_loss(C.byref(d), None, ws, ws, ws, ws, 1 << 30, None) == -1 and b"null output" in lib.idb_last_error()
    assert lib.idb_head_pack(ws, 0, 5, ws, ws, ws, None) == -1 and b"d in 1.." in lib.idb_last_error()
    assert lib.idb_head_pack(ws, 8, 5, None, ws, ws, None) == -1 and b"null pointer" in lib.idb_last_error()
    for shape in ((0, 8, 5), (4, 0, 5), (4, 8, 0), (65537, 8, 5), (4, 4097, 5), (4, 8, (1 << 20) + 1)):
        assert lib.idb_head_workspace_bytes(*shape, None, None) == 0


def test_workspace_query_reports_the_grid(lib):
    """B = 130, C = 4099 must take more than one row tile and more than one column block; B = 128 at a WebFace-sized C fills 256 CUs."""
    rt, cb = C.c_int32(0), C.c_int32(0)
    assert lib.idb_head_workspace_bytes(130, 512, 4099, C.byref(rt), C.byref(cb)) > 0 and rt.value == 2 and cb.value > 1
    assert lib.idb_head_workspace_bytes(128, 512, 10572, C.byref(rt), C.byref(cb)) > 0 and rt.value == 1 and cb.value >= 256
    assert lib.idb_head_workspace_bytes(65536, 4096, 1 << 20, C.byref(rt), C.byref(cb)) < (3 << 30)
    assert lib.idb_head_workspace_bytes(1, 7, 1, C.byref(rt), C.byref(cb)) > 0 and (rt.value, cb.value) == (1, 1)


def test_gpu_cases_keep_the_argmax_decidable():
    """The GPU test accepts either contender on rows whose float64 top-two gap is within twice the logit bound, and fails if more than
    5 % of a case's rows are such rows: the seeds are chosen so that the oracle alone stays under that share."""
    for loss, B, Cn, D in O.gpu_cases():
        if Cn > 301 and D != 512 and B not in (1, 130):       # the float64 products at C = 4099 take the time; the GPU test checks all
            continue
        emb, kernel, labels, norms = O.inputs(loss, B, Cn, D, O.gpu_seed(loss, B, Cn, D))
        th, _ = O.thetas(loss, emb, kernel, labels, **(dict(norms=norms) if loss == "AdaFace" else {}))
        share = O.ambiguous_rows(th, O.logit_bound(D)).mean() if Cn > 1 else 0.0
        assert share <= 0.05, (loss, B, Cn, D, share)
