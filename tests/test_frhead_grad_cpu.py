"""The FR loss head's backward without a GPU: the float64 oracle (tests/frhead_grad_oracle.py) against `embeddings.grad` and
`kernel.grad` recorded from the reference's own CosFace / ArcFace / AdaFace and CrossEntropyLoss under autograd
(tests/golden/frhead_grad_reference*.npz; float64 with torch.set_default_dtype(torch.float64): upstream's `m_hot` is created as
default-dtype zeros, so CosFace's 0.35 otherwise enters as a float32 value), its optimiser step against a recording of torch's SGD and
clip_grad_norm_ (and against torch's own, run here), the new C entry points' argument checks before any HIP call, the workspace query's
grid, the Python-side refusals, HeaderSGD's host bookkeeping, and the preconditions of the GPU test's cases.

Float64 bound, u = 2^-53, s = 64.  Oracle and autograd evaluate the same expression with different summation orders.  A cosine is
within e = (4 D + 16) u between the two (test_frhead_cpu.py), a logit within L = s (22.4 e + 16 u) (|c| <= 0.999, asserted for the
recorded cases; CosFace: s e), the log-sum-exp within L + (C + 16) u 4 s, so a probability within p (exp(2 L + (C + 16) u 4 s) - 1) and
the target's slope within e sin(m) / (1 - c^2)^1.5 + 64 u / sqrt(1 - c^2) <= 1.2e4 e.  Every entry of G therefore has relative error
at most R = 2 L + (C + 16) u 4 s + 1.2e4 e + 16 u (relative to (p + 1) s d / B for the target, whose p - 1 inherits p's absolute
error).  The products sum C (or B) terms, (K + 2) u relative to sum |G| |operand|; the projection scalar is such a sum as well, and the
division adds 2 u.  With `A` the same expression evaluated on absolute values (|G| |Wn|, then |x| sum |G r| added, divided by the
norm) the bound is (R + (C + B + D + 16) u) A per element, taken twice to cover both sides' orders: at most 3e-9 A at D = 512 (the slope term).
The clamp cases put a cosine at +-1 on purpose; there only the entries the clamp removes are ill-conditioned, and they contribute
exactly 0 on both sides, so the same bound holds with the slope factor taken at the clamp, 0.999.
"""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest
import torch

import frhead_grad_oracle as GO
import frhead_oracle as O
from faceposegenerator_amd import _lib
from faceposegenerator_amd import frhead as H

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
REF = {**np.load(os.path.join(GOLD, "frhead_grad_reference.npz")), **np.load(os.path.join(GOLD, "frhead_grad_reference_512.npz"))}
META = json.load(open(os.path.join(GOLD, "frhead_grad_reference.json")))


def _f64_bounds(ref, B, Cn, D):
    e = (4 * D + 16) * O.U64
    rel = 2 * O.S * (22.4 * e + 16 * O.U64) + (Cn + 16) * O.U64 * 4 * O.S + 1.2e4 * e + 16 * O.U64 + (Cn + B + D + 16) * O.U64
    aG, aw, ax = np.abs(ref["G"]), np.abs(ref["w"]), np.abs(ref["x"])
    rows, labels = np.arange(B), ref["labels"]
    aG[rows, labels] = O.S / B * (ref["p"][rows, labels] + 1) * np.abs(ref["slope"])     # p - 1 inherits p's absolute error
    a_emb = (aG @ aw.T + ax * (aG * np.abs(ref["r"])).sum(axis=1, keepdims=True)) / ref["n_e"]
    a_ker = ((aG.T @ ax + aw.T * (aG * np.abs(ref["r"])).sum(axis=0)[:, None]) / ref["cn"].T).T
    return 2 * rel * a_emb, 2 * rel * a_ker


def _recorded(name):
    _, loss, B, Cn, D, seed = next(c for c in O.CASES if c[0] == name)
    emb, kernel, labels, norms = O.inputs(loss, B, Cn, D, seed)
    return loss, B, Cn, D, emb, kernel, labels, norms


@pytest.mark.parametrize("name", GO.RECORDED)
def test_oracle_matches_the_autograd_recording(name):
    loss, B, Cn, D, emb, kernel, labels, norms = _recorded(name)
    got = [emb.astype(np.float64).sum(), kernel.astype(np.float64).sum(), labels.sum(), norms.astype(np.float64).sum()]
    assert np.allclose(got, REF[name + "_checksum"], rtol=1e-12, atol=1e-12)
    ref = GO.backward(loss, emb, kernel, labels, norms=norms)
    assert np.abs(ref["r"]).max() <= 0.999
    eb, kb = _f64_bounds(ref, B, Cn, D)
    assert (np.abs(ref["d_emb"] - REF[name + "_d_emb"]) <= eb).all()
    assert (np.abs(ref["d_kernel"] - REF[name + "_d_kernel"]) <= kb).all()
    assert abs(ref["loss"] - float(REF[name + "_loss"])) <= 1e-11
    assert np.abs(REF[name + "_d_kernel"]).max() > 1.0 and eb.max() <= 1e-7 * np.abs(ref["d_emb"]).max() and kb.max() <= 1e-7 * np.abs(ref["d_kernel"]).max()     # the bound is double-sized, the gradient is not


@pytest.mark.parametrize("kind", ["non_target", "target_clipped"])
def test_oracle_matches_the_recording_at_the_clamps(kind):
    emb, kernel, labels, norms = GO.clamp_case(kind)
    got = [emb.astype(np.float64).sum(), kernel.astype(np.float64).sum(), labels.sum(), norms.astype(np.float64).sum()]
    assert np.allclose(got, REF[f"clamp_{kind}_checksum"], rtol=1e-12, atol=1e-12)
    ref = GO.backward("AdaFace", emb, kernel, labels, norms=norms)
    B, Cn, D = 6, 33, 130
    eb, kb = _f64_bounds(ref, B, Cn, D)
    want_e, want_k = REF[f"clamp_{kind}_d_emb"], REF[f"clamp_{kind}_d_kernel"]
    assert (np.abs(ref["d_emb"] - want_e) <= eb).all() and (np.abs(ref["d_kernel"] - want_k) <= kb).all()
    if kind == "non_target":
        # cosine +1 (row 0, column 2) and -1 (row 1, column 3) against the 0.999 clamp: those entries pass nothing on.  What is left in
        # the two columns comes from the other rows alone (9e-10 of the largest gradient in the recording)
        assert ref["r"][0, 2] > 0.9999 and ref["r"][1, 3] < -0.9999 and ref["G"][0, 2] == 0.0 and ref["G"][1, 3] == 0.0
        assert np.abs(want_k[:, [2, 3]]).max() <= 1e-8 * np.abs(want_k).max()
        # the mask is what removes them: without it row 0 would receive s p_02 w_2 / B (in d_kernel the same entry is radial to column
        # 2, which lies along the row, and the projection removes it either way)
        without = GO.backward("AdaFace", emb, kernel, labels, norms=norms, drop="mask")
        assert np.abs(without["d_emb"][:2] - want_e[:2]).max() > 1e-2 * np.abs(want_e).max()
    else:
        # row 0: target cosine 0.995, inside the clamp, and theta - m scaler < eps: the clip of theta gives the target no slope;
        # row 1: target cosine 1, removed by the clamp as well
        theta = np.arccos(np.clip(ref["c_t"], -0.999, 0.999)) - 0.4 * ref["extras"]["margin_scaler"]
        assert abs(ref["c_t"][0] - 0.995) < 1e-6 and theta[0] < O.EPS and theta[1] < O.EPS and (ref["extras"]["margin_scaler"][:2] > 0.3).all()
        assert ref["slope"][:2].tolist() == [0.0, 0.0] and (ref["slope"][2:] > 0.9).all()
        assert ref["G"][0, 20] == 0.0 and ref["G"][1, 21] == 0.0
        without = GO.backward("AdaFace", emb, kernel, labels, norms=norms, drop="slope")
        assert np.abs(without["d_emb"][:2] - want_e[:2]).max() > 1e-2 * np.abs(want_e).max()


def test_sgd_oracle_matches_the_recording_and_torch():
    w0, grads = REF["sgd_w0"], REF["sgd_grads"]
    sgd = META["sgd"]
    p = torch.nn.Parameter(torch.from_numpy(w0.copy()))
    opt = torch.optim.SGD([p], lr=sgd["lr"], momentum=sgd["momentum"], weight_decay=sgd["weight_decay"])
    w, buf = w0, None
    for i, g in enumerate(grads):
        w, buf, norm = GO.sgd_step(w, g, buf, sgd["lr"], sgd["momentum"], sgd["weight_decay"], sgd["max_norm"])
        p.grad = torch.from_numpy(g.copy())
        t_norm = float(torch.nn.utils.clip_grad_norm_([p], sgd["max_norm"]))
        opt.step()
        assert abs(norm - REF["sgd_norms"][i]) <= 200 * O.U64 * norm and abs(norm - t_norm) <= 200 * O.U64 * norm
        assert np.abs(w - REF["sgd_w"][i]).max() <= 64 * O.U64 and np.abs(w - p.detach().numpy()).max() <= 64 * O.U64
    assert np.abs(buf - REF["sgd_buf"]).max() <= 64 * O.U64 * np.abs(buf).max()
    assert REF["sgd_norms"][0] > 5 > REF["sgd_norms"][-1]       # the clip is active on the first step and idle on the last


# ---- the C ABI, before any HIP call --------------------------------------------------------------------------------------------------
def _desc(**kw):
    d = _lib.HeadDesc()
    d.kind, d.b, d.d, d.c, d.s, d.m, d.h, d.t_alpha = 0, 4, 8, 5, 64.0, 0.35, 0.333, 1.0
    for f in ("emb", "norms", "label", "kernel", "wn", "col_norm", "ada_state"):
        setattr(d, f, 0x1000)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_abi_symbols_and_refusals(lib):
    for name in ("idb_head_grad_workspace_bytes", "idb_head_loss_grad", "idb_head_sgd_step"):
        assert hasattr(lib, name) and name in _lib.EXPORTS
    ws = 0x1000
    cases = [(dict(kind=3), b"loss kind"), (dict(b=0), b"b in 1.."), (dict(b=65537), b"b in 1.."), (dict(d=4097), b"d in 1.."),
             (dict(c=(1 << 20) + 1), b"c in 1.."), (dict(c=0), b"c in 1.."), (dict(kind=2, b=1), b"AdaFace needs b >= 2"),
             (dict(wn=None), b"not packed"), (dict(col_norm=None), b"not packed"), (dict(label=None), b"null pointer"),
             (dict(kind=2, norms=None), b"AdaFace needs norms"), (dict(s=0.0), b"s in"), (dict(t_alpha=1.5), b"t_alpha")]
    for kw, text in cases:
        d = _desc(**kw)
        assert lib.idb_head_loss_grad(C.byref(d), ws, ws, ws, ws, ws, ws, ws, ws, 1 << 40, None) == -1, kw
        assert text in lib.idb_last_error() and b"idb_head_loss_grad" in lib.idb_last_error(), (kw, lib.idb_last_error())
    d = _desc()
    for hole in range(7):                                     # each output pointer in turn
        outs = [ws] * 7
        outs[hole] = None
        assert lib.idb_head_loss_grad(C.byref(d), *outs, ws, 1 << 40, None) == -1 and b"null output" in lib.idb_last_error()
    fwd = lib.idb_head_workspace_bytes(4, 8, 5, None, None)
    need = lib.idb_head_grad_workspace_bytes(4, 8, 5, None, None, None)
    assert need > fwd > 0
    assert lib.idb_head_loss_grad(C.byref(d), ws, ws, ws, ws, ws, ws, ws, ws, fwd, None) == -1 and b"workspace too small" in lib.idb_last_error()
    assert lib.idb_head_loss_grad(C.byref(d), ws, ws, ws, ws, ws, ws, ws, ws + 4, need, None) == -1 and b"unaligned" in lib.idb_last_error()
    big = _desc(b=65536, d=4096, c=5)
    assert lib.idb_head_loss_grad(C.byref(big), ws, ws, ws, ws, ws, ws, ws, ws, 1 << 40, None) == -2
    assert b"2^27" in lib.idb_last_error()
    for shape in ((0, 8, 5), (4, 0, 5), (4, 8, 0), (65537, 8, 5), (4, 4097, 5), (4, 8, (1 << 20) + 1), (65536, 4096, 5)):
        assert lib.idb_head_grad_workspace_bytes(*shape, None, None, None) == 0

    def sgd(kernel=ws, grad=ws, buf=ws, d=8, c=5, lr=0.1, mom=0.9, wd=5e-4, mx=5.0, first=1, wn=ws, cn=ws, bad=ws, norm=ws, w=ws, wb=8192):
        return lib.idb_head_sgd_step(kernel, grad, buf, d, c, lr, mom, wd, mx, first, wn, cn, bad, norm, w, wb, None)

    for kw, text in [(dict(d=0), b"d in 1.."), (dict(c=(1 << 20) + 1), b"c in 1.."), (dict(kernel=None), b"null pointer"),
                     (dict(grad=None), b"null pointer"), (dict(buf=None), b"null pointer"), (dict(wn=None), b"null pointer"),
                     (dict(norm=None), b"null pointer"), (dict(lr=-1.0), b"lr in"), (dict(lr=float("nan")), b"lr in"), (dict(mom=1.0), b"momentum in"),
                     (dict(wd=-1e-3), b"weight_decay in"), (dict(mx=0.0), b"max_norm in"), (dict(wb=4096), b"workspace"), (dict(w=None), b"workspace"),
                     (dict(w=ws + 8), b"unaligned")]:
        assert sgd(**kw) == -1, kw
        assert text in lib.idb_last_error(), (kw, lib.idb_last_error())
    assert _lib.IDB_HEAD_SGD_WS_BYTES == 8192


def test_workspace_query_reports_the_grid(lib):
    """B = 130, C = 4099: two row tiles, several class blocks; D = 512: four chunks of 128 columns.  About 256 dX workgroups at
    the largest class counts, so the dX partials stay within blocks x B x D floats; B = 1024, C = 2^17, D = 512 is inside the limit."""
    rt, cb, ch = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    q = lambda *s: lib.idb_head_grad_workspace_bytes(*s, C.byref(rt), C.byref(cb), C.byref(ch))      # noqa: E731
    assert q(130, 512, 4099) > 0 and (rt.value, cb.value, ch.value) == (2, 33, 4)
    assert q(130, 130, 4099) > 0 and (rt.value, cb.value, ch.value) == (2, 33, 2)
    assert q(2, 7, 1) > 0 and (rt.value, cb.value, ch.value) == (1, 1, 1)
    assert q(37, 128, 301) > 0 and (rt.value, cb.value, ch.value) == (1, 3, 1)
    assert q(128, 512, 70722) > 0 and (rt.value, cb.value, ch.value) == (1, 185, 4)      # 553 class tiles, three per block
    n = q(1024, 512, 1 << 17)
    assert n > 0 and (rt.value, cb.value, ch.value) == (8, 32, 4)
    fwd = lib.idb_head_workspace_bytes(1024, 512, 1 << 17, None, None)
    assert fwd + 32 * 1024 * 512 * 4 <= n <= fwd + 32 * 1024 * 512 * 4 + 32 * 1024 * 8 + 1024      # O(blocks B D + B + C)
    assert q(128, 4096, 1 << 20) > 0 and cb.value == 256 and q(129, 4096, 1 << 20) > 0 and cb.value == 128
    assert q(65536, 2048, 1 << 20) > 0 and cb.value == 1 and q(65536, 2049, 1 << 20) == 0


# ---- Python ---------------------------------------------------------------------------------------------------------------------------
def test_python_refusals_and_names():
    for name in ("HeadGrad", "HeaderSGD", "train_header_step"):
        assert hasattr(H, name)
    assert H.HeadGrad._fields == ("embeddings", "kernel", "target_slope")
    hd = H.MarginHeader.from_synthetic(8, 4, 0, "CosFace")
    e, lab = torch.randn(3, 8), torch.tensor([0, 1, 2])
    with pytest.raises(ValueError, match="embeddings"):
        hd.loss_and_grad(torch.randn(3, 7), lab)
    with pytest.raises(ValueError, match="embeddings"):
        hd.loss_and_grad(torch.randn(8), lab)
    with pytest.raises(ValueError, match="label"):
        hd.loss_and_grad(e, torch.tensor([0, 1]))
    with pytest.raises(ValueError, match="label"):
        hd.loss_and_grad(e, torch.tensor([0, 4, 1]))
    with pytest.raises(ValueError, match="CosFace and ArcFace take"):
        hd.loss_and_grad(e, lab, norms=torch.ones(3))
    with pytest.raises(_lib.IdbError, match="not on a device"):       # valid arguments, but never packed: no silent CPU path
        hd.loss_and_grad(e, lab)
    ada = H.MarginHeader.from_synthetic(8, 4, 0, "AdaFace")
    with pytest.raises(ValueError, match="AdaFace takes"):
        ada.loss_and_grad(e, lab)
    with pytest.raises(ValueError, match="at least 2"):
        ada.loss_and_grad(e[:1], lab[:1], norms=torch.ones(1))
    with pytest.raises(ValueError, match="norms"):
        ada.loss_and_grad(e, lab, norms=torch.ones(2))
    for name in ("ElasticCosFace", "NonLinearHeader"):             # still refused
        with pytest.raises(NotImplementedError, match=name):
            H.MarginHeader.from_synthetic(8, 4, 0, name)
    with pytest.raises(NotImplementedError, match="training mode"):
        H.step_metrics(object(), hd, None, None, training=True)
    with pytest.raises(TypeError):
        H.HeaderSGD(object(), 0.1)
    for kw in (dict(lr=-0.1), dict(lr=0.1, momentum=1.0), dict(lr=0.1, weight_decay=-1.0), dict(lr=0.1, max_norm=0.0), dict(lr=float("nan"))):
        with pytest.raises(ValueError, match="HeaderSGD"):
            H.HeaderSGD(hd, **kw)
    opt = H.HeaderSGD(hd, 0.1)
    with pytest.raises(_lib.IdbError, match="not on a device"):
        opt.step(torch.zeros(8, 4))
    with pytest.raises(TypeError):
        H.train_header_step(hd, H.HeaderSGD(ada, 0.1), e, lab)       # an optimiser built on another header
    with pytest.raises(_lib.IdbError, match="not on a device"):
        H.train_header_step(hd, opt, e, lab)
    assert hd.grad_plan(3) == (1, 1, 1)
    with pytest.raises(ValueError, match="2\\^27"):
        H.MarginHeader.from_synthetic(4096, 4, 0, "CosFace").grad_plan(65536)


def test_header_sgd_bookkeeping_round_trips():
    hd = H.MarginHeader.from_synthetic(8, 4, 0, "CosFace")
    opt = H.HeaderSGD(hd, 0.1)
    assert (opt.lr, opt.momentum, opt.weight_decay, opt.max_norm, opt.steps) == (0.1, 0.9, 5e-4, 5.0, 0)     # train_FR.py:203-208, :293
    sd = opt.state_dict()
    assert sd == {"lr": 0.1, "momentum": 0.9, "weight_decay": 5e-4, "max_norm": 5.0, "steps": 0, "momentum_buffer": None}
    sd.update(lr=0.01, steps=3, momentum_buffer=torch.arange(32, dtype=torch.float32).reshape(8, 4))
    other = H.HeaderSGD(hd, 1.0, momentum=0.5)
    other.load_state_dict(sd)
    back = other.state_dict()
    assert (back["lr"], back["momentum"], back["steps"]) == (0.01, 0.9, 3) and torch.equal(back["momentum_buffer"], sd["momentum_buffer"])
    assert back["momentum_buffer"] is not sd["momentum_buffer"]
    for bad in (dict(momentum_buffer=None), dict(momentum_buffer=torch.zeros(4, 8)), dict(steps=0)):
        with pytest.raises(ValueError, match="HeaderSGD state dict"):
            other.load_state_dict({**sd, **bad})
    with pytest.raises(ValueError, match="without"):
        other.load_state_dict({"lr": 0.1})
    assert torch.equal(hd.state_dict()["kernel"], hd.kernel) and hd.state_dict()["kernel"] is not hd.kernel


# ---- preconditions of the GPU cases ---------------------------------------------------------------------------------------------------
def test_gpu_cases_stay_off_the_clamp_edges():
    """Every cosine of a gradient case is within 0.999 in float64 (AdaFace: 0.9989, its clamp is at 0.999), so no fp32 cosine sits on a
    clamp edge where 0 and 1 are both defensible; the clamp cases decide by a margin of 1e-3 or more."""
    for loss, B, Cn, D, (emb, kernel, labels, norms) in GO.all_gradient_inputs():
        ref = GO.backward(loss, emb, kernel, labels, norms=norms)
        assert np.abs(ref["r"]).max() <= (0.9989 if loss == "AdaFace" else 0.999), (loss, B, Cn, D, np.abs(ref["r"]).max())
    for kind in ("non_target", "target_clipped"):
        r = GO.backward("AdaFace", *GO.clamp_case(kind)[:3], norms=GO.clamp_case(kind)[3])["r"]
        assert ((np.abs(r) <= 0.998) | (np.abs(r) >= 0.9999)).all()


def test_gpu_cases_can_tell_a_missing_term():
    """Sensitivity precondition: for every input the GPU test checks per element (the whole shape matrix, the multi-tile blocks and the
    last-column labels: frhead_grad_oracle.all_gradient_inputs) and every term of the gradient the case can show
    (frhead_grad_oracle.terms_for: a single class shows only the one-hot, CosFace's target slope is 1, AdaFace has no row projection;
    the clamp mask belongs to the clamp cases), the oracle without that term differs from the true one by more than 4 x the case's GPU
    bound in some element."""
    seen_cases = 0
    for loss, B, Cn, D, (emb, kernel, labels, norms) in GO.all_gradient_inputs():
        ref = GO.backward(loss, emb, kernel, labels, norms=norms)
        serr = GO.scaler_err(B, norms, ref["extras"]) if loss == "AdaFace" else 0.0
        eb, kb = GO.grad_bounds(loss, B, Cn, D, ref, labels, GO.class_span(B, Cn), scaler_err=serr)
        for term in GO.terms_for(loss, Cn):
            bad = GO.backward(loss, emb, kernel, labels, norms=norms, drop=term)
            seen = (np.abs(bad["d_emb"] - ref["d_emb"]) > 4 * eb).any() or (np.abs(bad["d_kernel"] - ref["d_kernel"]) > 4 * kb).any()
            assert seen, (loss, B, Cn, D, term)
        seen_cases += 1
    assert seen_cases == len(GO.gpu_cases()) + len(GO.MULTI_TILE) + len(O.GPU_LOSSES) * len(GO.LAST_COLUMN_C) == 135 + 2 + 9
    for kind, term in (("non_target", "mask"), ("target_clipped", "slope")):
        emb, kernel, labels, norms = GO.clamp_case(kind)
        ref = GO.backward("AdaFace", emb, kernel, labels, norms=norms)
        eb, kb = GO.grad_bounds("AdaFace", 6, 33, 130, ref, labels, 128, scaler_err=GO.scaler_err(6, norms, ref["extras"]))
        bad = GO.backward("AdaFace", emb, kernel, labels, norms=norms, drop=term)
        assert (np.abs(bad["d_emb"] - ref["d_emb"]) > 4 * eb).any()
