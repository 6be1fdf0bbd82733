"""The FR loss head's backward on the GPU: HeadGrad.embeddings and HeadGrad.kernel per element against the float64 oracle
(tests/frhead_grad_oracle.py, itself checked against autograd recordings of the reference's classes in test_frhead_grad_cpu.py), the
target slope, the optimiser step and the header's share of the loop body.  Every bound is derived, none is measured; the measured
maxima are printed by the last test of the file.  u = 2^-24, v = 2^-53, s = 64; the forward's bounds are those of test_frhead_gpu.py.

G, per entry (frhead_grad_oracle.g_bound).  Every logit the kernel's softmax sees is within delta of the oracle's: delta =
logit_bound(D) off the target, target_bound + 2^-18 on it (the forward's log-sum-exp saw the fp32 rounding of the target logit, and the
backward takes the same value, so the row's probabilities sum to 1).  A softmax entry is a ratio of sums of exponentials, each of which
moves by a factor within e^(+-delta): p_ij moves by a factor within e^(+-2 delta), and so does 1 - p_it = sum_{j != t} p_ij.  That is
the chain |dz| <= logit_bound, |dlse| <= lse_bound, |dp_ij| <= p_ij (exp(|dz| + |dlse|) - 1) with the two taken together, which keeps
the target's p - 1 relative to 1 - p where the logits are concerned.  The forward's sum itself has a relative error e_sum = 2^-17 + 4 u
+ (C + 300) v 4 s (fp32 differences and expf, double sums: test_frhead_gpu.py), which enters every p_ij as a factor and 1 - p_it as
p_it (exp(e_sum) - 1) -- absolute: a row whose target owns the softmax to within 1e-5 has no relative accuracy left in p - 1, here as
in any fp32 softmax.  Off the target the kernel evaluates expf of the fp32 rounding of z - lse (|z - lse| < 256: 2^-17; expf 4 u) and
multiplies by the fp32 s / B (2 u): |dG_ij| <= (s / B) p_ij (exp(2 delta + e_sum + 2^-17) - 1 + 6 u).  The target's entry is formed in
double, (p_t - 1) (s / B) d_t, and rounded once: |dG_it| <= (s / B) (|d(1 - p_t)| |d_t| + (1 - p_t) |dd_t| + u (1 - p_t) |d_t|).
The slope d_t = sin(acos(c) + m) / sqrt(1 - c^2) has derivative sin(m) / (1 - c^2)^1.5 in c, and the double target cosine is within
e = (4 D + 16) v of the oracle's: |dd_t| <= e |sin m| / (1 - (|c| + e)^2)^1.5 + 64 v / sqrt(1 - c^2) (AdaFace: m is m scaler, and
the scaler's own error enters through cos(t) / sqrt(1 - c^2) <= 1 / sqrt(1 - c^2)); every case keeps |c| <= 0.999 (asserted), near +-1
the slope is unbounded and no accuracy is claimed there.  Entries the clamp removes are exactly 0 on both sides.
Products.  dX_ik = sum_j G_ij Wn_jk is an fma chain over the classes of one block (K <= frhead_grad_oracle.class_span) with fp32
operands rounded once (2 u): |d dX_ik| <= sum_j |dG_ij| |w_jk| + (K + 2) u sum_j |G_ij| |w_jk|; the blocks are then added in double.
dW_jk = sum_i G_ij x_ik likewise over the B rows.  The projection scalars sum G_ij r_ij in double with the fp32 cosine r, within
(D + 4) u of the oracle's: |d<x_i, dX_i>| <= sum_j |dG_ij| + (D + 4) u sum_j |G_ij|, the same down a column.  Projection and division
are done in double and rounded once: |d d_emb_ik| <= (|d dX_ik| + |x_ik| |d<x_i, dX_i>|) / |e_i| + u |d_emb_ik|, and the same with w_j,
col_norm_j for d_kernel.  The factor 1.001 covers second-order terms.  At D = 512 the bound is about 1 % of a row's gradient scale.
SGD (test_header_sgd): the step is evaluated in double per element and each fp32 state is rounded once, so one step has two fp32
roundings per element, the momentum buffer's and the weight's, six in three steps; they propagate through
eb' <= momentum eb + wd ew + u |buf'|, ew' <= ew + lr eb' + u |w'| (+ (D C + 16) v |coef g| for the norm inside coef, 1e-13 relative
for the double arithmetic).
train_header_step: each step is checked against the float64 loop restarted from the GPU's own state before that step (its kernel and
momentum buffer): the loss within the forward's loss bound, the stepped kernel within the step bound that the gradient bound kb
propagates to: |d coef| <= max_norm |kb|_2 / (|g|_2 - |kb|_2 + 1e-6)^2, |dd| <= coef kb + |g| |d coef| + |d coef| kb, then the two
roundings.  (A bound against the free-running float64 loop would need a Lipschitz constant of the gradient in the kernel; the
free-running loop is run as well, for the requirement that its loss falls.)
"""
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import frhead_grad_oracle as GO  # noqa: E402
import frhead_oracle as O  # noqa: E402

from faceposegenerator_amd import frhead as H  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MEASURED = {}                                                 # (what, loss, D) -> (largest error / bound, largest error)


def _note(what, loss, D, err, bound):
    ratio = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))))
    key = (what, loss, D)
    if key not in MEASURED or ratio > MEASURED[key][0]:
        MEASURED[key] = (ratio, float(np.max(err)))


def _kw(loss, norms):
    return dict(norms=torch.from_numpy(norms)) if loss == "AdaFace" else {}


def _header(loss, kernel, **kw):
    return H.MarginHeader(torch.from_numpy(np.ascontiguousarray(kernel)), loss, **kw).to(DEV)


@functools.lru_cache(maxsize=None)
def _reference(loss, B, Cn, D):
    emb, kernel, labels, norms = GO.case_inputs(loss, B, Cn, D)
    return emb, kernel, labels, norms, GO.backward(loss, emb, kernel, labels, norms=norms)


def _check(loss, D, header, emb, labels, norms, ref, tag=None, clamp_edges=True):
    """loss_and_grad against the oracle `ref`; returns (HeadLoss, HeadGrad)."""
    B, Cn = ref["p"].shape
    if clamp_edges:
        assert np.abs(ref["r"]).max() <= (0.9989 if loss == "AdaFace" else 0.999)
    t_emb, t_lab = torch.from_numpy(emb), torch.from_numpy(labels)
    out, grad = header.loss_and_grad(t_emb, t_lab, **_kw(loss, norms))
    assert grad.embeddings.dtype == torch.float32 and tuple(grad.embeddings.shape) == (B, D) and grad.embeddings.is_cuda
    assert grad.kernel.dtype == torch.float32 and tuple(grad.kernel.shape) == (D, Cn) and grad.kernel.is_contiguous()
    assert grad.target_slope.dtype == torch.float64 and tuple(grad.target_slope.shape) == (B,)
    rt, cb, ch = header.grad_plan(B)
    assert (rt, cb, ch) == (-(-B // 128), -(-Cn // GO.class_span(B, Cn)), -(-D // 128))
    serr = GO.scaler_err(B, norms, ref["extras"]) if loss == "AdaFace" else 0.0
    eb, kb = GO.grad_bounds(loss, B, Cn, D, ref, labels, GO.class_span(B, Cn), scaler_err=serr)
    e_err = np.abs(grad.embeddings.cpu().numpy().astype(np.float64) - ref["d_emb"])
    k_err = np.abs(grad.kernel.cpu().numpy().astype(np.float64) - ref["d_kernel"])
    tag = tag or loss
    _note("d_emb", tag, D, e_err, eb)
    _note("d_kernel", tag, D, k_err, kb)
    assert (e_err <= eb).all(), (e_err.max(), eb.max(), (e_err / np.maximum(eb, 1e-300)).max())
    assert (k_err <= kb).all(), (k_err.max(), kb.max(), (k_err / np.maximum(kb, 1e-300)).max())
    sb = GO.slope_bound(loss, D, ref, scaler_err=serr)
    s_err = np.abs(grad.target_slope.cpu().numpy() - ref["slope"])
    if clamp_edges:
        _note("target slope", tag, D, s_err, sb + 1e-300)
        assert (s_err <= sb).all(), (s_err.max(), sb.max())
    assert abs(out.loss - ref["loss"]) <= O.lse_bound(D, Cn) + O.target_bound(loss, D, ref["c_t"], scaler_err=serr).max() + (B + 2) * O.U64 * 4 * O.S
    return out, grad


# ---- every shape, every loss ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss,B,Cn,D", GO.gpu_cases(), ids=lambda v: str(v))
def test_gradients_against_oracle(lib, loss, B, Cn, D):
    emb, kernel, labels, norms, ref = _reference(loss, B, Cn, D)
    header = _header(loss, kernel)
    rt, cb, ch = header.grad_plan(B)
    if B == 130:
        assert rt == 2                                        # a second, partial row tile
    if Cn == 4099:
        assert cb == 33                                       # several class blocks, the last of three classes
    assert ch == {7: 1, 130: 2, 512: 4}[D]                    # scalar tail; unaligned rows and a 2-column last chunk; the vector path
    _, grad = _check(loss, D, header, emb, labels, norms, ref)
    if Cn == 1:                                               # a single class: the softmax is 1, p - onehot is 0
        assert not grad.embeddings.any() and not grad.kernel.any()


# column blocks of several class tiles: past 256 workgroups per D chunk a block takes two tiles (loss, B, C, D, classes per block)
MULTI_TILE = GO.MULTI_TILE


@pytest.mark.parametrize("loss,B,Cn,D,span", MULTI_TILE, ids=lambda v: str(v))
def test_multi_tile_class_blocks(lib, loss, B, Cn, D, span):
    assert GO.class_span(B, Cn) == span                       # 257 (129) class tiles over at most 256 (128) workgroups: two per block
    emb, kernel, labels, norms, ref = _reference(loss, B, Cn, D)
    header = _header(loss, kernel)
    assert header.grad_plan(B)[1] == -(-Cn // span) < -(-Cn // 128)
    _check(loss, D, header, emb, labels, norms, ref, tag=f"{loss} two-tile blocks")


@pytest.mark.parametrize("loss", O.GPU_LOSSES)
@pytest.mark.parametrize("Cn", GO.LAST_COLUMN_C)
def test_label_in_the_last_column_of_the_last_partial_tile(lib, loss, Cn):
    B, D = GO.LAST_COLUMN_BD
    emb, kernel, labels, norms = GO.last_column_inputs(loss, Cn)
    ref = GO.backward(loss, emb, kernel, labels, norms=norms)
    _, grad = _check(loss, D, _header(loss, kernel), emb, labels, norms, ref, tag=loss + " last column")
    assert grad.kernel[:, Cn - 1].abs().max().item() > 0


# ---- reproducibility, forward parity ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss", O.GPU_LOSSES)
def test_repeats_are_bit_identical_and_the_forward_half_is_header_loss(lib, loss):
    B, Cn, D = 130, 4099, 130
    emb, kernel, labels, norms, _ = _reference(loss, B, Cn, D)
    t_emb, t_lab, kw = torch.from_numpy(emb), torch.from_numpy(labels), _kw(loss, norms)
    header, fresh = _header(loss, kernel, t_alpha=0.3), _header(loss, kernel, t_alpha=0.3)
    out, grad = header.loss_and_grad(t_emb, t_lab, **kw)
    want = fresh.loss(t_emb, t_lab, **kw)
    for a, b in zip(out, want):
        assert torch.equal(a, b) if torch.is_tensor(a) else a == b
    if loss == "AdaFace":                                     # exactly one EMA step per call: 0.3 of the batch statistics, 0.7 of (20, 100)
        assert (header.batch_mean, header.batch_std) == (fresh.batch_mean, fresh.batch_std) and header.batch_mean != 20.0
        header.set_buffers(20.0, 100.0)
    out2, grad2 = header.loss_and_grad(t_emb, t_lab, **kw)
    assert torch.equal(grad.embeddings, grad2.embeddings) and torch.equal(grad.kernel, grad2.kernel)
    assert torch.equal(grad.target_slope, grad2.target_slope) and torch.equal(out.per_sample, out2.per_sample)


# ---- AdaFace at its clamp and clip ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["non_target", "target_clipped"])
def test_adaface_clamp_and_clip(lib, kind):
    """non_target: a column along (against) an embedding reads cosine +-1 against the 0.999 clamp; that entry passes nothing on, neither
    to its row of d_emb nor to its column of d_kernel.  target_clipped: theta - m scaler < eps, so the target's term is exactly 0 and the
    rest of the row's gradient stands.  Against the oracle and against the autograd recording (which the oracle matches to 1e-7 of the
    largest gradient at the very most: test_frhead_grad_cpu.py)."""
    B, Cn, D = 6, 33, 130
    emb, kernel, labels, norms = GO.clamp_case(kind)
    ref = GO.backward("AdaFace", emb, kernel, labels, norms=norms)
    _, grad = _check("AdaFace", D, _header("AdaFace", kernel), emb, labels, norms, ref, tag="AdaFace " + kind, clamp_edges=False)
    rec = np.load(os.path.join(GOLD, "frhead_grad_reference.npz"))
    eb, kb = GO.grad_bounds("AdaFace", B, Cn, D, ref, labels, 128, scaler_err=GO.scaler_err(B, norms, ref["extras"]))
    ge, gk = grad.embeddings.cpu().numpy().astype(np.float64), grad.kernel.cpu().numpy().astype(np.float64)
    want_e, want_k = rec[f"clamp_{kind}_d_emb"], rec[f"clamp_{kind}_d_kernel"]
    assert (np.abs(ge - want_e) <= eb + 1e-7 * np.abs(want_e).max()).all() and (np.abs(gk - want_k) <= kb + 1e-7 * np.abs(want_k).max()).all()
    slope = grad.target_slope.cpu().numpy()
    if kind == "non_target":
        assert ref["G"][0, 2] == 0.0 and ref["G"][1, 3] == 0.0
        assert np.abs(gk[:, [2, 3]]).max() <= 1e-6 * np.abs(gk).max()      # 9e-10 in float64: nothing from rows 0 and 1
    else:
        assert slope[:2].tolist() == [0.0, 0.0] and (slope[2:] > 0.9).all()
        without = GO.backward("AdaFace", emb, kernel, labels, norms=norms, drop="slope")
        assert (np.abs(without["d_emb"][:2] - ref["d_emb"][:2]) > 4 * eb[:2]).any()     # the target's term would have been visible


def test_a_target_cosine_of_exactly_one_is_refused_under_arcface(lib):
    """D = 1: every cosine is +-1 exactly in double, 1 - c^2 is 0 and the slope is not finite (upstream: inf / NaN gradients)."""
    header = _header("ArcFace", np.array([[4.0, -1.0, 0.5]], dtype=np.float32))
    with pytest.raises(ValueError, match="exactly"):
        header.loss_and_grad(torch.tensor([[2.0], [3.0]]), torch.tensor([0, 1]))
    out, grad = _header("CosFace", np.array([[4.0, -1.0, 0.5]], dtype=np.float32)).loss_and_grad(torch.tensor([[2.0], [3.0]]), torch.tensor([0, 1]))
    assert grad.target_slope.tolist() == [1.0, 1.0] and math.isfinite(out.loss)
    emb, kernel, labels, norms = GO.case_inputs("CosFace", 4, 33, 130)
    e = torch.from_numpy(emb.copy())
    e[2] = 0.0
    with pytest.raises(ValueError, match="zero or non-finite row"):
        _header("CosFace", kernel).loss_and_grad(e, torch.from_numpy(labels))


# ---- the optimiser ----------------------------------------------------------------------------------------------------------------------
def _step_bound(w_new, buf_new, g_abs, eb, ew, lr, momentum, wd, d_err=0.0):
    """The two fp32 roundings of one step, with the errors eb, ew the states carried in and d_err of the clipped gradient; g_abs =
    |coef g|, on which the norm's (n + 16) v relative error acts through coef."""
    rel = (buf_new.size + 16) * O.U64
    eb = (momentum * eb + wd * ew + d_err + rel * g_abs) * (1 + 1e-12) + (O.U32 + 1e-13) * np.abs(buf_new)
    ew = ew + lr * eb + (O.U32 + 1e-13) * np.abs(w_new)
    return eb, ew


def test_header_sgd(lib):
    """Three steps on (D, C) = (130, 301) against torch's SGD and clip_grad_norm_ in float64 on the CPU, fed the GPU's own fp32 gradients."""
    B, Cn, D = 37, 301, 130
    emb, kernel, labels, norms, _ = _reference("ArcFace", B, Cn, D)
    t_emb, t_lab = torch.from_numpy(emb), torch.from_numpy(labels)
    header = _header("ArcFace", kernel)
    lr, mom, wd = 0.1, 0.9, 5e-4
    opt = H.HeaderSGD(header, lr)
    p = torch.nn.Parameter(torch.from_numpy(kernel).double())
    ref_opt = torch.optim.SGD([p], lr=lr, momentum=mom, weight_decay=wd)
    eb = ew = np.zeros((D, Cn))
    norms_seen = []
    for step, want_norm in enumerate((8.0, 6.0, 0.5)):
        _, grad = header.loss_and_grad(t_emb, t_lab)
        g = grad.kernel * (want_norm / float(grad.kernel.double().norm()))
        p.grad = g.cpu().double()
        ref_norm = float(torch.nn.utils.clip_grad_norm_([p], 5.0))
        ref_opt.step()
        norm = opt.step(g)
        norms_seen.append(norm)
        assert abs(norm - ref_norm) <= (D * Cn + 8) * O.U64 * ref_norm
        w_ref, buf_ref = p.detach().numpy(), ref_opt.state[p]["momentum_buffer"].numpy()
        eb, ew = _step_bound(w_ref, buf_ref, min(1.0, 5.0 / (ref_norm + 1e-6)) * np.abs(p.grad.numpy()), eb, ew, lr, mom, wd)
        w_err = np.abs(header.kernel.numpy().astype(np.float64) - w_ref)
        b_err = np.abs(opt.state_dict()["momentum_buffer"].numpy().astype(np.float64) - buf_ref)
        _note(f"sgd weight, step {step + 1}", "ArcFace", D, w_err, ew)
        _note(f"sgd momentum, step {step + 1}", "ArcFace", D, b_err, eb)
        assert (w_err <= ew).all() and (b_err <= eb).all(), (w_err.max(), ew.max(), b_err.max(), eb.max())
        # the repack happened: the stepped header computes what a fresh header built from its state dict computes, bit for bit
        assert torch.equal(header.state_dict()["kernel"], header.kernel) and opt.steps == step + 1
        fresh = H.MarginHeader.from_state_dict(header.state_dict(), "ArcFace").to(DEV)
        assert torch.equal(header(t_emb, t_lab), fresh(t_emb, t_lab))
        assert not torch.equal(header.kernel, torch.from_numpy(kernel))
    assert norms_seen[0] > 5 and norms_seen[1] > 5 and norms_seen[2] < 5      # the clip is active, active, idle


def test_train_header_step(lib):
    """Five steps with CosFace on B = 37, C = 33, D = 130.  Each step against the float64 loop restarted from the GPU's own state; the
    free-running float64 loop's loss falls, and so does the GPU's."""
    B, Cn, D, lr, mom, wd, mx = 37, 33, 130, 0.02, 0.9, 5e-4, 5.0
    emb, kernel, labels, norms = GO.case_inputs("CosFace", B, Cn, D)
    t_emb, t_lab = torch.from_numpy(emb), torch.from_numpy(labels)
    w, buf, free = kernel.astype(np.float64), None, []
    for _ in range(5):                                        # float64 forward, float64 SGD, no GPU
        ref = GO.backward("CosFace", emb, w, labels)
        free.append(ref["loss"])
        w, buf, _n = GO.sgd_step(w, ref["d_kernel"], buf, lr, mom, wd, mx)
    assert free[4] < free[0] - 0.05 and all(b < a for a, b in zip(free, free[1:]))
    header = _header("CosFace", kernel)
    opt = H.HeaderSGD(header, lr, momentum=mom, weight_decay=wd, max_norm=mx)
    got = []
    for step in range(5):
        k_before = header.kernel.numpy().copy()
        buf_before = None if step == 0 else opt.state_dict()["momentum_buffer"].numpy().astype(np.float64)
        ref = GO.backward("CosFace", emb, k_before, labels)
        out = H.train_header_step(header, opt, t_emb, t_lab)
        assert sorted(out) == ["acc", "correct", "grad_embeddings", "grad_norm", "loss"]
        got.append(out["loss"])
        loss_bound = O.lse_bound(D, Cn) + O.target_bound("CosFace", D, ref["c_t"]).max() + (B + 2) * O.U64 * 4 * O.S
        _note("train step loss", "CosFace", D, np.array(abs(out["loss"] - ref["loss"])), np.array(loss_bound))
        assert abs(out["loss"] - ref["loss"]) <= loss_bound
        assert out["acc"] == O.multi_class_acc(np.full(B, 1) * (np.arange(B) < out["correct"]), np.ones(B))
        eb, kb = GO.grad_bounds("CosFace", B, Cn, D, ref, labels, GO.class_span(B, Cn))
        assert (np.abs(out["grad_embeddings"].cpu().numpy() - ref["d_emb"]) <= eb).all()
        w_ref, buf_ref, n_ref = GO.sgd_step(k_before, ref["d_kernel"], buf_before, lr, mom, wd, mx)
        kb2 = math.sqrt(float((kb * kb).sum()))
        assert abs(out["grad_norm"] - n_ref) <= kb2 + 1e-12 * n_ref
        d_coef = mx * kb2 / (n_ref - kb2 + 1e-6) ** 2
        d_err = min(1.0, mx / (n_ref + 1e-6)) * kb + np.abs(ref["d_kernel"]) * d_coef + d_coef * kb
        sb, sw = _step_bound(w_ref, buf_ref, np.abs(ref["d_kernel"]), 0.0, 0.0, lr, mom, wd, d_err)
        w_err = np.abs(header.kernel.numpy().astype(np.float64) - w_ref)
        _note("train step kernel", "CosFace", D, w_err, sw)
        assert (w_err <= sw).all(), (step, w_err.max(), sw.max())
        assert (np.abs(opt.state_dict()["momentum_buffer"].numpy() - buf_ref) <= sb).all()
    assert got[4] < got[0] - 0.05 and opt.steps == 5


def test_zz_report_measured_maxima():
    """Prints the largest error of every checked quantity over the tests above as a fraction of its derived bound (DESIGN.md 4.13
    records them)."""
    for (what, loss, D), (ratio, err) in sorted(MEASURED.items()):
        print(f"measured {what:24s} {loss:26s} D={D:4d}: {ratio:.3e} of its bound (largest error {err:.3e})")
    assert all(ratio <= 1.0 for ratio, _ in MEASURED.values())
