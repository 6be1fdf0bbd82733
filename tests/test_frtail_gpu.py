"""The backbone's embedding stage on the GPU (frtail.EmbeddingStage, StageSGD, train_step; csrc/idb_tail.hip) per element against the
float64 oracle (tests/frtail_oracle.py, itself checked against float64 autograd and a recording of the reference's class in
test_frtail_cpu.py).  Every bound is derived, none is measured; the measured maxima are printed by the last test of the file.

u = 2^-24, v = 2^-53.  The derivations stand next to the code that evaluates them: frtail_oracle.forward_bounds (statistics in double;
the fp32 affine sc, sh, one rounding each; d = fl(fma(x, sc, sh) * fl(1 / (1 - p))); the products carry (K + 2) u sum |a||b| plus the
propagated operand error; the features statistics see the GPU's own z; f, norm and the unit row are formed in double and rounded once)
and frtail_oracle.backward_bounds.  The forward is checked against the oracle's forward from the inputs.  The backward is a function
of the cotangent and the saved context (z, f, norms, the two statistics); the GPU's context is itself checked element by element by
the forward test, and the backward is checked against the oracle's backward evaluated on that same stored context, so its bound is that
of the backward's own arithmetic: g_f and the BatchNorm1d sums in double ((n + 8) v, (B + 8) v), g_z rounded once (u), dgrad an fma
chain over n ((n + 2) u sum |g_z||W| + sum |dg_z||W|, then two roundings for the 1 / (1 - p) scale), the bn2 sums in double over the
fp32 g_y, d_x rounded once, wgrad an fma chain over the batch ((B + 2) u sum |g_z||d| + sum (|dg_z||d| + |g_z||dd|)).
Precondition tests for these inputs (conditioning of the statistics, the kept share, every term visible at 4x the bound) are in
test_frtail_cpu.py.
SGD: two fp32 roundings per state and step, propagated as frtail_oracle.sgd_bound states (test_header_sgd's form).
train_step: each step's loss against the float64 loop restarted from the GPU's own state (the bound is in that test's docstring).
"""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import frtail_oracle as TO  # noqa: E402

from faceposegenerator_amd import frhead as H  # noqa: E402
from faceposegenerator_amd import frtail as T  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MEASURED = {}
SEEN_PLANS = set()
GRADS = ("bn2.weight", "bn2.bias", "fc.weight", "fc.bias", "features.bias", "input")


def _note(what, err, bound):
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    ratio = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))))
    if what not in MEASURED or ratio > MEASURED[what][0]:
        MEASURED[what] = (ratio, float(np.max(err)))
    print(f"{what}: largest error {float(np.max(err)):.3e}, {ratio:.4f} of its bound")


def _close(what, got, want, bound):
    err = np.abs(np.asarray(got, dtype=np.float64) - want)
    _note(what, err, bound)
    assert (err <= bound).all(), (what, float(err.max()), float(np.max(bound)), float((err / np.maximum(bound, 1e-300)).max()))


def _sd(prm, ch, hw):
    sd = {k: torch.from_numpy(v.astype(np.float32)) for k, v in prm.items()}
    sd["fc.weight"] = torch.from_numpy(TO.to_upstream(prm["fc.weight"], ch, hw).astype(np.float32))
    return sd


def _stage(prm, ch, hw, p):
    return T.EmbeddingStage.from_state_dict(_sd(prm, ch, hw), dropout=p).to(DEV)


@functools.lru_cache(maxsize=None)
def _case(B, ch, hw, n, p):
    x, prm, keep, g = TO.case_inputs(B, ch, hw, n, p)
    fw = TO.forward(x, prm, keep, p)
    return x, prm, keep, g, fw, TO.forward_bounds(x, prm, fw)


def _xdev(x, B, hw, ch, dtype=torch.float32):
    return torch.from_numpy(x.astype(np.float32)).view(B, hw, ch).to(DEV, dtype)


def _keep_up(keep, ch, hw):
    return torch.from_numpy(TO.to_upstream(keep, ch, hw))


def _ctx_np(out):
    c = out._ctx
    return dict(emb=c["emb"].cpu().numpy().astype(np.float64), norm=c["norms"].cpu().numpy(), f=c["f"].cpu().numpy().astype(np.float64),
                z=c["z"].cpu().numpy().astype(np.float64), bn2_stat=c["bn2_stat"].cpu().numpy(), feat_stat=c["feat_stat"].cpu().numpy())


def _check_forward(tag, out, fw, fb):
    c = _ctx_np(out)
    _close(f"{tag} z", c["z"], fw["z"], fb["z"])
    _close(f"{tag} f", c["f"], fw["f"], fb["f"])
    _close(f"{tag} norms", c["norm"], fw["norm"], fb["norm"])
    _close(f"{tag} embeddings", out.embeddings.cpu().numpy(), fw["emb"], fb["emb"])
    _close(f"{tag} bn2 mean", c["bn2_stat"][0], fw["bn2_stat"][0], fb["bn2_mean"])
    _close(f"{tag} bn2 invstd", c["bn2_stat"][1], fw["bn2_stat"][1], fb["bn2_invstd"])
    _close(f"{tag} features mean", c["feat_stat"][0], fw["feat_stat"][0], fb["feat_mean"])
    _close(f"{tag} features invstd", c["feat_stat"][1], fw["feat_stat"][1], fb["feat_invstd"])
    return c


def _check_running(tag, stage, running, rb):
    for k, want in running.items():
        _close(f"{tag} {k}", stage.t[k].cpu().numpy(), want, rb[k])


def _grad_np(grad, B, K):
    return {"bn2.weight": grad.bn2_weight, "bn2.bias": grad.bn2_bias, "fc.weight": grad.fc_weight, "fc.bias": grad.fc_bias,
            "features.bias": grad.features_bias, "input": grad.input.reshape(B, K)}


@pytest.mark.parametrize("B,ch,hw,n,p", TO.gpu_cases(), ids=lambda v: str(v))
def test_forward_backward_against_oracle(lib, B, ch, hw, n, p):
    x, prm, keep, g, fw, fb = _case(B, ch, hw, n, p)
    K = hw * ch
    stage = _stage(prm, ch, hw, p)
    ks, rt = stage.plan(B)
    SEEN_PLANS.add((ks > 1, rt))
    assert rt == -(-B // 128) and (ks == 1) == (hw == 1)
    xd = _xdev(x, B, hw, ch)
    out = stage(xd, keep=None if p == 0 else _keep_up(keep, ch, hw))
    tag = f"[{ch},{hw},{n}]"
    ctx = _check_forward(tag, out, fw, fb)
    _check_running(f"{tag} after one call", stage, fw["running"], fb["running"])
    assert stage.tracked == {"bn2": 1, "features": 1}
    grad = stage.backward(out, torch.from_numpy(g).to(DEV))
    assert grad.fc_weight.dtype == torch.float32 and tuple(grad.fc_weight.shape) == (n, K) and tuple(grad.input.shape) == (B, hw, ch)
    bw = TO.backward(x, prm, keep, p, g, ctx)
    bb = TO.backward_bounds(x, prm, ctx, bw)
    got = _grad_np(grad, B, K)
    for k in GRADS:
        _close(f"{tag} d {k}", got[k].cpu().numpy(), bw[k], bb[k])
    assert torch.equal(grad.fc_weight_upstream(), torch.from_numpy(TO.to_upstream(grad.fc_weight.cpu().numpy(), ch, hw)).to(DEV))
    # the second call blends the running statistics once more, from the first call's fp32 values
    prm2 = dict(prm)
    prm2.update({k: stage.t[k].cpu().numpy().astype(np.float64) for k in fw["running"]})
    fw2 = TO.forward(x, prm2, keep, p)
    stage(xd, keep=None if p == 0 else _keep_up(keep, ch, hw))
    _check_running(f"{tag} after two calls", stage, fw2["running"], TO.forward_bounds(x, prm2, fw2)["running"])
    assert stage.state_dict()["bn2.num_batches_tracked"].item() == 2


def test_plans_cover_both_geometries(lib):
    """Runs after the matrix: one K slice and several occurred, and a second row tile."""
    for (B, ch, hw, n, p) in TO.gpu_cases():
        ks, rt = C.c_int32(0), C.c_int32(0)
        assert lib.idb_tail_workspace_bytes(B, ch, hw, n, C.byref(ks), C.byref(rt)) > 0
        SEEN_PLANS.add((ks.value > 1, rt.value))
    assert any(not many for many, _ in SEEN_PLANS) and any(many for many, _ in SEEN_PLANS) and any(rt == 2 for _, rt in SEEN_PLANS)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32], ids=str)
def test_forward_dtypes(lib, dtype):
    B, ch, hw, n, p = 37, 64, 49, 64, 0.4
    x, prm, keep, g, fw, fb = _case(B, ch, hw, n, p)
    xd = _xdev(x, B, hw, ch, dtype)
    assert np.array_equal(xd.float().cpu().numpy().reshape(B, -1).astype(np.float64), x)      # the dtype stores x exactly
    out = _stage(prm, ch, hw, p)(xd, keep=_keep_up(keep, ch, hw))
    _check_forward(f"{dtype}", out, fw, fb)


def test_eval_mode_against_oracle(lib):
    B, ch, hw, n, p = 37, 64, 49, 64, 0.4
    x, prm, keep, g, _, _ = _case(B, ch, hw, n, p)
    fw = TO.forward(x, prm, None, p, training=False)
    fb = TO.forward_bounds(x, prm, fw)
    stage = _stage(prm, ch, hw, p).eval()
    before = {k: v.clone() for k, v in stage.t.items()}
    out = stage(_xdev(x, B, hw, ch))
    _check_forward("eval", out, fw, fb)
    assert all(torch.equal(before[k], stage.t[k]) for k in before) and stage.tracked == {"bn2": 0, "features": 0}
    one = stage(_xdev(x, B, hw, ch)[:1])                       # a batch of one is accepted in eval mode
    assert torch.equal(one.embeddings, out.embeddings[:1])
    with pytest.raises(ValueError, match="eval-mode forward"):
        stage.backward(out, torch.from_numpy(g).to(DEV))


def test_eval_agrees_with_folded_backbone(lib):
    """stage.eval()(arc.features_map(x)) against F.normalize(arc(x)): the folded head computes the same function with bn2, fc and
    features in one fp32 matrix, so the two agree within the sum of the two paths' bounds: the stage's forward bound, and for the folded
    head (K + 2) u sum |x||Wf| for its chain plus u per folded weight and bias (sum |x| u |Wf| + u |bias|), propagated through the
    normalisation like the stage's |df|.  This holds only if features_map returns layer4's output and the NHWC column order is right."""
    from faceposegenerator_amd.arcface import ArcFace
    arc = ArcFace.from_synthetic("r18", seed=3).to(DEV)
    B = 4
    gi = np.arange(B * 3 * 112 * 112, dtype=np.int64)
    img = torch.from_numpy((((TO._h(gi, 511) - 255) / 255.0).astype(np.float32)).reshape(B, 3, 112, 112))
    fm = arc.features_map(img)
    assert tuple(fm.shape) == (B, 7, 7, 512) and fm.dtype == arc.tdt
    stage = T.EmbeddingStage.from_backbone(arc).to(DEV).eval()
    out = stage(fm)
    folded = torch.nn.functional.normalize(arc(img))
    x = fm.float().cpu().numpy().reshape(B, -1).astype(np.float64)
    prm = {k: v.cpu().numpy().astype(np.float64) for k, v in stage.t.items()}
    fw = TO.forward(x, prm, None, 0.4, training=False)
    fb = TO.forward_bounds(x, prm, fw)
    _close("eval vs oracle on the trunk's map", out.embeddings.cpu().numpy(), fw["emb"], fb["emb"])
    Wf = arc._fw["fc.w"].numpy().astype(np.float64)
    K = x.shape[1]
    ey = (K + 3) * TO.U32 * (np.abs(x) @ np.abs(Wf).T) + 2 * TO.U32 * np.abs(fw["f"]) + TO.U32 * np.abs(arc._fw["fc.b"].numpy())
    norm = fw["norm"]
    en = np.sqrt((ey ** 2).sum(1))
    e_folded = (ey / norm[:, None] + np.abs(fw["f"]) * (en / norm ** 2)[:, None] + 3 * TO.U32 * np.abs(fw["emb"])) * TO.SECOND
    _close("stage eval vs folded head", out.embeddings.cpu().numpy(), folded.cpu().numpy().astype(np.float64), fb["emb"] + e_folded)
    _close("folded head vs oracle", folded.cpu().numpy(), fw["emb"], e_folded)
    # the bounds are tight enough to see the likeliest silent bug: fc.weight's columns left in upstream's order c * hw + p
    wrong = dict(prm, **{"fc.weight": TO.to_upstream(prm["fc.weight"], 512, 49)})
    assert (np.abs(TO.forward(x, wrong, None, 0.4, training=False)["emb"] - fw["emb"]) > 4 * (fb["emb"] + e_folded)).any()


def test_renormalised_against_oracle(lib):
    B, ch, hw, n, p = 37, 64, 49, 64, 0.4
    x, prm, keep, g, fw, fb = _case(B, ch, hw, n, p)
    stage = _stage(prm, ch, hw, p)
    out = stage(_xdev(x, B, hw, ch), keep=_keep_up(keep, ch, hw))
    ctx = _ctx_np(out)
    grad = stage.backward(out, torch.from_numpy(g).to(DEV), renormalised=True)
    bw = TO.backward(x, prm, keep, p, g, ctx, renormalised=True)
    bb = TO.backward_bounds(x, prm, ctx, bw)
    got = _grad_np(grad, B, hw * ch)
    for k in GRADS:
        _close(f"renormalised d {k}", got[k].cpu().numpy(), bw[k], bb[k])
    plain = stage.backward(out, torch.from_numpy(g).to(DEV))
    assert not torch.equal(plain.fc_weight, grad.fc_weight)


def test_bit_identical_and_optional_input_grad(lib):
    B, ch, hw, n, p = 130, 128, 49, 192, 0.4
    x, prm, keep, g, _, _ = _case(B, ch, hw, n, p)
    xd, gd, ku = _xdev(x, B, hw, ch), torch.from_numpy(g).to(DEV), _keep_up(keep, ch, hw)
    outs, grads = [], []
    for _ in range(2):
        stage = _stage(prm, ch, hw, p)
        out = stage(xd, keep=ku)
        outs.append(out)
        grads.append(stage.backward(out, gd))
    for k in ("emb", "norms", "z", "f", "bn2_stat", "feat_stat", "affine"):
        assert torch.equal(outs[0]._ctx[k], outs[1]._ctx[k]), k
    for a, b in zip(grads[0][:6], grads[1][:6]):
        assert torch.equal(a, b)
    lean = stage.backward(outs[1], gd, need_input_grad=False)
    assert lean.input is None
    for a, b in zip(lean[:5], grads[1][:5]):
        assert torch.equal(a, b)
    drawn = []
    for _ in range(2):
        gen = torch.Generator(device=DEV).manual_seed(123)
        st = _stage(prm, ch, hw, p)
        o = st(xd, generator=gen)
        share = float(o._ctx["keep"].float().mean())
        assert 0.58 <= share <= 0.62                          # B K = 815 360 draws at 0.6: 6 sigma is 0.0033
        drawn.append((o.embeddings, o._ctx["keep"]))
    assert torch.equal(drawn[0][0], drawn[1][0]) and torch.equal(drawn[0][1], drawn[1][1])
    assert not torch.equal(drawn[0][0], outs[0].embeddings)


def _stage_np(stage):
    return [stage.t[k].cpu().numpy().astype(np.float64) for k in T.TRAINABLE]


def test_stage_sgd(lib):
    """Three steps at (64, 49, 64) against the float64 SGD fed the GPU's own gradients, the clip active, active, idle."""
    B, ch, hw, n, p = 37, 64, 49, 64, 0.4
    x, prm, keep, g, _, _ = _case(B, ch, hw, n, p)
    stage = _stage(prm, ch, hw, p)
    lr, mom, wd = 0.1, 0.9, 5e-4
    opt = T.StageSGD(stage, lr)
    out = stage(_xdev(x, B, hw, ch), keep=_keep_up(keep, ch, hw))
    grad = stage.backward(out, torch.from_numpy(g).to(DEV))
    gl = [grad.bn2_weight, grad.bn2_bias, grad.fc_weight, grad.fc_bias, grad.features_bias]
    base = float(torch.sqrt(sum((t.double() ** 2).sum() for t in gl)))
    ws, bufs = _stage_np(stage), None
    total = sum(w.size for w in ws)
    eb = [np.zeros_like(w) for w in ws]
    ew = [np.zeros_like(w) for w in ws]
    seen = []
    for step, want in enumerate((8.0, 6.0, 0.5)):
        scaled = [t * (want / base) for t in gl]
        sg = T.StageGrad(scaled[0], scaled[1], scaled[2], scaled[3], scaled[4], None, hw, ch)
        gs = [t.cpu().numpy().astype(np.float64) for t in scaled]
        ws, bufs, ref_norm = TO.sgd_step(ws, gs, bufs, lr, mom, wd, 5.0)
        norm = opt.step(sg)
        seen.append(norm)
        assert abs(norm - ref_norm) <= (total + 8) * TO.U64 * ref_norm
        coef = min(1.0, 5.0 / (ref_norm + 1e-6))
        have = _stage_np(stage)
        for i, k in enumerate(T.TRAINABLE):
            eb[i], ew[i] = TO.sgd_bound(ws[i], bufs[i], eb[i], ew[i], lr, mom, wd, coef * np.abs(gs[i]), total)
            _close(f"sgd {k}, step {step + 1}", have[i], ws[i], ew[i])
            _close(f"sgd momentum {k}, step {step + 1}", opt._buf[k].cpu().numpy(), bufs[i], eb[i])
    assert seen[0] > 5 and seen[1] > 5 and seen[2] < 5 and opt.steps == 3
    assert torch.equal(stage.t["features.weight"].cpu(), torch.ones(n))
    sd = opt.state_dict()
    again = T.StageSGD(stage, 0.5)
    again.load_state_dict(sd)
    assert again.lr == lr and again.steps == 3 and all(torch.equal(again._buf[k], opt._buf[k]) for k in T.TRAINABLE)


def _loop_step(x, prm, keep, p, labels, kernel, loss):
    """One float64 loop step's gradients from a given state: the stage's forward, the header's backward, the stage's backward."""
    import frhead_grad_oracle as GO
    fw = TO.forward(x, prm, keep, p)
    emb = fw["emb"]
    hb = GO.backward(loss, emb, kernel, labels)
    bw = TO.backward(x, prm, keep, p, hb["d_emb"], fw)
    return fw, hb, bw


def _manual_step(stage, header, opt_s, opt_h, xd, lab, ku):
    """The loop body through the public calls that are tested one by one: the sequence train_step must be."""
    out = stage(xd, keep=ku)
    ada = header.loss_name == "AdaFace"
    if ada:                                                   # the loop's literal lines
        norm = torch.norm(out.embeddings, 2, 1, True)
        hl, hg = header.loss_and_grad(torch.div(out.embeddings, norm), lab, norms=norm)
    else:
        hl, hg = header.loss_and_grad(out.embeddings, lab)
    grad = stage.backward(out, hg.embeddings, renormalised=ada)
    ns = opt_s.step(grad)
    nh = opt_h.step(hg.kernel)
    return {"loss": hl.loss, "acc": hl.acc, "correct": hl.correct, "grad_norm_stage": ns, "grad_norm_header": nh, "grad_input": grad.input}


def _same_state(a, b):
    """Two (stage, header, StageSGD, HeaderSGD) sets hold the same bits everywhere."""
    (sa, ha, osa, oha), (sb, hb, osb, ohb) = a, b
    for k in sa.t:
        assert torch.equal(sa.t[k], sb.t[k]), k
    assert sa.tracked == sb.tracked and osa.steps == osb.steps and oha.steps == ohb.steps
    for k in T.TRAINABLE:
        assert torch.equal(osa._buf[k], osb._buf[k]), k
    assert torch.equal(ha.kernel, hb.kernel) and torch.equal(oha._buf, ohb._buf)
    assert torch.equal(ha._state.cpu(), hb._state.cpu())


def test_train_step(lib):
    """Five CosFace steps at B = 37, 33 classes, (64, 49, 64), explicit masks, then one AdaFace step.
    Every step is checked twice.  (1) Against the float64 loop restarted from the GPU's own state before that step (stage tensors,
    running statistics, header kernel): the loss within the header's loss bound plus what the stage's forward bound on the embeddings
    adds (a cosine moves by at most 2 |d emb_i|_2 <= 2 sqrt(n) |d emb|_inf and the loss by at most twice the largest logit change:
    4 s sqrt(n) |d emb|_inf).  (2) Against a twin set of stage, header and optimisers that starts from the same state and takes the
    same step through the public calls the other tests check one by one against their oracles (stage(), header.loss_and_grad,
    stage.backward, StageSGD.step, HeaderSGD.step, with the loop's norm / div lines and renormalised=True for AdaFace): repeats are
    bit-identical, so loss, accuracy, both gradient norms, the input gradient, the five tensors, the running statistics, the header
    kernel and both momentum buffers must be equal bit for bit after every step.  That pins train_step's wiring (which gradient
    reaches which optimiser, the flag, the learning rates) without the header's Lipschitz constant in the embeddings.  The GPU's loss falls over the five steps, as the free-running float64 loop's does (asserted on the CPU)."""
    import frhead_oracle as HO
    B, ch, hw, n, p, Cn, lr = 37, 64, 49, 64, 0.4, 33, 0.05
    x, prm, keep, g, _, _ = _case(B, ch, hw, n, p)
    labels = (TO._h(np.arange(B) + 3, Cn)).astype(np.int64)
    kernel = ((TO._h(np.arange(n * Cn) + 13, 2001).reshape(n, Cn) - 1000) / 1000.0 * 0.05).astype(np.float32)
    xd, ku, lab = _xdev(x, B, hw, ch), _keep_up(keep, ch, hw), torch.from_numpy(labels)

    def fresh(loss):
        stage = _stage(prm, ch, hw, p)
        header = H.MarginHeader(torch.from_numpy(kernel), loss).to(DEV)
        return stage, header, T.StageSGD(stage, lr), H.HeaderSGD(header, 2 * lr)      # two learning rates: a swap would show

    one, two = fresh("CosFace"), fresh("CosFace")
    stage, header, opt_s, opt_h = one
    losses = []
    for step in range(5):
        state = {k: v.cpu().numpy().astype(np.float64) for k, v in stage.t.items()}
        kern = header.kernel.numpy().astype(np.float64)
        before = {k: stage.t[k].clone() for k in T.TRAINABLE}
        fw, hb, _ = _loop_step(x, state, keep, p, labels, kern, "CosFace")
        fb = TO.forward_bounds(x, state, fw)
        res = T.train_step(stage, header, opt_s, opt_h, xd, lab, keep=ku)
        ref = _manual_step(*two, xd, lab, ku)
        losses.append(res["loss"])
        lb = HO.lse_bound(n, Cn) + HO.target_bound("CosFace", n, hb["c_t"]).max() + (B + 2) * HO.U64 * 4 * HO.S \
            + 4 * HO.S * np.sqrt(n) * float(fb["emb"].max())
        print(f"train_step {step}: loss {res['loss']:.6f} (float64 from the same state {hb['loss']:.6f}, bound {lb:.2e}), "
              f"norms {res['grad_norm_stage']:.4f} {res['grad_norm_header']:.4f}")
        assert abs(res["loss"] - hb["loss"]) <= lb
        assert sorted(res) == sorted(ref)
        for k in ("loss", "acc", "correct", "grad_norm_stage", "grad_norm_header"):
            assert res[k] == ref[k], k
        assert tuple(res["grad_input"].shape) == (B, hw, ch) and torch.equal(res["grad_input"], ref["grad_input"])
        _same_state(one, two)
        assert all(not torch.equal(before[k], stage.t[k]) for k in T.TRAINABLE)           # the step was applied to all five
        assert not torch.equal(header.kernel, torch.from_numpy(kern.astype(np.float32)))
        assert 0 <= res["correct"] <= B and res["acc"] == H.multi_class_acc(res["correct"], B)
    assert losses[-1] < losses[0] and opt_s.steps == 5 and stage.tracked["bn2"] == 5
    # AdaFace, one step: the loop's norm / div lines and the second projection, against the twin
    one, two = fresh("AdaFace"), fresh("AdaFace")
    before = one[0].t["fc.weight"].clone()
    res = T.train_step(*one, xd, lab, keep=ku)
    ref = _manual_step(*two, xd, lab, ku)
    for k in ("loss", "acc", "correct", "grad_norm_stage", "grad_norm_header"):
        assert res[k] == ref[k], k
    assert torch.equal(res["grad_input"], ref["grad_input"])
    _same_state(one, two)
    assert np.isfinite(res["loss"]) and res["grad_norm_stage"] > 0 and not torch.equal(before, one[0].t["fc.weight"])


def test_refusals_after_launch(lib):
    B, ch, hw, n, p = 3, 64, 1, 64, 0.4
    x, prm, keep, g, _, _ = _case(B, ch, hw, n, p)
    stage = _stage(prm, ch, hw, p)
    xd, ku = _xdev(x, B, hw, ch), _keep_up(keep, ch, hw)
    bad = xd.clone()
    bad[1, 0, 5] = float("nan")
    before = {k: v.clone() for k, v in stage.t.items()}
    with pytest.raises(ValueError, match="non-finite"):
        stage(bad, keep=ku)
    # a refused call leaves the stage as it was
    assert all(torch.equal(before[k], stage.t[k]) for k in before) and stage.tracked == {"bn2": 0, "features": 0}
    with pytest.raises(ValueError, match="non-finite"):       # eval mode has no statistics launch: the per-row launch finds it
        stage.eval()(bad)
    stage.train()
    with pytest.raises(ValueError, match="batch of one"):
        stage(xd[:1])
    with pytest.raises(ValueError, match=r"keep: expected bool or uint8 \[3, 64\]"):
        stage(xd, keep=ku[:2])
    with pytest.raises(ValueError, match="keep: expected bool or uint8"):
        stage(xd, keep=ku.float())
    with pytest.raises(ValueError, match="keep: a dropout mask in eval mode"):
        stage.eval()(xd, keep=ku)
    stage.train()
    with pytest.raises(ValueError, match="no CPU fallback"):
        stage(xd.cpu(), keep=ku)
    flat = xd.clone()
    flat[:, :, 7] = 1.5
    zero_eps = T.EmbeddingStage.from_state_dict(_sd(prm, ch, hw), dropout=p, eps=0.0).to(DEV)
    with pytest.raises(ValueError, match="bn2 channel whose batch variance is exactly 0"):
        zero_eps(flat, keep=ku)
    sd = _sd(prm, ch, hw)
    sd["fc.weight"][9] = 0.0                                  # feature 9 is its bias for every sample
    zero_eps = T.EmbeddingStage.from_state_dict(sd, dropout=p, eps=0.0).to(DEV)
    with pytest.raises(ValueError, match="a feature whose batch variance is exactly 0"):
        zero_eps(xd, keep=ku)
    # backward and the optimiser
    out = stage(xd, keep=ku)
    gd = torch.from_numpy(g).to(DEV)
    with pytest.raises(ValueError, match=r"grad_embeddings: expected fp32 \[3, 64\]"):
        stage.backward(out, gd[:2])
    with pytest.raises(ValueError, match="grad_embeddings: expected fp32"):
        stage.backward(out, gd.double())
    other = _stage(prm, ch, hw, p)
    with pytest.raises(ValueError, match="not produced by this stage"):
        other.backward(out, gd)
    grad = stage.backward(out, gd)
    opt = T.StageSGD(stage, 0.1)
    with pytest.raises(ValueError, match="gradient of fc.bias expected fp32"):
        opt.step(grad._replace(fc_bias=grad.fc_bias[:5]))
    with pytest.raises(ValueError, match="gradient of bn2.weight expected fp32"):
        opt.step(grad._replace(bn2_weight=grad.bn2_weight.cpu()))
    with pytest.raises(TypeError, match="expected the StageGrad"):
        opt.step(grad.fc_weight)
    assert opt.steps == 0
    # "cuda" without an index is the current device
    plain = T.EmbeddingStage.from_state_dict(_sd(prm, ch, hw), dropout=p).to("cuda")
    assert torch.equal(plain(xd, keep=ku).embeddings, out.embeddings)


def test_print_measured(lib):
    """The largest error of each quantity as a share of its bound (for DESIGN 4.14); run the whole file to fill it."""
    groups = {}
    for what, (ratio, err) in MEASURED.items():
        key = what.split("] ")[-1] if "] " in what else what
        if key not in groups or ratio > groups[key][0]:
            groups[key] = (ratio, err)
    for key, (ratio, err) in sorted(groups.items()):
        print(f"measured {key}: {ratio:.4f} of the bound (largest error {err:.3e})")
    assert all(r <= 1.0 for r, _ in MEASURED.values())
