"""Float64 restatement of the backbone's trunk in training (faceposegenerator_amd/frtrunk.py, csrc/idb_block.hip): IBasicBlock and the
stem, forward and backward, with the per-element bounds the GPU tests hold the kernels to and the seed-free case inputs the recorder
and both test files rebuild.  The convolutions are torch's float64 CPU convolutions.

Everything is in the DEVICE layout: activations NHWC [B, H, W, C]; conv weights [cout, ky, kx, cin] (`w_to_upstream` / `w_to_device`
convert to and from upstream's [cout, cin, ky, kx]).  Parameter keys are upstream's without a prefix (bn1.weight, conv1.weight, ...,
downsample.0.weight, downsample.1.weight).

`omit` names a term to leave out (tests: the comparisons must be able to see every term):
  "bn_mean_term", "bn_xhat_term", "prelu_bwd", "identity", "pad_zero" (the padded taps read the BatchNorm's shift instead of 0).

Bounds.  u = 2^-24, v = 2^-53, SECOND = 1 + 2^-10 for products of two first-order terms, as in frtail_oracle.
  Statistics over R rows from values carrying an error ec (0 for the block's input): |d mean| <= mean(ec) + (R + 4) v spread,
  |d var| <= (2 / R) sum |c - mean| (ec + |d mean|) + (2 R + 16) v spread^2, d invstd = invstd^3 |d var| / 2 + 4 v invstd.
  sc = fl(gamma invstd), sh = fl(beta - mean gamma invstd): one rounding each on top of the statistics' terms.
  y = fma(c, sc, sh): |dy| <= |c| |d sc| + |d sh| + |sc| ec + u |y|.  PReLU: the slope's product is one more rounding; where |y| <= |dy|
  the two sides may take different branches, which differ by at most (1 + |slope|) |dy| there.
  A product is an fma chain of K terms (K = taps cin, taps cout, or the rows of a wgrad slice, whose slices meet in double and are
  rounded once): (K + 2) u sum |a| |b| + sum |da| |b| + sum |a| |db|.
  The backward is a function of stored values (the context) on both sides, so only the kernels' arithmetic is bounded: the sums run in
  double ((R + 8) v relative to the sums of magnitudes), every stored fp32 value is rounded once, and a recomputed activation differs
  from the oracle's by its own roundings (no branch can differ: fma(c, sc, sh) and its double evaluation have the same sign).
No bound is measured.
"""
import numpy as np
import torch
import torch.nn.functional as F

from frtail_oracle import SECOND, U32, U64, _h

EPS, MOMENTUM = 1e-5, 0.1


def w_to_upstream(w):
    return np.ascontiguousarray(np.transpose(w, (0, 3, 1, 2)))


def w_to_device(w):
    return np.ascontiguousarray(np.transpose(w, (0, 2, 3, 1)))


def _nchw(a):
    return torch.from_numpy(np.ascontiguousarray(np.transpose(a, (0, 3, 1, 2))))


def _nhwc(t):
    return np.ascontiguousarray(t.numpy().transpose(0, 2, 3, 1))


def _pad(w):
    return 1 if w.shape[1] == 3 else 0


def conv_fwd(a, w, stride):
    return _nhwc(F.conv2d(_nchw(a), torch.from_numpy(w_to_upstream(w)), stride=stride, padding=_pad(w)))


def conv_dgrad(g, w, stride, in_shape):
    B, H, W, cin = in_shape
    return _nhwc(torch.nn.grad.conv2d_input((B, cin, H, W), torch.from_numpy(w_to_upstream(w)), _nchw(g), stride=stride, padding=_pad(w)))


def conv_wgrad(g, a, w_shape, stride):
    cout, k, _, cin = w_shape
    return w_to_device(torch.nn.grad.conv2d_weight(_nchw(a), (cout, cin, k, k), _nchw(g), stride=stride, padding=1 if k == 3 else 0).numpy())


# ---- inputs: integer arithmetic only, no RNG ---------------------------------------------------------------------------------------
def _u(shape, salt, mod=2001):
    """Hashed values in [-1, 1] of a shape."""
    n = int(np.prod(shape))
    return ((_h(np.arange(n, dtype=np.int64) * 3 + salt, mod) - (mod // 2)) / float(mod // 2)).reshape(shape)


def _bn_params(prm, key, ch, salt, big_shift=False, damp=1.0):
    """The ranges of arcface.synth_weights: gammas 0.8-1.2 (bn3 damped), shifts non-zero (large for bn1), running variances 0.5-2."""
    idx = np.arange(ch)
    sign = np.where(_h(idx + salt, 2) == 0, -1.0, 1.0)
    prm[f"{key}.weight"] = damp * (0.8 + 0.4 * _h(idx + salt + 3, 101) / 100.0)
    mag = (0.5 + 1.5 * _h(idx + salt + 11, 81) / 80.0) if big_shift else (0.05 + 0.2 * _h(idx + salt + 11, 81) / 80.0)
    prm[f"{key}.bias"] = sign * mag
    prm[f"{key}.running_mean"] = (_h(idx + salt + 23, 41) - 20) / 100.0
    prm[f"{key}.running_var"] = 0.5 + 1.5 * _h(idx + salt + 29, 51) / 50.0


def _f32(prm):
    return {k: np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64) for k, a in prm.items()}


def has_downsample(cin, planes, stride):
    return stride != 1 or cin != planes


def case_inputs(B, cin, planes, H, W, stride, downsample=None):
    """x [B, H, W, cin] (per-channel scales and offsets, so that no channel is nearly constant), the parameters (fp32 values, conv
    weights ~ sqrt(3 / fan_in) uniform, in the device layout), g [B, Ho, Wo, planes]."""
    ds = has_downsample(cin, planes, stride) if downsample is None else downsample
    scale = 0.5 + 1.5 * (_h(np.arange(cin) + 17, 97) / 96.0)
    shift = (_h(np.arange(cin) + 5, 61) - 30) / 20.0
    x = _u((B, H, W, cin), 1000003 * (B + H) + stride) * 2.0 * scale + shift
    prm = {}
    _bn_params(prm, "bn1", cin, 7, big_shift=True)
    prm["conv1.weight"] = _u((planes, 3, 3, cin), 101) * np.sqrt(3.0 / (9 * cin))
    _bn_params(prm, "bn2", planes, 13)
    prm["prelu.weight"] = 0.05 + 0.35 * _h(np.arange(planes) + 19, 71) / 70.0
    prm["conv2.weight"] = _u((planes, 3, 3, planes), 211) * np.sqrt(3.0 / (9 * planes))
    _bn_params(prm, "bn3", planes, 31, damp=0.15)
    if ds:
        prm["downsample.0.weight"] = _u((planes, 1, 1, cin), 307) * np.sqrt(3.0 / cin)
        _bn_params(prm, "downsample.1", planes, 41)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    g = _u((B, Ho, Wo, planes), 91 + B, 513) / B
    return x.astype(np.float32).astype(np.float64), _f32(prm), g.astype(np.float32).astype(np.float64)


def stem_inputs(B, H, W):
    """images [B, 3, H, W] in [-1, 1] (NCHW, as the augmentation hands them out), the stem's parameters, g [B, H, W, 64]."""
    img = _u((B, 3, H, W), 4242 + B + H)
    prm = {"conv1.weight": _u((64, 3, 3, 3), 55) * np.sqrt(3.0 / 27)}
    _bn_params(prm, "bn1", 64, 61)
    prm["prelu.weight"] = 0.05 + 0.35 * _h(np.arange(64) + 67, 71) / 70.0
    g = _u((B, H, W, 64), 191 + B, 513) / B
    return img.astype(np.float32).astype(np.float64), _f32(prm), g.astype(np.float32).astype(np.float64)


# (B, cin, planes, H, W, stride): the smallest cases that reach each thing that can go wrong
BLOCK_CASES = ((2, 64, 64, 8, 8, 1), (3, 64, 128, 7, 7, 2), (2, 64, 64, 8, 8, 2), (2, 128, 128, 4, 4, 1), (4, 64, 64, 1, 1, 1),
               (5, 64, 64, 12, 12, 1))
STEM_CASE = (2, 8, 8)


# ---- pieces ------------------------------------------------------------------------------------------------------------------------
def bn_forward(c, prm, key, training=True, eps=EPS, momentum=MOMENTUM):
    """-> stat [2, ch] (mean, invstd), affine [2, ch] (sc, sh), var, the new running statistics (None in eval)."""
    ch = c.shape[-1]
    cr = c.reshape(-1, ch)
    R = cr.shape[0]
    if training:
        mean, var = cr.mean(0), cr.var(0)
        running = {f"{key}.running_mean": (1 - momentum) * prm[f"{key}.running_mean"] + momentum * mean,
                   f"{key}.running_var": (1 - momentum) * prm[f"{key}.running_var"] + momentum * var * (R / (R - 1.0))}
    else:
        mean, var, running = prm[f"{key}.running_mean"], prm[f"{key}.running_var"], None
    inv = 1.0 / np.sqrt(var + eps)
    sc = prm[f"{key}.weight"] * inv
    return np.stack([mean, inv]), np.stack([sc, prm[f"{key}.bias"] - mean * sc]), var, running


def act(c, affine, slope=None):
    y = c * affine[0] + affine[1]
    return y if slope is None else np.where(y > 0, y, slope * y)


def _conv_act(c, affine, slope, w, stride, omit=None):
    a = act(c, affine, slope) if affine is not None else c
    if omit == "pad_zero" and affine is not None and w.shape[1] == 3:      # the wrong network: the padding ring holds act(0)
        ring = act(np.zeros_like(c[:1, :1, :1]), affine, slope)
        full = np.pad(a - ring, ((0, 0), (1, 1), (1, 1), (0, 0))) + ring
        up = torch.from_numpy(w_to_upstream(w))
        return _nhwc(F.conv2d(_nchw(full), up, stride=stride, padding=0))
    return conv_fwd(a, w, stride)


def bn_backward(c, g, stat, affine, gamma, slope=None, add=None, omit=None):
    """For y = c sc + sh, p = prelu(y) (slope given) and g the gradient of p: (g_c, d gamma, d beta, d slope, intermediates)."""
    ch = c.shape[-1]
    R = c.size // ch
    y = c * affine[0] + affine[1]
    gy = g if (slope is None or omit == "prelu_bwd") else np.where(y > 0, g, slope * g)
    xh = (c - stat[0]) * stat[1]
    ax = tuple(range(c.ndim - 1))
    s1, s2 = gy.sum(ax), (gy * xh).sum(ax)
    ds = (g * np.minimum(y, 0.0)).sum(ax) if slope is not None else None
    t1 = s1 / R if omit != "bn_mean_term" else 0.0
    t2 = xh * (s2 / R) if omit != "bn_xhat_term" else 0.0
    gc = gamma * stat[1] * (gy - t1 - t2)
    if add is not None and omit != "identity":
        gc = gc + add
    return gc, s2, s1, ds, dict(y=y, gy=gy, xh=xh, R=R)


# ---- bounds of the pieces ----------------------------------------------------------------------------------------------------------
def _stat_bound(c, ec, stat, prm, key, affine, training=True):
    """-> (d mean, d var, d invstd, d sc, d sh) of a BatchNorm over values c known to within ec."""
    ch = c.shape[-1]
    cr, er = c.reshape(-1, ch), np.broadcast_to(ec, c.shape).reshape(-1, ch)
    R = cr.shape[0]
    gam = np.abs(prm[f"{key}.weight"])
    if training:
        spread = np.abs(cr - cr[0]).max(0) + er.max(0)
        em = er.mean(0) + (R + 4) * U64 * spread
        ev = (2.0 / R) * (np.abs(cr - stat[0]) * (er + em)).sum(0) * SECOND + (2 * R + 16) * U64 * spread ** 2
    else:
        em = ev = np.zeros(ch)
    ei = 0.5 * stat[1] ** 3 * ev * SECOND + 4 * U64 * stat[1]
    esc = gam * ei + U32 * np.abs(affine[0])
    esh = gam * (em * stat[1] + np.abs(stat[0]) * ei) * SECOND + U32 * np.abs(affine[1])
    return em, ev, ei, esc, esh


def _act_bound(c, ec, affine, esc, esh, slope=None):
    y = c * affine[0] + affine[1]
    ey = (np.abs(c) * esc + esh + ec * np.abs(affine[0])) * SECOND + U32 * np.abs(y)
    if slope is None:
        return ey
    a = np.where(y > 0, y, slope * y)
    return (np.where(y > 0, 1.0, np.abs(slope)) + (np.abs(y) <= ey) * (1.0 + np.abs(slope))) * ey + U32 * np.abs(a)


def _conv_bound(a, ea, w, stride):
    K = w.shape[1] * w.shape[2] * w.shape[3]
    return ((K + 2) * U32 * conv_fwd(np.abs(a), np.abs(w), stride) + conv_fwd(ea, np.abs(w), stride)) * SECOND


def _running_bound(running, key, em, ev, R, momentum=MOMENTUM):
    return {f"{key}.running_mean": momentum * em + U32 * np.abs(running[f"{key}.running_mean"]) * SECOND,
            f"{key}.running_var": momentum * ev * (R / (R - 1.0)) * SECOND + U32 * np.abs(running[f"{key}.running_var"]) * SECOND}


def _bn_backward_bound(c, g, eg, stat, affine, gamma, slope, add, eadd, r):
    """Bounds of (g_c, d gamma, d beta, d slope) for a gradient g known to within eg; r: bn_backward's intermediates."""
    R, y, gy, xh = r["R"], r["y"], r["gy"], np.abs(r["xh"])
    ax = tuple(range(c.ndim - 1))
    egy = eg if slope is None else np.where(y > 0, eg, np.abs(slope) * eg) + 2 * U64 * np.abs(gy)
    e1 = egy.sum(ax) + (R + 8) * U64 * np.abs(gy).sum(ax)
    e2 = (egy * xh).sum(ax) * SECOND + (R + 8) * U64 * (np.abs(gy) * xh).sum(ax)
    s1, s2 = gy.sum(ax), (gy * r["xh"]).sum(ax)
    out = {"beta": (e1 + U32 * (np.abs(s1) + e1)) * SECOND, "gamma": (e2 + U32 * (np.abs(s2) + e2)) * SECOND}
    if slope is not None:
        m = np.abs(np.minimum(y, 0.0))
        e3 = (eg * m).sum(ax) * SECOND + U32 * (np.abs(g) * m).sum(ax) + (R + 8) * U64 * (np.abs(g) * m).sum(ax)
        out["slope"] = (e3 + U32 * (np.abs((g * np.minimum(y, 0.0)).sum(ax)) + e3)) * SECOND
    k = np.abs(gamma) * stat[1]
    gc = gamma * stat[1] * (gy - s1 / R - r["xh"] * (s2 / R)) + (add if add is not None else 0.0)
    e = k * (egy + e1 / R + xh * e2 / R) * SECOND + 8 * U64 * k * (np.abs(gy) + np.abs(s1) / R + xh * np.abs(s2) / R)
    if add is not None:
        e = e + eadd + 2 * U64 * np.abs(add)
    out["gc"] = e + U32 * (np.abs(gc) + e)
    return out


def _recompute_bound(c, affine, slope):
    """The load path's activation from stored c, sc, sh against its double evaluation: one rounding, one more under the slope."""
    y = c * affine[0] + affine[1]
    if slope is None:
        return U32 * np.abs(y)
    return (np.where(y > 0, 1.0, np.abs(slope)) * U32 * np.abs(y) + U32 * np.abs(np.where(y > 0, y, slope * y))) * SECOND


def _dgrad_bound(g, eg, w, stride, in_shape):
    K = w.shape[0] * w.shape[1] * w.shape[2]
    return ((K + 2) * U32 * conv_dgrad(np.abs(g), np.abs(w), stride, in_shape) + conv_dgrad(eg, np.abs(w), stride, in_shape)) * SECOND


def _wgrad_bound(g, eg, a, ea, w_shape, stride):
    M = g.size // g.shape[-1]
    return ((M + 2) * U32 * conv_wgrad(np.abs(g), np.abs(a), w_shape, stride) + conv_wgrad(eg, np.abs(a), w_shape, stride) +
            conv_wgrad(np.abs(g), ea, w_shape, stride)) * SECOND


# ---- the block ---------------------------------------------------------------------------------------------------------------------
def block_forward(x, prm, stride, training=True, omit=None, bounds=False):
    """-> a dict: out, c1, c2, cd (None without the downsample branch), stat{1,2,3,d}, affine{1,2,3,d}, running (training); with
    bounds=True also "bound": {out, c1, c2, cd, running: {...}, stat1 ...: (d mean, d invstd)}."""
    ds = "downsample.0.weight" in prm
    st1, af1, _, r1 = bn_forward(x, prm, "bn1", training)
    c1 = _conv_act(x, af1, None, prm["conv1.weight"], 1, omit)
    st2, af2, _, r2 = bn_forward(c1, prm, "bn2", training)
    c2 = _conv_act(c1, af2, prm["prelu.weight"], prm["conv2.weight"], stride, omit)
    st3, af3, _, r3 = bn_forward(c2, prm, "bn3", training)
    cd = std = afd = rd = None
    if ds:
        cd = conv_fwd(x, prm["downsample.0.weight"], stride)
        std, afd, _, rd = bn_forward(cd, prm, "downsample.1", training)
        idn = act(cd, afd)
    else:
        idn = x
    out = act(c2, af3) + (idn if omit != "identity" else 0.0)
    fw = dict(out=out, c1=c1, c2=c2, cd=cd, stat1=st1, affine1=af1, stat2=st2, affine2=af2, stat3=st3, affine3=af3, statd=std, affined=afd)
    if training:
        fw["running"] = {}
        for r in (r1, r2, r3, rd):
            if r:
                fw["running"].update(r)
    if not bounds:
        return fw
    b, rb = {}, {}
    rows = lambda a: a.size // a.shape[-1]      # noqa: E731
    em, ev, ei, esc, esh = _stat_bound(x, 0.0, st1, prm, "bn1", af1, training)
    b["stat1"] = (em, ei)
    if training:
        rb.update(_running_bound(fw["running"], "bn1", em, ev, rows(x)))
    b["c1"] = _conv_bound(act(x, af1), _act_bound(x, 0.0, af1, esc, esh), prm["conv1.weight"], 1)
    em, ev, ei, esc, esh = _stat_bound(c1, b["c1"], st2, prm, "bn2", af2, training)
    b["stat2"] = (em, ei)
    if training:
        rb.update(_running_bound(fw["running"], "bn2", em, ev, rows(c1)))
    sl = prm["prelu.weight"]
    b["c2"] = _conv_bound(act(c1, af2, sl), _act_bound(c1, b["c1"], af2, esc, esh, sl), prm["conv2.weight"], stride)
    em, ev, ei, esc, esh = _stat_bound(c2, b["c2"], st3, prm, "bn3", af3, training)
    b["stat3"] = (em, ei)
    if training:
        rb.update(_running_bound(fw["running"], "bn3", em, ev, rows(c2)))
    e3 = _act_bound(c2, b["c2"], af3, esc, esh)
    eid = 0.0
    if ds:
        b["cd"] = _conv_bound(x, 0.0 * x, prm["downsample.0.weight"], stride)
        em, ev, ei, esc, esh = _stat_bound(cd, b["cd"], std, prm, "downsample.1", afd, training)
        b["statd"] = (em, ei)
        if training:
            rb.update(_running_bound(fw["running"], "downsample.1", em, ev, rows(cd)))
        eid = _act_bound(cd, b["cd"], afd, esc, esh)
    b["out"] = (e3 + eid) * SECOND + U32 * np.abs(out)
    b["running"] = rb
    fw["bound"] = b
    return fw


BLOCK_GRADS = ("bn1.weight", "bn1.bias", "conv1.weight", "bn2.weight", "bn2.bias", "prelu.weight", "conv2.weight", "bn3.weight", "bn3.bias",
               "downsample.0.weight", "downsample.1.weight", "downsample.1.bias")


def block_backward(x, prm, stride, g, ctx, omit=None, bounds=False):
    """The gradients as a function of the cotangent g and a saved context `ctx` (keys c1, c2, cd, stat*, affine*: the oracle's own
    forward, or the values a GPU forward stored).  -> {upstream key: gradient (conv weights in the device layout), "input": d x};
    with bounds=True also "bound": the same keys."""
    ds = "downsample.0.weight" in prm
    c1, c2, sl = ctx["c1"], ctx["c2"], prm["prelu.weight"]
    w1, w2 = prm["conv1.weight"], prm["conv2.weight"]
    out, b = {}, {}
    g_c2, out["bn3.weight"], out["bn3.bias"], _, r3 = bn_backward(c2, g, ctx["stat3"], ctx["affine3"], prm["bn3.weight"], omit=omit)
    a2 = act(c1, ctx["affine2"], sl)
    out["conv2.weight"] = conv_wgrad(g_c2, a2, w2.shape, stride)
    g_a2 = conv_dgrad(g_c2, w2, stride, c1.shape)
    g_c1, out["bn2.weight"], out["bn2.bias"], out["prelu.weight"], r2 = bn_backward(c1, g_a2, ctx["stat2"], ctx["affine2"], prm["bn2.weight"],
                                                                                   sl, omit=omit)
    a1 = act(x, ctx["affine1"])
    out["conv1.weight"] = conv_wgrad(g_c1, a1, w1.shape, 1)
    g_a1 = conv_dgrad(g_c1, w1, 1, x.shape)
    add = g
    if ds:
        wd, cd = prm["downsample.0.weight"], ctx["cd"]
        g_cd, out["downsample.1.weight"], out["downsample.1.bias"], _, rd = bn_backward(cd, g, ctx["statd"], ctx["affined"],
                                                                                        prm["downsample.1.weight"], omit=omit)
        out["downsample.0.weight"] = conv_wgrad(g_cd, x, wd.shape, stride)
        add = conv_dgrad(g_cd, wd, stride, x.shape)
    out["input"], out["bn1.weight"], out["bn1.bias"], _, r1 = bn_backward(x, g_a1, ctx["stat1"], ctx["affine1"], prm["bn1.weight"], None, add,
                                                                          omit=omit)
    if not bounds:
        return out
    zero = 0.0 * g
    b3 = _bn_backward_bound(c2, g, zero, ctx["stat3"], ctx["affine3"], prm["bn3.weight"], None, None, None, r3)
    b["bn3.weight"], b["bn3.bias"] = b3["gamma"], b3["beta"]
    b["conv2.weight"] = _wgrad_bound(g_c2, b3["gc"], a2, _recompute_bound(c1, ctx["affine2"], sl), w2.shape, stride)
    e_a2 = _dgrad_bound(g_c2, b3["gc"], w2, stride, c1.shape)
    b2 = _bn_backward_bound(c1, g_a2, e_a2, ctx["stat2"], ctx["affine2"], prm["bn2.weight"], sl, None, None, r2)
    b["bn2.weight"], b["bn2.bias"], b["prelu.weight"] = b2["gamma"], b2["beta"], b2["slope"]
    b["conv1.weight"] = _wgrad_bound(g_c1, b2["gc"], a1, _recompute_bound(x, ctx["affine1"], None), w1.shape, 1)
    e_a1 = _dgrad_bound(g_c1, b2["gc"], w1, 1, x.shape)
    eadd = zero if not ds else None
    if ds:
        bd = _bn_backward_bound(cd, g, zero, ctx["statd"], ctx["affined"], prm["downsample.1.weight"], None, None, None, rd)
        b["downsample.1.weight"], b["downsample.1.bias"] = bd["gamma"], bd["beta"]
        b["downsample.0.weight"] = _wgrad_bound(g_cd, bd["gc"], x, 0.0 * x, wd.shape, stride)
        eadd = _dgrad_bound(g_cd, bd["gc"], wd, stride, x.shape)
    b1 = _bn_backward_bound(x, g_a1, e_a1, ctx["stat1"], ctx["affine1"], prm["bn1.weight"], None, add, eadd, r1)
    b["bn1.weight"], b["bn1.bias"], b["input"] = b1["gamma"], b1["beta"], b1["gc"]
    out["bound"] = b
    return out


# ---- the stem ----------------------------------------------------------------------------------------------------------------------
def stem_forward(img, prm, training=True, bounds=False):
    """img [B, 3, H, W] -> dict(out, c1, stat1, affine1, running, x (NHWC, 3 channels))."""
    x = np.ascontiguousarray(np.transpose(img, (0, 2, 3, 1)))
    c = conv_fwd(x, prm["conv1.weight"], 1)
    st, af, _, run = bn_forward(c, prm, "bn1", training)
    fw = dict(out=act(c, af, prm["prelu.weight"]), c1=c, stat1=st, affine1=af, x=x)
    if training:
        fw["running"] = run
    if bounds:
        b = {"c1": _conv_bound(x, 0.0 * x, prm["conv1.weight"], 1)}
        em, ev, ei, esc, esh = _stat_bound(c, b["c1"], st, prm, "bn1", af, training)
        b["stat1"] = (em, ei)
        b["out"] = _act_bound(c, b["c1"], af, esc, esh, prm["prelu.weight"])
        b["running"] = _running_bound(run, "bn1", em, ev, c.size // 64) if training else {}
        fw["bound"] = b
    return fw


STEM_GRADS = ("conv1.weight", "bn1.weight", "bn1.bias", "prelu.weight")


def stem_backward(img, prm, g, ctx, bounds=False):
    x = np.ascontiguousarray(np.transpose(img, (0, 2, 3, 1)))
    c, sl = ctx["c1"], prm["prelu.weight"]
    out = {}
    g_c, out["bn1.weight"], out["bn1.bias"], out["prelu.weight"], r = bn_backward(c, g, ctx["stat1"], ctx["affine1"], prm["bn1.weight"], sl)
    out["conv1.weight"] = conv_wgrad(g_c, x, prm["conv1.weight"].shape, 1)
    if bounds:
        bb = _bn_backward_bound(c, g, 0.0 * g, ctx["stat1"], ctx["affine1"], prm["bn1.weight"], sl, None, None, r)
        out["bound"] = {"bn1.weight": bb["gamma"], "bn1.bias": bb["beta"], "prelu.weight": bb["slope"],
                        "conv1.weight": _wgrad_bound(g_c, bb["gc"], x, 0.0 * x, prm["conv1.weight"].shape, 1)}
    return out
