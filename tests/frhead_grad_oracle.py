"""Float64 restatement of the FR loss head's backward (what autograd leaves in `embeddings.grad` and `kernel.grad` after
`CrossEntropyLoss()(header(embeddings, label), label).backward()` with the reference's CosFace / ArcFace / AdaFace) and of the header's
optimiser step (`clip_grad_norm_`, then `torch.optim.SGD` with momentum and weight decay), in direct numpy.  Inputs and the forward come
from tests/frhead_oracle.py.  tests/test_frhead_grad_cpu.py checks it against recordings of the reference's own classes under autograd
(tests/golden/frhead_grad_reference*.npz).  It also carries the cases, seeds and bound functions the CPU and GPU tests share; the
derivation of the bounds is in tests/test_frhead_grad_gpu.py.

With r the raw cosine, (lo, hi) the clamp, z the forward's logits, p = softmax(z), g = (p - onehot) / B:
    G = g s d [lo <= r <= hi],  d = 1 off the target (the limit of sin(acos c) / sqrt(1 - c^2), which upstream evaluates to NaN at +-1),
    target d: CosFace 1, ArcFace sin(acos(c) + m) / sqrt(1 - c^2), AdaFace sin(t) / sqrt(1 - c^2) if eps <= t <= pi - eps else 0,
    dX = G Wn, dW = G^T X, d_emb_i = (dX_i - x_i <x_i, dX_i>) / |e_i| (AdaFace: dX_i), d_kernel[:, j] = (dW_j - w_j <w_j, dW_j>) / |k_j|.
`drop` leaves one term out (onehot, inv_b, slope, mask, row_projection, col_projection), for the sensitivity precondition of the GPU
cases."""
import math

import numpy as np

import frhead_oracle as O

U32, U64 = O.U32, O.U64


def backward(loss, emb, kernel, labels, s=O.S, m=None, norms=None, h=0.333, t_alpha=1.0, batch_mean=20.0, batch_std=100.0, drop=None):
    """-> dict: d_emb [B, D], d_kernel [D, C], slope [B] (the target's, mask folded in), and the intermediates the bounds need."""
    m = O.DEFAULT_M[loss] if m is None else m
    e, k, labels = np.asarray(emb, dtype=np.float64), np.asarray(kernel, dtype=np.float64), np.asarray(labels).reshape(-1)
    B, rows = e.shape[0], np.arange(e.shape[0])
    ada = loss == "AdaFace"
    n_e = np.ones((B, 1)) if ada else np.linalg.norm(e, axis=1, keepdims=True)
    cn = np.linalg.norm(k, axis=0, keepdims=True)
    x, w = e / n_e, k / cn
    r = x @ w
    lo, hi = (-1 + O.EPS, 1 - O.EPS) if ada else (-1.0, 1.0)
    mask = ((r >= lo) & (r <= hi)).astype(np.float64)
    kw = dict(norms=norms, h=h, t_alpha=t_alpha, batch_mean=batch_mean, batch_std=batch_std) if ada else {}
    z, extras = O.thetas(loss, emb, kernel, labels, s=s, m=m, **kw)
    mean_loss, per, lse = O.cross_entropy(z, labels)
    p = np.exp(z - lse[:, None])
    onehot = np.zeros_like(p)
    onehot[rows, labels] = 1.0
    g = p - (0.0 if drop == "onehot" else onehot)
    if drop != "inv_b":
        g = g / B
    c_t = np.clip(r[rows, labels], lo, hi)
    if loss == "CosFace":
        slope = np.ones(B)
    elif loss == "ArcFace":
        slope = np.sin(np.arccos(c_t) + m) / np.sqrt(1 - c_t * c_t)
    else:
        theta = np.arccos(c_t) - m * extras["margin_scaler"]
        slope = np.where((theta >= O.EPS) & (theta <= math.pi - O.EPS), np.sin(theta) / np.sqrt(1 - c_t * c_t), 0.0)
    d = np.ones_like(p)
    if drop != "slope":
        d[rows, labels] = slope
    G = g * s * d * (1.0 if drop == "mask" else mask)
    dX, dW = G @ w.T, G.T @ x                                  # [B, D], [C, D]
    row_dot, col_dot = (G * r).sum(axis=1, keepdims=True), (G * r).sum(axis=0)[:, None]
    if ada:
        d_emb = dX
    else:
        d_emb = (dX - (0.0 if drop == "row_projection" else x * row_dot)) / n_e
    d_kernel = ((dW - (0.0 if drop == "col_projection" else w.T * col_dot)) / cn.T).T
    return dict(d_emb=d_emb, d_kernel=d_kernel, slope=slope * mask[rows, labels], loss=mean_loss, per=per, lse=lse, z=z, p=p, G=G, r=r, x=x, w=w,
                n_e=n_e, cn=cn, extras=extras, c_t=r[rows, labels], labels=labels)


# ---- the optimiser -------------------------------------------------------------------------------------------------------------------
def sgd_step(w, g, buf, lr, momentum=0.9, weight_decay=5e-4, max_norm=5.0):
    """One clip_grad_norm_ + torch.optim.SGD step in float64: -> (w, buf, total_norm).  buf is None on the first step."""
    w, g = np.asarray(w, dtype=np.float64), np.asarray(g, dtype=np.float64)
    total = math.sqrt(float((g * g).sum()))
    coef = min(1.0, max_norm / (total + 1e-6))
    d = coef * g + weight_decay * w
    buf = d if buf is None else momentum * np.asarray(buf, dtype=np.float64) + d
    return w - lr * buf, buf, total


# ---- cases ---------------------------------------------------------------------------------------------------------------------------
GRAD_B, GRAD_C, GRAD_D = (2, 37, 130), (1, 2, 33, 301, 4099), (7, 130, 512)
# recorded under autograd with the reference's classes: the three losses at (37, 301, 64), one (19, 151, 512) case (frhead_oracle.CASES)
RECORDED = ("cos_64", "arc_64", "ada_64", "arc_512")


def gpu_cases():
    return [(loss, B, C, D) for loss in O.GPU_LOSSES for B in GRAD_B for C in GRAD_C for D in GRAD_D]


def gpu_seed(loss, B, C, D):
    return 5000 + O.gpu_seed(loss, B, C, D)


def case_inputs(loss, B, C, D):
    """frhead_oracle.inputs with a weak pull towards the class direction (target cosines up to 0.57): after the margin the target
    competes with the other classes instead of owning the softmax, so that even the two rows of B = 2 carry a gradient whose terms can
    be told apart (test_frhead_grad_cpu.py asserts it), and no cosine comes near a clamp edge."""
    return O.inputs(loss, B, C, D, gpu_seed(loss, B, C, D), pull=0.35)


# column blocks of several class tiles: past 256 workgroups per D chunk a block takes two tiles (loss, B, C, D, classes per block)
MULTI_TILE = [("ArcFace", 2, 32801, 7, 256), ("CosFace", 130, 16400, 130, 256)]
LAST_COLUMN_C, LAST_COLUMN_BD = (33, 301, 4099), (37, 130)


def last_column_inputs(loss, C):
    """case_inputs at (B, D) = LAST_COLUMN_BD with every label on the last column of the last partial class tile."""
    B, D = LAST_COLUMN_BD
    emb, kernel, labels, norms = case_inputs(loss, B, C, D)
    return emb, kernel, np.full(B, C - 1, dtype=np.int64), norms


def all_gradient_inputs():
    """Every input the GPU test checks per element with the regular bounds: the shape matrix, the multi-tile blocks and the
    last-column labels.  Yields (loss, B, C, D, (emb, kernel, labels, norms))."""
    for loss, B, C, D in gpu_cases():
        yield loss, B, C, D, case_inputs(loss, B, C, D)
    for loss, B, C, D, _span in MULTI_TILE:
        yield loss, B, C, D, case_inputs(loss, B, C, D)
    for loss in O.GPU_LOSSES:
        for C in LAST_COLUMN_C:
            yield (loss, *LAST_COLUMN_BD[:1], C, LAST_COLUMN_BD[1], last_column_inputs(loss, C))


def clamp_case(kind):
    """AdaFace, (B, C, D) = (6, 33, 130).  'non_target': column 2 lies along embedding 0 and column 3 against embedding 1 (cosine +-1
    against the 0.999 clamp: no gradient flows through those entries).  'target_clipped': the target column of rows 0 and 1 lies along
    their embedding and their norm is large (positive margin scaler), so theta - m scaler < eps: the target's slope is 0."""
    B, C, D = 6, 33, 130
    emb, kernel, labels, norms = O.inputs("AdaFace", B, C, D, 4242)
    emb, kernel, norms = emb.copy(), kernel.copy(), norms.copy()
    labels = np.array([20, 21, 22, 23, 24, 25], dtype=np.int64)
    if kind == "non_target":
        kernel[:, 2], kernel[:, 3] = emb[0] * 2, -emb[1] * 3
    elif kind == "target_clipped":
        u = emb[0].astype(np.float64)
        v = emb[2] - u * (emb[2] @ u) / (u @ u)                # row 0: cosine 0.995, inside the clamp, so the clip of theta alone decides
        kernel[:, 20] = (2 * (0.995 * u / np.linalg.norm(u) + math.sqrt(1 - 0.995 ** 2) * v / np.linalg.norm(v))).astype(np.float32)
        kernel[:, 21] = emb[1] * 0.5                           # row 1: cosine 1, the clamp removes it as well
        for col, row, other in ((5, 0, 3), (6, 1, 4)):
            u = emb[row].astype(np.float64)
            v = emb[other] - u * (emb[other] @ u) / (u @ u)
            kernel[:, col] = (0.45 * u / np.linalg.norm(u) + math.sqrt(1 - 0.45 ** 2) * v / np.linalg.norm(v)).astype(np.float32)
        norms[:] = np.array([90.0, 95.0, 6.0, 7.0, 8.0, 9.0], dtype=np.float32).reshape(-1, 1)
    else:
        raise ValueError(kind)
    return emb, kernel, labels, norms


def class_span(B, C):
    """Classes per block of the dX launch: about 256 workgroups of 128-class tiles (idb_head_grad_workspace_bytes reports the blocks)."""
    tiles, cap = -(-C // 128), max(1, 256 // -(-B // 128))
    return 128 * -(-tiles // cap)


def terms_for(loss, C):
    """The terms of the gradient whose absence a case of this loss can show.  The target's slope is 1 for CosFace, AdaFace has no row
    projection, and with a single class G is 0 whatever the factors: only a missing one-hot shows.  The clamp mask is all ones on
    cases that keep |r| <= 0.999; the clamp cases (clamp_case) carry it."""
    if C == 1:
        return ("onehot",)
    out = ["onehot", "inv_b", "col_projection"]
    if loss != "CosFace":
        out.append("slope")
    if loss != "AdaFace":
        out.append("row_projection")
    return tuple(out)


# ---- bounds (derivation: tests/test_frhead_grad_gpu.py) ------------------------------------------------------------------------------
def slope_bound(loss, D, ref, m=None, scaler_err=0.0):
    """Per row: |slope - oracle slope| for a target cosine within cos_eps(D) of the oracle's, |c| <= 0.999 (callers assert it)."""
    m = O.DEFAULT_M[loss] if m is None else m
    if loss == "CosFace":
        return np.zeros(ref["c_t"].shape)
    eps = O.cos_eps(D)
    far = np.minimum(np.abs(ref["c_t"]) + eps, 0.9995)
    sin3 = (1 - far * far) ** 1.5
    if loss == "ArcFace":
        return eps * abs(math.sin(m)) / sin3 + 64 * U64 / np.sqrt(1 - far * far)
    mm = m * np.abs(ref["extras"]["margin_scaler"]) + m * scaler_err
    return eps * np.abs(np.sin(mm)) / sin3 + m * scaler_err / np.sqrt(1 - far * far) + 64 * U64 / np.sqrt(1 - far * far)


def g_bound(loss, B, C, D, ref, labels, s=O.S, scaler_err=0.0):
    """[B, C]: |G_ij - oracle G_ij| per entry."""
    rows = np.arange(B)
    p, G = ref["p"], ref["G"]
    tb = O.target_bound(loss, D, ref["c_t"], s=s, scaler_err=scaler_err)
    delta = np.maximum(O.logit_bound(D, s), tb + 2.0 ** -18)[:, None]      # per row: every logit the softmax sees is within delta
    e_sum = 2.0 ** -17 * 1.001 + 4 * U32 + (C + 300) * U64 * 4 * s         # relative error of the forward's sum of exponentials
    rho = np.exp(2 * delta + e_sum + 2.0 ** -17) - 1 + 6 * U32
    gb = (s / B) * p * rho * 1.001
    p_t, slope = p[rows, labels], np.abs(ref["slope"])
    one_minus = (1 - p_t) * (np.exp(2 * delta[:, 0]) - 1) + p_t * (math.exp(e_sum) - 1)
    gb[rows, labels] = (s / B) * (one_minus * slope + (1 - p_t) * slope_bound(loss, D, ref, scaler_err=scaler_err) + U32 * (1 - p_t) * slope) * 1.001
    return gb * (G != 0)                                       # entries the clamp removes on both sides are exactly 0


def grad_bounds(loss, B, C, D, ref, labels, class_span, s=O.S, scaler_err=0.0):
    """-> (bound of d_emb [B, D], bound of d_kernel [D, C]).  class_span: the classes one dX block sums in one fma chain."""
    gb, aG = g_bound(loss, B, C, D, ref, labels, s, scaler_err), np.abs(ref["G"])
    aw, ax = np.abs(ref["w"]), np.abs(ref["x"])
    xb = (gb @ aw.T + (min(C, class_span) + 2) * U32 * (aG @ aw.T)) * 1.001
    wb = (gb.T @ ax + (B + 2) * U32 * (aG.T @ ax)) * 1.001
    cos_err = (D + 4) * U32 * 1.001
    if loss == "AdaFace":
        eb = xb + U32 * np.abs(ref["d_emb"])
    else:
        rd = gb.sum(axis=1, keepdims=True) + cos_err * aG.sum(axis=1, keepdims=True)
        eb = (xb + ax * rd) / ref["n_e"] * 1.001 + U32 * np.abs(ref["d_emb"])
    cd = gb.sum(axis=0)[:, None] + cos_err * aG.sum(axis=0)[:, None]
    kb = ((wb + aw.T * cd) / ref["cn"].T * 1.001).T + U32 * np.abs(ref["d_kernel"])
    tiny = 1e-30                                               # a bound of exactly 0 only where the oracle is exactly 0
    return eb + tiny * (eb > 0), kb + tiny * (kb > 0)


def scaler_err(B, norms, extras, h=0.333):
    safe = np.clip(np.asarray(norms, dtype=np.float64), 0.001, 100)
    mean, std = extras["batch_mean"], extras["batch_std"]
    return 2 * h * (2 * B + 16) * U64 * (np.abs(safe - mean).max() + mean) / (std + O.EPS)
