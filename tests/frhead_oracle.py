"""Float64 restatement of the face-recognition loss head (FR_training/utils/losses.py CosFace / ArcFace / AdaFace, CrossEntropyLoss,
multi_class_acc, AverageMeter, ArcBiFaceGANDataset's label rule): direct numpy formulas, no tiling, every step written as upstream
writes it.  tests/test_frhead_cpu.py checks it against recordings of the reference's own classes (tests/golden/frhead_reference.npz)."""
import math

import numpy as np

EPS = 1e-3
DEFAULT_M = {"CosFace": 0.35, "ArcFace": 0.50, "AdaFace": 0.4}
# recorded cases: (name, loss, B, C, D, seed)
CASES = [("cos_64", "CosFace", 37, 301, 64, 1), ("arc_64", "ArcFace", 37, 301, 64, 2), ("ada_64", "AdaFace", 37, 301, 64, 3),
         ("cos_512", "CosFace", 19, 151, 512, 4), ("arc_512", "ArcFace", 19, 151, 512, 5), ("ada_512", "AdaFace", 19, 151, 512, 6),
         ("ada_512_ema", "AdaFace", 19, 151, 512, 7)]


def inputs(loss, B, C, D, seed, pull=1.0):
    """(embeddings fp32 [B, D], kernel fp32 [D, C], labels int64 [B], norms fp32 [B, 1]): class directions drawn as upstream
    initialises them (normal, std 0.01), embeddings a mixture of their class direction and noise, so that the target is usually but not
    always the largest cosine and no cosine comes near +-1."""
    rng = np.random.default_rng(seed)
    kernel = (rng.standard_normal((D, C)) * 0.01).astype(np.float32)
    labels = rng.integers(0, C, B).astype(np.int64)
    wn = kernel.astype(np.float64) / np.linalg.norm(kernel.astype(np.float64), axis=0, keepdims=True)
    noise = rng.standard_normal((B, D))
    noise /= np.linalg.norm(noise, axis=1, keepdims=True)
    mix = pull * rng.uniform(0.0, 2.0, (B, 1))
    emb = mix * wn[:, labels].T + noise
    norms = rng.uniform(5.0, 40.0, (B, 1))
    if loss == "AdaFace":                                     # AdaFace takes unit rows and their norms
        emb = emb / np.linalg.norm(emb, axis=1, keepdims=True)
    else:
        emb = emb * norms
    return emb.astype(np.float32), kernel, labels, norms.astype(np.float32)


def l2_norm(x, axis):
    return x / np.linalg.norm(x, 2, axis, keepdims=True)


def ada_stats(norms, t_alpha, batch_mean, batch_std):
    """(safe_norms, new batch_mean, new batch_std): clip, mean, UNBIASED std, the EMA update."""
    safe = np.clip(np.asarray(norms, dtype=np.float64).reshape(-1, 1), 0.001, 100)
    mean, std = safe.mean(), safe.std(ddof=1)
    return safe, mean * t_alpha + (1 - t_alpha) * batch_mean, std * t_alpha + (1 - t_alpha) * batch_std


def thetas(loss, emb, kernel, labels, s=64.0, m=None, norms=None, h=0.333, t_alpha=1.0, batch_mean=20.0, batch_std=100.0):
    """-> (thetas float64 [B, C], extras): upstream's forward on float64 copies of the fp32 inputs."""
    m = DEFAULT_M[loss] if m is None else m
    emb, kernel, labels = np.asarray(emb, dtype=np.float64), np.asarray(kernel, dtype=np.float64), np.asarray(labels).reshape(-1)
    rows = np.arange(emb.shape[0])
    kernel_norm = l2_norm(kernel, 0)
    extras = {}
    if loss in ("CosFace", "ArcFace"):
        cos = np.clip(l2_norm(emb, 1) @ kernel_norm, -1, 1)
        if loss == "CosFace":
            cos[rows, labels] -= m
            return cos * s, extras
        theta = np.arccos(cos)
        theta[rows, labels] += m
        return np.cos(theta) * s, extras
    if loss != "AdaFace":
        raise ValueError(loss)
    cosine = np.clip(emb @ kernel_norm, -1 + EPS, 1 - EPS)
    safe, batch_mean, batch_std = ada_stats(norms, t_alpha, batch_mean, batch_std)
    scaler = np.clip((safe - batch_mean) / (batch_std + EPS) * h, -1, 1)
    m_arc = np.zeros_like(cosine)
    m_arc[rows, labels] = 1.0
    theta_m = np.clip(np.arccos(cosine) + m_arc * (m * scaler * -1), EPS, math.pi - EPS)
    m_cos = np.zeros_like(cosine)
    m_cos[rows, labels] = 1.0
    out = (np.cos(theta_m) - m_cos * (m + m * scaler)) * s
    extras.update(batch_mean=float(batch_mean), batch_std=float(batch_std), margin_scaler=scaler.reshape(-1))
    return out, extras


def cross_entropy(th, labels):
    """(mean loss, per-sample loss, lse): a plain log-sum-exp about the row maximum."""
    th, labels = np.asarray(th, dtype=np.float64), np.asarray(labels).reshape(-1)
    mx = th.max(axis=1)
    lse = mx + np.log(np.exp(th - mx[:, None]).sum(axis=1))
    per = lse - th[np.arange(th.shape[0]), labels]
    return float(per.sum() / per.shape[0]), per, lse


def argmax(th):
    return np.argmax(np.asarray(th), axis=1)                   # the first maximum, as torch.argmax


def top2_gap(th):
    """Per row: the largest logit minus the second largest (0 for tied maxima); inf when C = 1."""
    th = np.asarray(th, dtype=np.float64)
    if th.shape[1] < 2:
        return np.full(th.shape[0], np.inf)
    part = np.partition(th, -2, axis=1)
    return part[:, -1] - part[:, -2]


def multi_class_acc(pred, labels):
    pred, labels = np.asarray(pred).reshape(-1), np.asarray(labels).reshape(-1)
    acc = int((pred == labels).sum()) / labels.shape[0]
    return round(acc * 100, 2)


def average_meter(values):
    total, count = 0, 0
    for v in values:
        total += v * 1
        count += 1
    return total / count


def dataset_labels(file_names):
    labels = np.array([int(f.split("_")[0]) for f in file_names])
    return labels, int(labels.max()) + 1


# ---- bounds and cases shared by the CPU and the GPU test (derivations: tests/test_frhead_gpu.py) -------------------------------------
U32, U64 = 2.0 ** -24, 2.0 ** -53
S = 64.0
GPU_B, GPU_C, GPU_D = (1, 2, 37, 128, 130), (1, 2, 33, 301, 4099), (512, 130, 7)
GPU_LOSSES = ("CosFace", "ArcFace", "AdaFace")


def gpu_cases():
    """Every (loss, B, C, D) of the GPU test; AdaFace refuses B = 1 (the unbiased std of one norm)."""
    return [(loss, B, C, D) for loss in GPU_LOSSES for B in GPU_B for C in GPU_C for D in GPU_D if not (loss == "AdaFace" and B < 2)]


def gpu_seed(loss, B, C, D):
    return 1000 * GPU_LOSSES.index(loss) + 97 * B + 7 * C + D


def logit_bound(D, s=S):
    return s * (D + 4) * U32 * 1.001


def lse_bound(D, C, s=S):
    return logit_bound(D, s) + 2.0 ** -18 + 2.0 ** -17 * 1.001 + 4 * U32 + (C + 300) * U64 * 4 * s


def cos_eps(D):
    return (4 * D + 16) * U64


def target_bound(loss, D, cos_target, s=S, m=None, scaler_err=0.0):
    """Per row, from the oracle's own target cosine."""
    m = DEFAULT_M[loss] if m is None else m
    eps, c = cos_eps(D), np.abs(np.asarray(cos_target, dtype=np.float64))
    if loss == "CosFace":
        return np.full(c.shape, s * (eps + 8 * U64))
    if loss == "AdaFace":
        return np.full(c.shape, s * (eps / math.sqrt(1 - (1 - EPS) ** 2) + 16 * U64 + 2 * m * scaler_err))
    far = np.minimum(c + eps, 1.0)
    with np.errstate(divide="ignore"):
        lipschitz = np.where(far < 1.0, eps / np.sqrt(np.maximum(1 - far * far, 1e-300)), np.inf)
    return s * (np.minimum(lipschitz, math.pi / 2 * math.sqrt(2 * eps)) + 16 * U64)


def target_cosine(loss, emb, kernel, labels):
    emb, kernel = np.asarray(emb, dtype=np.float64), np.asarray(kernel, dtype=np.float64)
    x = emb if loss == "AdaFace" else l2_norm(emb, 1)
    return np.einsum("bd,db->b", x, l2_norm(kernel, 0)[:, np.asarray(labels).reshape(-1)])


def ambiguous_rows(th, bound):
    """Rows whose float64 top-two gap does not exceed twice the logit bound: either contender is an acceptable argmax."""
    return top2_gap(th) <= 2 * bound
