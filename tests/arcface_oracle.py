"""Plain-torch fp32 NCHW restatement of the ArcFace IResNet (insightface arcface_torch ``iresnet.py``, as loaded by the reference's
ArcFace_functions.prepare_locked_ArcFace_model), written from the architecture alone, with UNFOLDED eval-mode BatchNorms.

``emulate`` = torch.float16 / torch.bfloat16 rounds every stored activation (and every conv weight) to that dtype, the way the
reference runs under fp16 autocast: conv / bn / prelu outputs and the residual sum are 16-bit tensors, ``fc`` runs in fp32 on the
rounded input, ``features`` in fp32.  Used to size the GPU tolerances on CPU.

Also ``run_folded``: the engine's arithmetic (faceposegenerator_amd.arcface.fold_weights) evaluated by plain torch in NHWC order with
the second-output ``bn1`` — the CPU check that the folding is exact."""
from __future__ import annotations

from typing import Dict, List, Optional

import torch
import torch.nn.functional as F

ARCHS = {"r18": [2, 2, 2, 2], "r34": [3, 4, 6, 3], "r50": [3, 4, 14, 3], "r100": [3, 13, 30, 3], "r200": [6, 26, 60, 6]}
PLANES = [64, 128, 256, 512]
EPS = 1e-5


def _r(x: torch.Tensor, emulate: Optional[torch.dtype]) -> torch.Tensor:
    return x if emulate is None else x.to(emulate).float()


def _bn(x, sd, key, emulate):
    return _r(F.batch_norm(x, sd[f"{key}.running_mean"].float(), sd[f"{key}.running_var"].float(), sd[f"{key}.weight"].float(),
                           sd[f"{key}.bias"].float(), False, 0.0, EPS), emulate)


def _conv(x, w, stride, pad, emulate):
    return _r(F.conv2d(x, _r(w.float(), emulate), None, stride, pad), emulate)


def _prelu(x, w, emulate):
    return _r(F.prelu(x, w.float()), emulate)


def stem(sd, x, emulate=None):
    x = _r(x.float(), emulate)
    return _prelu(_bn(_conv(x, sd["conv1.weight"], 1, 1, emulate), sd, "bn1", emulate), sd["prelu.weight"], emulate)


def block(sd, key, x, stride, emulate=None):
    out = _bn(x, sd, f"{key}.bn1", emulate)
    out = _conv(out, sd[f"{key}.conv1.weight"], 1, 1, emulate)
    out = _prelu(_bn(out, sd, f"{key}.bn2", emulate), sd[f"{key}.prelu.weight"], emulate)
    out = _bn(_conv(out, sd[f"{key}.conv2.weight"], stride, 1, emulate), sd, f"{key}.bn3", emulate)
    idt = x
    if f"{key}.downsample.0.weight" in sd:
        idt = _bn(_conv(x, sd[f"{key}.downsample.0.weight"], stride, 0, emulate), sd, f"{key}.downsample.1", emulate)
    return _r(out + idt, emulate)


def stage(sd, arch, i, x, emulate=None):
    """layer{i+1} of ``arch`` on its input x (NCHW)."""
    for j in range(ARCHS[arch][i]):
        x = block(sd, f"layer{i + 1}.{j}", x, 2 if j == 0 else 1, emulate)
    return x


def head(sd, x, emulate=None):
    x = _bn(x, sd, "bn2", emulate).flatten(1)                       # NCHW order: c*49 + h*7 + w; dropout = identity in eval
    x = F.linear(x.float(), sd["fc.weight"].float(), sd["fc.bias"].float())
    return F.batch_norm(x, sd["features.running_mean"].float(), sd["features.running_var"].float(), sd["features.weight"].float(),
                        sd["features.bias"].float(), False, 0.0, EPS)


def forward(sd, arch, x, emulate=None, stages_out: Optional[List[torch.Tensor]] = None):
    """x: float [B,3,112,112], already (x/255 - 0.5)/0.5 -> [B,512] fp32.  stages_out, if given, receives the stem output and the
    output of each layer (NCHW)."""
    x = stem(sd, x, emulate)
    if stages_out is not None:
        stages_out.append(x)
    for i in range(4):
        x = stage(sd, arch, i, x, emulate)
        if stages_out is not None:
            stages_out.append(x)
    return head(sd, x, emulate)


# ---- the folded engine arithmetic, evaluated by plain torch (fp32, NHWC, no rounding) -------------------------------------------
def _im2col_nhwc(x: torch.Tensor, stride: int) -> torch.Tensor:
    """[B,H,W,C] -> [B,OH,OW,9*C] in [tap][channel] order, zero padding 1 (the K order of idb_gemm's 3x3 sources)."""
    B, H, W, C = x.shape
    xp = F.pad(x, (0, 0, 1, 1, 1, 1))
    oh, ow = (H + stride - 1) // stride, (W + stride - 1) // stride
    taps = [xp[:, dy:dy + stride * (oh - 1) + 1:stride, dx:dx + stride * (ow - 1) + 1:stride, :] for dy in range(3) for dx in range(3)]
    return torch.cat(taps, dim=3)


def _gemm(a: torch.Tensor, w: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    return a @ w.t() + b


def run_folded(fw: Dict[str, torch.Tensor], arch: str, x: torch.Tensor, stages_out: Optional[List[torch.Tensor]] = None) -> torch.Tensor:
    """fold_weights(...) output applied to x [B,3,112,112] the way the engine does, in fp32: stem (bn1 folded) + PReLU, second output
    = the next bn1; per block conv1 (+bn2, PReLU) on that second output, conv2 (+bn3) with the downsample as a second K segment or the
    identity as a residual, second output = the next block's bn1; head = one fp32 matrix over the NHWC-flattened map.
    stages_out receives the NHWC stem / layer outputs."""
    x = x.float().permute(0, 2, 3, 1).contiguous()
    y = _gemm(_im2col_nhwc(x, 1), fw["stem.w"], fw["stem.b"])
    x = F.prelu(y.permute(0, 3, 1, 2), fw["stem.slope"]).permute(0, 2, 3, 1)
    xb = x * fw["stem.out2_scale"] + fw["stem.out2_shift"]
    if stages_out is not None:
        stages_out.append(x)
    for i, nb in enumerate(ARCHS[arch]):
        for j in range(nb):
            k = f"layer{i + 1}.{j}"
            s = 2 if j == 0 else 1
            h = _gemm(_im2col_nhwc(xb, 1), fw[f"{k}.conv1.w"], fw[f"{k}.conv1.b"])
            h = F.prelu(h.permute(0, 3, 1, 2), fw[f"{k}.conv1.slope"]).permute(0, 2, 3, 1)
            a = _im2col_nhwc(h, s)
            if j == 0:
                a = torch.cat([a, x[:, ::2, ::2, :]], dim=3)                  # 1x1 stride-2 source: pixel (2oy, 2ox)
                x = _gemm(a, fw[f"{k}.conv2.w"], fw[f"{k}.conv2.b"])
            else:
                x = _gemm(a, fw[f"{k}.conv2.w"], fw[f"{k}.conv2.b"]) + x
            if f"{k}.out2_scale" in fw:
                xb = x * fw[f"{k}.out2_scale"] + fw[f"{k}.out2_shift"]
        if stages_out is not None:
            stages_out.append(x)
    return x.reshape(x.shape[0], -1) @ fw["fc.w"].t() + fw["fc.b"]
