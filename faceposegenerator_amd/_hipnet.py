"""What the evaluation networks (arcface.py, headpose.py) share: the load-time folding helpers and the device shell around
libidb_kernels.so — weight upload, stream, split-K workspace, one checked idb_gemm call and the chunked batch loop."""
from __future__ import annotations

from typing import Callable, Dict, Optional, Tuple

import torch

from . import _lib as L

SD = Dict[str, torch.Tensor]


def bn_affine(sd: SD, key: str, eps: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """eval-mode BatchNorm ``key`` as y = a x + b (float64)."""
    a = sd[f"{key}.weight"].double() / torch.sqrt(sd[f"{key}.running_var"].double() + eps)
    return a, sd[f"{key}.bias"].double() - sd[f"{key}.running_mean"].double() * a


def pack_conv(w: torch.Tensor) -> torch.Tensor:
    """[cout][cin][kh][kw] -> [cout][kh*kw*cin] ([tap][channel] K order of idb_gemm; for a grouped conv, row block g is group g's
    matrix)."""
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1)


def check_state_dict(sd: SD, shapes: Dict[str, Tuple[int, ...]], what: str) -> None:
    """Strict keys and shapes against ``shapes``: missing / unexpected / wrong-shaped keys raise ValueError naming them (``what``
    opens the message); num_batches_tracked is accepted and ignored."""
    need = {k for k in shapes if not k.endswith("num_batches_tracked")}
    have = {k for k in sd if not k.endswith("num_batches_tracked")}
    missing, extra = sorted(need - have), sorted(have - set(shapes))
    if missing or extra:
        raise ValueError(f"{what} state dict: missing keys {missing[:8]}{'...' if len(missing) > 8 else ''}, "
                         f"unexpected keys {extra[:8]}{'...' if len(extra) > 8 else ''}")
    for k in sorted(need):
        if tuple(sd[k].shape) != shapes[k]:
            raise ValueError(f"{what} state dict: {k} has shape {tuple(sd[k].shape)}, expected {shapes[k]}")


class HipNet:
    """Device shell of an evaluation network.  A subclass sets ``NAME`` and ``DTYPES`` (the wording of its errors), folds its weights
    on the CPU into ``self._fw`` and says through ``_operand`` which of them the MFMA kernels read (operand dtype; the rest stay fp32)."""

    NAME = "HipNet"
    DTYPES = "float16 or bfloat16"

    def __init__(self, torch_dtype: torch.dtype, chunk: int):
        if torch_dtype not in (torch.float16, torch.bfloat16):
            raise ValueError(f"{self.NAME} runs in {self.DTYPES}")
        self.tdt = torch_dtype
        self.dt = L.IDB_F16 if torch_dtype == torch.float16 else L.IDB_BF16
        self._fw: Dict[str, torch.Tensor] = {}          # the subclass's fold_weights(...) result (CPU, fp32)
        self.chunk = int(chunk)
        self.device: Optional[torch.device] = None
        self.lib = None
        self._ws = None

    def _operand(self, key: str) -> bool:
        raise NotImplementedError

    def to(self, device):
        device = torch.device(device)
        if device.type != "cuda":
            raise ValueError(f"{self.NAME} runs on the GPU only (HIP kernels); use .to('cuda:N')")
        self.lib = L.load()
        idx = device.index if device.index is not None else torch.cuda.current_device()
        L.check(self.lib.idb_device_check(idx), "idb_device_check")
        self.device = torch.device("cuda", idx)
        self.w: Dict[str, torch.Tensor] = {
            k: v.to(self.device, dtype=self.tdt if self._operand(k) else torch.float32).contiguous() for k, v in self._fw.items()}
        return self

    def _need_device(self):
        if self.device is None:
            raise RuntimeError("call .to('cuda:N') first")

    def _stream(self) -> int:
        return torch.cuda.current_stream(self.device).cuda_stream

    def _workspace(self, nbytes: int) -> Optional[torch.Tensor]:
        if nbytes == 0:
            return None
        if self._ws is None or self._ws.numel() < nbytes:
            self._ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        return self._ws

    def _gemm(self, srcs, w_ptr, n, batch, oh, ow, **fields) -> None:
        """One checked idb_gemm in the operand dtype (arguments of _lib.gemm_desc)."""
        d = L.gemm_desc(self.dt, srcs, w_ptr, n, batch, oh, ow, **fields)
        L.check(L.run_gemm(self.lib, d, self._workspace, self._stream()), "idb_gemm")

    def _chunked(self, x: torch.Tensor, fn: Callable[[torch.Tensor], Tuple[torch.Tensor, ...]]) -> Tuple[torch.Tensor, ...]:
        """fn on contiguous batch slices of at most ``chunk`` samples; each of its outputs concatenated along the batch."""
        self._need_device()
        outs = [fn(x[s:s + self.chunk].contiguous()) for s in range(0, x.shape[0], self.chunk)]
        return outs[0] if len(outs) == 1 else tuple(torch.cat(o) for o in zip(*outs))
