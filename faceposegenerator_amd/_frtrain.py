"""What the three optimisers of the face-recognition training loop share (``frhead.HeaderSGD``, ``frtail.StageSGD``,
``frtrunk.BackboneSGD``): the loop's ``clip_grad_norm_`` + ``torch.optim.SGD(momentum, weight_decay).step()`` as one library call
(``csrc/idb_sgd.hip``), its hyper-parameters, its state dict and the life of its momentum buffers; and the one check that a module
goes to a HIP device."""
from __future__ import annotations

import math
from typing import Dict

import torch

_HYPER = ("lr", "momentum", "weight_decay", "max_norm")


def hip_device(device, who: str) -> torch.device:
    """torch.device(device) with its index resolved ("cuda" names the current device; tensors carry its index); anything but a HIP
    device is refused in `who`'s name."""
    dev = torch.device(device)
    if dev.type != "cuda":
        raise ValueError(f"{who} runs on a HIP device only (there is no CPU fallback)")
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device() if torch.cuda.is_available() else 0)
    return dev


def _each(buf, fn):
    """fn over a momentum buffer (one tensor) or over a dict of them."""
    return {k: fn(v) for k, v in buf.items()} if isinstance(buf, dict) else fn(buf)


class ClippedSGD:
    """Hyper-parameters (`lr` may be reassigned between steps: the loop's scheduler), `steps`, and the momentum buffers `_buf`, which
    exist exactly after the first step.  A subclass names its state-dict key (`_KEY`, `_EXIST`) and supplies `_new_buffers`,
    `_buffers_out`, `_buffers_in` and `step`."""
    _KEY = "momentum_buffers"
    _EXIST = "momentum buffers exist"

    def __init__(self, lr: float, momentum: float, weight_decay: float, max_norm: float):
        self.lr, self.momentum, self.weight_decay, self.max_norm = float(lr), float(momentum), float(weight_decay), float(max_norm)
        if not (0.0 <= self.lr <= 1e4 and 0.0 <= self.momentum < 1.0 and 0.0 <= self.weight_decay <= 1e4 and 0.0 < self.max_norm <= 1e30):
            raise ValueError(f"{type(self).__name__}: lr in [0, 1e4], momentum in [0, 1), weight_decay in [0, 1e4], max_norm in (0, 1e30]")
        self.steps = 0
        self._buf = None

    def _new_buffers(self):
        """Uninitialised buffers on the device, in the device layout of the weights."""
        raise NotImplementedError

    def _buffers_out(self, buf):
        """`buf` (detached host copies) in the state dict's layout."""
        raise NotImplementedError

    def _buffers_in(self, bufs):
        """The state dict's buffers, checked, as `_buf` keeps them."""
        raise NotImplementedError

    def state_dict(self) -> Dict[str, object]:
        bufs = None if self._buf is None else self._buffers_out(_each(self._buf, lambda v: v.detach().cpu()))
        return {"lr": self.lr, "momentum": self.momentum, "weight_decay": self.weight_decay, "max_norm": self.max_norm, "steps": self.steps,
                self._KEY: bufs}

    def load_state_dict(self, sd) -> None:
        name = type(self).__name__
        missing = [k for k in _HYPER + ("steps", self._KEY) if k not in sd]
        if missing:
            raise ValueError(f"{name} state dict without {missing}")
        bufs, steps = sd[self._KEY], int(sd["steps"])
        if (bufs is None) != (steps == 0):
            raise ValueError(f"{name} state dict: {self._EXIST} exactly after the first step")
        new = None if bufs is None else self._buffers_in(bufs)
        self.lr, self.momentum, self.weight_decay, self.max_norm = (float(sd[k]) for k in _HYPER)
        self.steps, self._buf = steps, new

    def _begin(self, dev) -> bool:
        """The buffers on `dev`, created at the first step.  Returns whether this is the first step."""
        first = self._buf is None
        if first:
            self._buf = self._new_buffers()
        else:
            self._buf = _each(self._buf, lambda v: v if v.device == dev else v.to(dev))
        return first

    def _finish(self, norm: float) -> float:
        self.steps += 1
        if not math.isfinite(norm):
            raise ValueError(f"{type(self).__name__}.step: the gradient norm is not finite ({norm}); the step has been applied")
        return norm
