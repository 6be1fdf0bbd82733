"""Recorder of tests/golden/frtail_reference.{npz,json}: the reference's own IResNet class driven through its embedding stage in float64.

    python tests/golden/make_frtail_reference.py <path to the reference's FR_training directory>

Run once on a CPU; no test imports this file and nothing on a GPU machine needs it.  It builds the reference's
iresnet18(num_features=64, dropout=0.4) in float64 train mode, sets the stage's parameters and a replacement for layer4's output (a
forward hook that returns the tensor) from frtail_oracle.case_inputs -- integer arithmetic, no RNG, so the test rebuilds the same
inputs instead of storing them --, captures the dropout mask from the dropout module's output, and drives backward with the formula
cotangent on F.normalize(model(x)).  Recorded: the bit-packed mask, the embeddings and the small gradients in full, the running
statistics and num_batches_tracked, and for fc.weight.grad and the input gradient their row sums, column sums and a strided sample."""
import importlib.util
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import frtail_oracle as TO  # noqa: E402

B, CH, HW, N, P, STRIDE = 4, 512, 49, 64, 0.4, 997


def main(ref_dir: str) -> None:
    spec = importlib.util.spec_from_file_location("ref_iresnet", os.path.join(ref_dir, "backbones", "iresnet.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    torch.manual_seed(20)
    model = mod.iresnet18(num_features=N, dropout=P).double().train()
    x, prm, _, g = TO.case_inputs(B, CH, HW, N, P)
    with torch.no_grad():
        for name in ("bn2", "features"):
            m = getattr(model, name)
            m.weight.copy_(torch.from_numpy(prm[f"{name}.weight"]))
            m.bias.copy_(torch.from_numpy(prm[f"{name}.bias"]))
            m.running_mean.copy_(torch.from_numpy(prm[f"{name}.running_mean"]))
            m.running_var.copy_(torch.from_numpy(prm[f"{name}.running_var"]))
        model.fc.weight.copy_(torch.from_numpy(TO.to_upstream(prm["fc.weight"], CH, HW)))
        model.fc.bias.copy_(torch.from_numpy(prm["fc.bias"]))
    fmap = torch.from_numpy(TO.to_upstream(x, CH, HW)).view(B, CH, 7, 7).requires_grad_(True)
    seen = {}
    model.layer4.register_forward_hook(lambda m, i, o: fmap)
    model.dropout.register_forward_pre_hook(lambda m, i: seen.__setitem__("in", i[0].detach().clone()))
    model.dropout.register_forward_hook(lambda m, i, o: seen.__setitem__("out", o.detach().clone()))
    emb = F.normalize(model(torch.zeros(B, 3, 112, 112, dtype=torch.float64)))
    assert bool((seen["in"] != 0).all()), "a bn2 output of exactly 0 hides its mask bit"
    keep = (seen["out"] != 0).numpy().astype(np.uint8)                     # upstream's flatten order
    emb.backward(torch.from_numpy(g).double())
    rec = {"keep_bits": np.packbits(keep.reshape(-1)), "embeddings": emb.detach().numpy()}
    for name, prm_t in (("bn2.weight", model.bn2.weight), ("bn2.bias", model.bn2.bias), ("fc.bias", model.fc.bias),
                        ("features.bias", model.features.bias)):
        rec[f"grad.{name}"] = prm_t.grad.numpy()
    for name, a in (("fc.weight", model.fc.weight.grad.numpy()), ("input", fmap.grad.reshape(B, CH * HW).numpy())):
        rec[f"grad.{name}.rowsum"], rec[f"grad.{name}.colsum"] = a.sum(1), a.sum(0)
        rec[f"grad.{name}.sample"] = a.reshape(-1)[::STRIDE].copy()
    for name in ("bn2", "features"):
        m = getattr(model, name)
        rec[f"running.{name}.running_mean"], rec[f"running.{name}.running_var"] = m.running_mean.numpy(), m.running_var.numpy()
    meta = {"B": B, "ch": CH, "hw": HW, "n": N, "p": P, "stride": STRIDE, "torch": torch.__version__,
            "features_weight_requires_grad": bool(model.features.weight.requires_grad),
            "features_weight_grad_is_none": model.features.weight.grad is None,
            "num_batches_tracked": {k: int(getattr(model, k).num_batches_tracked) for k in ("bn2", "features")},
            "kept_share": float(keep.mean())}
    np.savez_compressed(os.path.join(HERE, "frtail_reference.npz"), **rec)
    with open(os.path.join(HERE, "frtail_reference.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
    print(meta, {k: v.shape for k, v in rec.items()})


if __name__ == "__main__":
    main(sys.argv[1])
