"""Golden fixtures for ViTClassifier FROM THE REFERENCE ITSELF (build container only: needs the reference checkout).

Instantiates the unmodified reference ViTClassifier (models/vit.py:243-340) with the inert stand-ins of
oracle/gen_golden.py, on CPU at float32 matmul precision 'highest' (its constructor sets 'medium'), and writes ONLY
arrays to tests/golden/ref_vitcls_*.npz: config (JSON), parameters, three input batches with labels, logits, the
training loss and every non-None gradient, the names of the parameters whose gradient is None, the first group's
learning rate, the state after steps 1 and 3 of its own configure_optimizers(), validation loss / accuracy and the
state_dict key list.

    python -B tools/gen_golden_vitcls.py
"""
import copy
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.gen_golden import OUT, _install_stand_ins, make_config  # noqa: E402


def vit_config(*args, **kw):
    """A make_config() config reshaped to the reference's configs/vit/*.yaml schema (no gamma, no som)."""
    cfg = make_config(*args, **kw)
    hp = cfg["hyperparameters"]
    hp["model_arch"] = "vit"
    del hp["gamma"], hp["som"]
    return cfg


CASES = {
    # hd = 8: E 24, 3 heads, 8x8 images, p = 4 (N = 5), 5 classes
    "ref_vitcls_hd8": dict(cfg=vit_config(3, 8, 4, 24, 2, 3, 12, 1, (1, 1), 5, 5), B=5),
    # hd = 32: E 32, 1 head, 16x16 images, p = 4 (N = 17), 7 classes
    "ref_vitcls_hd32": dict(cfg=vit_config(3, 16, 4, 32, 2, 1, 8, 1, (1, 1), 7, 6), B=6),
}


def run_case(name, spec):
    from models.vit import ViTClassifier
    cfg = copy.deepcopy(spec["cfg"])
    torch.manual_seed(0)
    m = ViTClassifier(cfg)
    torch.set_float32_matmul_precision("highest")
    g = torch.Generator().manual_seed(321)
    with torch.no_grad():                       # non-trivial LayerNorm affines and biases
        for _, p in m.named_parameters():
            if p.requires_grad and p.ndim == 1:
                p.add_(0.1 * torch.randn(p.shape, generator=g))
    d = cfg["data"]
    B = spec["B"]
    xs = [torch.randn(B, d["num_channels"], d["input_size"], d["input_size"], generator=g) for _ in range(3)]
    ys = [torch.randint(0, d["num_classes"], (B,), generator=g) for _ in range(3)]
    out = {"config": np.array(json.dumps(cfg)), "state_keys": np.array(list(m.state_dict().keys()))}
    for k, v in m.state_dict().items():
        out["param/" + k] = v.detach().numpy().copy()
    for i in range(3):
        out[f"x{i}"], out[f"y{i}"] = xs[i].numpy(), ys[i].numpy()
    m.eval()
    with torch.no_grad():
        out["logits"] = m(xs[0]).numpy()
        vloss = m.validation_step((xs[1], ys[1]), 0)
        logits1 = m(xs[1])
        out["val_loss"] = np.float32(vloss.item())
        out["val_acc"] = np.float32((logits1.argmax(-1) == ys[1]).float().mean().item())
    m.train()
    (opt,), _ = m.configure_optimizers()
    out["lr0"] = np.float64(opt.param_groups[0]["lr"])
    none = []
    for step in range(3):
        opt.zero_grad(set_to_none=True)
        loss = m.training_step((xs[step], ys[step]), step)
        loss.backward()
        if step == 0:
            out["loss"] = np.float32(loss.item())
            for n, p in m.named_parameters():
                if not p.requires_grad:
                    continue
                if p.grad is None:
                    none.append(n)
                else:
                    out["grad/" + n] = p.grad.detach().numpy().copy()
        opt.step()
        if step in (0, 2):
            for n, p in m.named_parameters():
                if p.requires_grad:
                    out[f"step{step + 1}/" + n] = p.detach().numpy().copy()
    out["grad_none"] = np.array(none)
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path) / 1024:.0f} KiB, loss {out['loss']:.6f}, {len(none)} None gradients")


if __name__ == "__main__":
    _install_stand_ins()
    for name, spec in CASES.items():
        run_case(name, spec)
