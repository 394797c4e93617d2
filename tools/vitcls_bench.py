"""ViTClassifier step time at the vit_cifar-10 (B 128, N 65) and vit_cifar-100 (B 512, N 257) shapes, with the pruned
last block (tuning.hooks.cls_prune) on and off, alternated in one process; and the single-query attention kernels
alone against their HBM floors (K and V read once in the forward; read once and written once in the backward).

    python tools/vitcls_bench.py [--steps 30] [--rounds 5]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vit_som_amd  # noqa: E402
from vit_som_amd import ops  # noqa: E402
from vit_som_amd.tuning import hooks  # noqa: E402

HBM_TBPS = 6.29          # MI355X peak HBM bandwidth (TB/s), the floors' denominator


def config(p, B, classes):
    return {"hyperparameters": {"model_arch": "vit", "total_epochs": 100, "batch_size": B,
                                "vit": {"patch_size": p, "emb_dim": 192, "depth": 12, "dec_emb_dim": 96, "dec_depth": 2,
                                        "heads": 3, "mlp_ratio": 4},
                                "optimizer": {"type": "adamw", "lr": 1e-3, "min_lr": 1e-6, "beta_1": 0.9, "beta_2": 0.999,
                                              "scheduler": "cosine_annealing", "warmup_epochs": 25, "weight_decay": 0.05,
                                              "layer_decay": 0.75, "smoothing": 0.1}},
            "data": {"dataset": "bench", "num_classes": classes, "num_channels": 3, "input_size": 32}}


def time_steps(m, opt, x, y, steps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(steps):
        m.train_step_fused(x, y)
        opt.step()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / steps


def time_kernel(fn, reps=50):
    fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    out = {}
    for name, p, B, classes in (("vit_cifar-10", 4, 128, 10), ("vit_cifar-100", 2, 512, 100)):
        torch.manual_seed(0)
        m = vit_som_amd.ViTClassifier(config(p, B, classes), device="cuda:0")
        (opt,), _ = m.configure_optimizers()
        x, y = torch.randn(B, 3, 32, 32, device="cuda"), torch.randint(0, classes, (B,), device="cuda")
        res = {True: [], False: []}
        try:
            for prune in (True, False):                                   # warm-up of both variants
                hooks.set(cls_prune=prune)
                time_steps(m, opt, x, y, 3)
            for _ in range(a.rounds):
                for prune in (True, False):
                    hooks.set(cls_prune=prune)
                    res[prune].append(time_steps(m, opt, x, y, a.steps))
        finally:
            hooks.reset()
        N, E, H, hd = (32 // p) ** 2 + 1, 192, 3, 64
        q, kv = torch.randn(B, E, device="cuda"), torch.randn(B * N, 2 * E, device="cuda")
        o, lse, do = torch.empty(B, E, device="cuda"), torch.empty(B, H, device="cuda"), torch.randn(B, E, device="cuda")
        dq, dkv = torch.empty(B, E, device="cuda"), torch.empty(B * N, 2 * E, device="cuda")
        fwd_us = time_kernel(lambda: ops.attention_q1_fwd(q, kv, o, lse, B, N, H, hd))
        bwd_us = time_kernel(lambda: ops.attention_q1_bwd(do, o, lse, q, kv, dq, dkv, B, N, H, hd))
        kv_bytes = kv.numel() * 4
        fwd_floor, bwd_floor = kv_bytes / (HBM_TBPS * 1e6), 2 * kv_bytes / (HBM_TBPS * 1e6)
        out[name] = {
            "B": B, "N": N,
            "ms_per_step_pruned": {"median": float(np.median(res[True])), "min": float(np.min(res[True])),
                                   "max": float(np.max(res[True]))},
            "ms_per_step_full": {"median": float(np.median(res[False])), "min": float(np.min(res[False])),
                                 "max": float(np.max(res[False]))},
            "q1_fwd_us": fwd_us, "q1_fwd_floor_us": fwd_floor, "q1_fwd_floor_fraction": fwd_floor / fwd_us,
            "q1_bwd_us": bwd_us, "q1_bwd_floor_us": bwd_floor, "q1_bwd_floor_fraction": bwd_floor / bwd_us,
        }
        del m, opt
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
