"""Timing of the device data pipeline (vit_som_amd/data.py).

    data_ab.py kernels            launch vsom_augment_plan + vsom_augment_batch (and, for the RandAugment cases,
                                  vsom_randaug_plan + vsom_augment_batch_ra) REPS times per case (run it under
                                  rocprofv3 --kernel-trace --stats --output-format csv); prints event timings too
    data_ab.py trace FILE.csv     per-case durations of the four kernels from that run's kernel trace
    data_ab.py primitives         device-event time of vsom_augment_batch_ra with one primitive in slot 0 of every sample
                                  (and the empty record), at the two-crop CIFAR / Tiny-ImageNet shapes
    data_ab.py fit [steps] [rounds]
                                  wall time of `steps` steps of train.fit's inner loop at the c3 benchmark shapes, fed by
                                  TensorLoader (CPU gather + copy, no augmentation), by DeviceLoader (gather +
                                  augmentation on the device) and by DeviceLoader with auto_augment (RandAugment and
                                  timm's rand-m9 as well), alternated in one process
"""
import csv
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

REPS, WARM = 25, 5
# (name, C, H, S, B, two crops, evaluation geometry, RandAugment(2) + rand-m9)
CASES = [("cifar 3x32x32 B=512, one crop", 3, 32, 32, 512, False, False, False),
         ("cifar 3x32x32 B=512, two crops", 3, 32, 32, 512, True, False, False),
         ("cifar 3x32x32 B=512, evaluation (32 -> 36 -> window)", 3, 32, 32, 512, False, True, False),
         ("tiny-imagenet 3x64x64 B=256, one crop", 3, 64, 64, 256, False, False, False),
         ("tiny-imagenet 3x64x64 B=256, two crops", 3, 64, 64, 256, True, False, False),
         ("tiny-imagenet 3x64x64 B=256, evaluation (64 -> 73 -> window)", 3, 64, 64, 256, False, True, False),
         ("cifar 3x32x32 B=512, two crops + RandAugment(2) + rand-m9", 3, 32, 32, 512, True, False, True),
         ("tiny-imagenet 3x64x64 B=256, two crops + RandAugment(2) + rand-m9", 3, 64, 64, 256, True, False, True)]
# which cases launch a kernel: the evaluation transform has no plan, the RandAugment cases use the kernels of their own
KERNELS = {"augment_batch_kernel": lambda c: not c[7], "augment_plan_kernel": lambda c: not c[6],
           "augment_batch_ra_kernel": lambda c: c[7], "randaug_plan_kernel": lambda c: c[7]}


def case_bytes(C, H, S, B):
    return B * C * H * H, B * C * S * S * 4


def kernels():
    import torch
    from vit_som_amd.data import DeviceDataset, DeviceTransform
    g = torch.Generator().manual_seed(0)
    for name, C, H, S, B, two, ev, ra in CASES:
        ds = DeviceDataset(torch.randint(0, 256, (4 * B, C, H, H), dtype=torch.uint8, generator=g), torch.zeros(4 * B, dtype=torch.int64))
        tr = DeviceTransform(not ev, C, S, (0.4914, 0.4822, 0.4465), (0.2023, 0.1994, 0.2010), two_stage=two, auto_augment=ra,
                             randaug_n=2, autoaugment=True)
        index = torch.randperm(4 * B, generator=g)[:B].cuda()
        out = torch.empty(B, C, S, S, device="cuda")
        params = torch.zeros(B, 16, dtype=torch.int32, device="cuda")
        rec = torch.zeros(B, 72, dtype=torch.int32, device="cuda") if ra else None
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ts = []
        for r in range(REPS):
            ev0.record()
            tr.apply(ds, index, out, params, 1, r, ra=rec)
            ev1.record()
            torch.cuda.synchronize()
            ts.append(1e3 * ev0.elapsed_time(ev1))
        rd, wr = case_bytes(C, H, S, B)
        print(f"{name}: {rd / 1e6:.2f} MB in, {wr / 1e6:.2f} MB out; events around the launches: median {statistics.median(ts[WARM:]):.1f} us, "
              f"min {min(ts[WARM:]):.1f} us")


PRIMITIVES = ("none", "affine NEAREST (rotate 9)", "affine BICUBIC (rotate 27)", "brightness", "color", "contrast", "sharpness",
              "posterize", "solarize", "solarize-add", "invert", "autocontrast", "equalize")


def primitives():
    import math
    import numpy as np
    import torch
    from vit_som_amd import ops
    g = torch.Generator().manual_seed(0)
    for name, C, H, S, B, two, ev, ra in CASES:
        if not ra:
            continue
        src = torch.randint(0, 256, (4 * B, C, H, H), dtype=torch.uint8, generator=g).cuda()
        index = torch.randperm(4 * B, generator=g)[:B].cuda()
        mean, std = torch.tensor((0.4914, 0.4822, 0.4465), device="cuda"), torch.tensor((0.2023, 0.1994, 0.2010), device="cuda")
        out = torch.empty(B, C, S, S, device="cuda")
        params = torch.zeros(B, 16, dtype=torch.int32, device="cuda")
        lr = (math.log(0.75), math.log(4 / 3))
        ops.augment_plan(index, params, 4 * B, H, S, (0.08, 1.0), lr, (0.08, 1.0), lr, 0.5, 0.25, 1, 0)
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        print(name)
        for op, label in enumerate(PRIMITIVES):
            row = np.zeros(72, np.int32)
            t = -math.radians((9.0 if op == 1 else 27.0) % 360.0)
            c, sn, cx = math.cos(t), math.sin(t), S / 2.0
            a = (c, sn, cx - (c * cx + sn * cx), -sn, c, cx - (-sn * cx + c * cx)) if op in (1, 2) else (0.0,) * 6
            row[8:12] = [op, 4 if op == 7 else 100, np.array(1.27, np.float32).view(np.int32), 125 | 123 << 8 | 114 << 16]
            row[12:24] = np.array(a, np.float64).view(np.int32)
            rec = torch.from_numpy(np.tile(row, (B, 1))).cuda()
            ts = []
            for r in range(REPS):
                ev0.record()
                ops.augment_batch_ra(src, index, params, rec, out, S, mean, std, 1, 0)
                ev1.record()
                torch.cuda.synchronize()
                ts.append(1e3 * ev0.elapsed_time(ev1))
            print(f"    {label:28s} median {statistics.median(ts[WARM:]):6.1f} us  min {min(ts[WARM:]):6.1f}")


def trace(path):
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    for kernel, launches in KERNELS.items():
        d = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if kernel in r["Kernel_Name"]]
        cases = [c for c in CASES if launches(c)]
        assert len(d) == REPS * len(cases), (kernel, len(d))
        for k, c in enumerate(cases):
            t = d[k * REPS + WARM:(k + 1) * REPS]
            print(f"{kernel:24s} {c[0]:66s} median {statistics.median(t):6.1f} us  min {min(t):6.1f}  max {max(t):6.1f}")


def fit(steps, rounds):
    import torch
    import bench
    from vit_som_amd import ViTSOM
    from vit_som_amd.data import DeviceDataset, DeviceLoader, DeviceTransform
    from vit_som_amd.train import TensorLoader
    cfg = bench.c3_config(512)
    cfg["data"]["augment"] = {"horizontal_flip": 0.5, "randaug_n": 0, "resize_scale": [0.08, 1.0], "resize_ratio": [0.75, 1.3333],
                              "reprob": 0.25, "remode": "pixel", "recount": 1, "autoaugment": False}
    torch.manual_seed(0)
    model = ViTSOM(cfg, device="cuda")
    model.set_schedule(50000, 10000)
    (opt,), _ = model.configure_optimizers()
    dev = model.arena.device
    n = 512 * 100
    g = torch.Generator().manual_seed(0)
    u8 = torch.randint(0, 256, (n, 3, 32, 32), dtype=torch.uint8, generator=g)
    y = torch.randint(0, 10, (n,), generator=g)
    full = {"data": dict(cfg["data"], augment=dict(cfg["data"]["augment"], randaug_n=2, autoaugment=True))}
    ds = DeviceDataset(u8, y, dev)
    loaders = {"TensorLoader": TensorLoader(u8.float().div_(255), y, 512, shuffle=True, drop_last=True),
               "DeviceLoader": DeviceLoader(ds, 512, DeviceTransform.from_config(cfg, True), shuffle=True, drop_last=True),
               "DeviceLoader + RandAugment(2) + rand-m9": DeviceLoader(ds, 512, DeviceTransform.from_config(full, True, auto_augment=True),
                                                                       shuffle=True, drop_last=True)}

    def run(loader, k):
        torch.cuda.synchronize()
        t0, done = time.perf_counter(), 0
        while done < k:
            for xb, yb in loader:                                           # train.fit's inner loop
                model.train_step_fused(xb.to(dev, non_blocking=True), yb.to(dev, non_blocking=True))
                opt.step()
                done += 1
                if done == k:
                    break
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / k
    res = {k: [] for k in loaders}
    for k, l in loaders.items():
        run(l, 5)
    for r in range(rounds):
        for k, l in loaders.items():
            res[k].append(run(l, steps))
    for k, v in res.items():
        print(f"{k}: " + " ".join(f"{t:.3f}" for t in v) + f"  min {min(v):.3f} ms/step over {steps} steps")


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "kernels"
    if mode == "kernels":
        kernels()
    elif mode == "primitives":
        primitives()
    elif mode == "trace":
        trace(sys.argv[2])
    else:
        fit(int(sys.argv[2]) if len(sys.argv) > 2 else 200, int(sys.argv[3]) if len(sys.argv) > 3 else 3)
