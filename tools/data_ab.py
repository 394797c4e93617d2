"""Timing of the device data pipeline (vit_som_amd/data.py).

    data_ab.py kernels            launch vsom_augment_plan + vsom_augment_batch REPS times per case (run it under
                                  rocprofv3 --kernel-trace --stats --output-format csv); prints event timings too
    data_ab.py trace FILE.csv     per-case durations of the two kernels from that run's kernel trace
    data_ab.py fit [steps] [rounds]
                                  wall time of `steps` steps of train.fit's inner loop at the c3 benchmark shapes, fed by
                                  TensorLoader (CPU gather + copy, no augmentation) and by DeviceLoader (gather +
                                  augmentation on the device), alternated in one process
"""
import csv
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

REPS, WARM = 25, 5
# (name, C, H, S, B, two crops, evaluation geometry)
CASES = [("cifar 3x32x32 B=512, one crop", 3, 32, 32, 512, False, False),
         ("cifar 3x32x32 B=512, two crops", 3, 32, 32, 512, True, False),
         ("cifar 3x32x32 B=512, evaluation (32 -> 36 -> window)", 3, 32, 32, 512, False, True),
         ("tiny-imagenet 3x64x64 B=256, one crop", 3, 64, 64, 256, False, False),
         ("tiny-imagenet 3x64x64 B=256, two crops", 3, 64, 64, 256, True, False),
         ("tiny-imagenet 3x64x64 B=256, evaluation (64 -> 73 -> window)", 3, 64, 64, 256, False, True)]


def case_bytes(C, H, S, B):
    return B * C * H * H, B * C * S * S * 4


def kernels():
    import torch
    from vit_som_amd.data import DeviceDataset, DeviceTransform
    g = torch.Generator().manual_seed(0)
    for name, C, H, S, B, two, ev in CASES:
        ds = DeviceDataset(torch.randint(0, 256, (4 * B, C, H, H), dtype=torch.uint8, generator=g), torch.zeros(4 * B, dtype=torch.int64))
        tr = DeviceTransform(not ev, C, S, (0.4914, 0.4822, 0.4465), (0.2023, 0.1994, 0.2010), two_stage=two)
        index = torch.randperm(4 * B, generator=g)[:B].cuda()
        out = torch.empty(B, C, S, S, device="cuda")
        params = torch.zeros(B, 16, dtype=torch.int32, device="cuda")
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ts = []
        for r in range(REPS):
            ev0.record()
            tr.apply(ds, index, out, params, 1, r)
            ev1.record()
            torch.cuda.synchronize()
            ts.append(1e3 * ev0.elapsed_time(ev1))
        rd, wr = case_bytes(C, H, S, B)
        print(f"{name}: {rd / 1e6:.2f} MB in, {wr / 1e6:.2f} MB out; events around the launches: median {statistics.median(ts[WARM:]):.1f} us, "
              f"min {min(ts[WARM:]):.1f} us")


def trace(path):
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    for kernel in ("augment_batch_kernel", "augment_plan_kernel"):
        d = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if kernel in r["Kernel_Name"]]
        cases = [c for c in CASES if kernel == "augment_batch_kernel" or not c[6]]          # no plan in the evaluation transform
        assert len(d) == REPS * len(cases), (kernel, len(d))
        for k, c in enumerate(cases):
            t = d[k * REPS + WARM:(k + 1) * REPS]
            print(f"{kernel:22s} {c[0]:58s} median {statistics.median(t):6.1f} us  min {min(t):6.1f}  max {max(t):6.1f}")


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
    loaders = {"TensorLoader": TensorLoader(u8.float().div_(255), y, 512, shuffle=True, drop_last=True),
               "DeviceLoader": DeviceLoader(DeviceDataset(u8, y, dev), 512, DeviceTransform.from_config(cfg, True), shuffle=True, drop_last=True)}

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
    elif mode == "trace":
        trace(sys.argv[2])
    else:
        fit(int(sys.argv[2]) if len(sys.argv) > 2 else 200, int(sys.argv[3]) if len(sys.argv) > 3 else 3)
