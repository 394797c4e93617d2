"""Timing of the variable-size device data pipeline (vit_som_amd/csrc/augment_ragged.hip) at flowers shapes: batch 128,
S = 224, synthetic sources with sides in 500 .. 700.

    ragged_ab.py kernels          REPS times: the training input of a step (vsom_augment_plan_ragged, crop 1, crop 2) and the
                                  evaluation transform, alternated (run it under rocprofv3 --kernel-trace --stats
                                  --output-format csv); prints the bytes each launch has to move and event timings
    ragged_ab.py trace FILE.csv   durations of the four launches from that run's kernel trace, with their share of the HBM rate
    ragged_ab.py fit [steps] [rounds]
                                  wall time per step of train.fit's inner loop for the vit_som_flowers-102 config at batch 128,
                                  fed by DeviceLoader over a ragged set and fed one resident batch (no input side),
                                  alternated in one process
"""
import csv
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS, WARM = 25, 5
B, S, R, C, N = 128, 224, 256, 3, 512
HBM_TBS = 8.0                                                 # MI355X peak, for the share column
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def synthetic_set(n, lo=500, hi=700, seed=0):
    """Random bytes, made on the device: n images with sides in lo .. hi."""
    import torch
    from vit_som_amd.data import RaggedDeviceDataset
    g = torch.Generator().manual_seed(seed)
    shapes = torch.randint(lo, hi + 1, (n, 2), generator=g, dtype=torch.int32)
    sizes = (C * shapes[:, 0].long() * shapes[:, 1].long() + 15) // 16 * 16
    offsets = torch.cumsum(sizes, 0) - sizes
    data = torch.randint(0, 256, (int(sizes.sum()),), dtype=torch.uint8, device="cuda")
    return RaggedDeviceDataset(data, offsets, shapes, torch.arange(n) % 102, C, "cuda")


def kernels():
    import torch
    from vit_som_amd import ops
    from vit_som_amd.data import DeviceTransform
    ds = synthetic_set(N)
    tr = DeviceTransform(True, C, S, MEAN, STD, variable_size=True)
    ev = DeviceTransform(False, C, S, MEAN, STD, variable_size=True)
    g = torch.Generator().manual_seed(1)
    index = torch.randperm(N, generator=g)[:B].cuda()
    out = torch.empty(B, C, S, S, device="cuda")
    params = torch.zeros(B, 16, dtype=torch.int32, device="cuda")
    scratch = torch.empty(ops.augment_ragged_scratch_bytes(B, C, S), dtype=torch.uint8, device="cuda")
    e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    t_train, t_eval = [], []
    for r in range(REPS):
        e[0].record()
        tr.apply(ds, index, out, params, 1, r, scratch=scratch)
        e[1].record()
        ev.apply(ds, index, out, None, 1, r)
        e[2].record()
        torch.cuda.synchronize()
        t_train.append(1e3 * e[0].elapsed_time(e[1]))
        t_eval.append(1e3 * e[1].elapsed_time(e[2]))
    p, shp = params.cpu().long(), ds.shapes[index].cpu().long()
    crop1, crop2 = int((C * p[:, 2] * p[:, 3]).sum()), int((C * p[:, 6] * p[:, 7]).sum())
    u8, f32 = B * C * S * S, 4 * B * C * S * S
    # evaluation: the rows and columns of the source the centre window reaches (window / resized size of each side)
    short = shp.min(1).values.double()
    oh, ow = (R * shp[:, 0] / short).floor(), (R * shp[:, 1] / short).floor()
    ev_in = int((C * (shp[:, 0] * S / oh).ceil() * (shp[:, 1] * S / ow).ceil()).sum())
    print(f"bytes of the last repetition's plan (B={B}, S={S}, sources {int(shp.min())} .. {int(shp.max())} px):")
    print(f"BYTES crop1 {crop1 + u8} (crop areas {crop1 / 1e6:.1f} MB in, scratch {u8 / 1e6:.1f} MB out)")
    print(f"BYTES crop2 {crop2 + f32} (crop areas of the scratch {crop2 / 1e6:.1f} MB in, fp32 {f32 / 1e6:.1f} MB out)")
    print(f"BYTES eval {ev_in + f32} (window's source region {ev_in / 1e6:.1f} MB in, fp32 {f32 / 1e6:.1f} MB out)")
    for name, t in (("training input (plan + crop 1 + crop 2)", t_train), ("evaluation transform", t_eval)):
        print(f"events around the launches, {name}: median {statistics.median(t[WARM:]):.1f} us, min {min(t[WARM:]):.1f}, max {max(t[WARM:]):.1f}")


def trace(path, bytes_of=None):
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    dur = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3                     # noqa: E731
    plan = [dur(r) for r in rows if "augment_plan_ragged_kernel" in r["Kernel_Name"]]
    passes = [dur(r) for r in rows if "ragged_pass_kernel" in r["Kernel_Name"]]
    assert len(plan) == REPS and len(passes) == 3 * REPS, (len(plan), len(passes))
    series = {"plan": plan, "crop1": passes[0::3], "crop2": passes[1::3], "eval": passes[2::3]}
    for name, d in series.items():
        t = d[WARM:]
        line = f"{name:6s} median {statistics.median(t):7.1f} us  min {min(t):7.1f}  max {max(t):7.1f}"
        if bytes_of and name in bytes_of:
            gbs = bytes_of[name] / statistics.median(t) / 1e3
            line += f"   {bytes_of[name] / 1e6:6.1f} MB -> {gbs:6.0f} GB/s = {100 * gbs / (1e3 * HBM_TBS):.1f} % of {HBM_TBS:.0f} TB/s"
        print(line)


def fit(steps, rounds):
    import torch
    from vit_som_amd import ViTSOM
    from vit_som_amd.data import DeviceLoader, DeviceTransform
    from vit_som_amd.train import load_config
    cfg = load_config(os.path.join(ROOT, "tests", "golden", "config_vit_som_flowers-102.yaml"))
    cfg["data"]["augment"].update(randaug_n=0, autoaugment=False)
    assert cfg["hyperparameters"]["batch_size"] == B and cfg["data"]["input_size"] == S
    torch.manual_seed(0)
    model = ViTSOM(cfg, device="cuda")
    model.set_schedule(8000, 10000)
    (opt,), _ = model.configure_optimizers()
    dev = model.arena.device
    ds = synthetic_set(B * 8)
    loader = DeviceLoader(ds, B, DeviceTransform.from_config(cfg, True, variable_size=True), shuffle=True, drop_last=True)
    xb0, yb0 = next(iter(loader))
    resident = [(xb0.clone(), yb0.clone())] * len(loader)

    def run(batches, k):
        torch.cuda.synchronize()
        t0, done = time.perf_counter(), 0
        while done < k:
            for xb, yb in batches:                                          # train.fit's inner loop
                model.train_step_fused(xb.to(dev, non_blocking=True), yb.to(dev, non_blocking=True))
                opt.step()
                done += 1
                if done == k:
                    break
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / k
    arms = {"one resident batch (no input side)": resident, "DeviceLoader over the ragged set": loader}
    res = {k: [] for k in arms}
    for a in arms.values():
        run(a, 3)
    for r in range(rounds):
        for k, a in arms.items():
            res[k].append(run(a, steps))
    for k, v in res.items():
        print(f"{k}: " + " ".join(f"{t:.3f}" for t in v) + f"  min {min(v):.3f} ms/step over {steps} steps")


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "kernels"
    if mode == "kernels":
        kernels()
    elif mode == "trace":
        given = dict(a.split("=") for a in sys.argv[3:])
        trace(sys.argv[2], {k: int(v) for k, v in given.items()} or None)
    else:
        fit(int(sys.argv[2]) if len(sys.argv) > 2 else 20, int(sys.argv[3]) if len(sys.argv) > 3 else 3)
