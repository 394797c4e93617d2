"""Timing of the map-quality evaluators at the benchmark shapes (batch 512, 40 x 40 map, L = 12 288; profiles/r10_map_quality.txt).

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o mq -- python tools/map_quality_bench.py kernels
    python tools/map_quality_bench.py trace DIR/.../mq_kernel_trace.csv
    python tools/map_quality_bench.py wall [batches] [repeats]

kernels: vsom_map_stats on a [512, 1600] distance matrix and vsom_umatrix on 1600 prototypes of 12 288 values (cosine), REPS
times each, for a kernel trace; trace: their durations from that trace, the first WARM dropped, and what the bytes they have
to move make of them; wall: evaluate_map_quality against evaluate_clustering over the same loader of resident batches,
alternated in one process."""
import csv
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS, WARM = 30, 5
B, ROWS, COLS, L = 512, 40, 40, 12288
HBM_TBS = 8.0


def kernels():
    import torch
    from vit_som_amd import ops
    K = ROWS * COLS
    g = torch.Generator(device="cuda").manual_seed(0)
    dist = torch.rand(B, K, device="cuda", generator=g)
    bmu = dist.argmin(dim=1)
    gy, gx = torch.meshgrid(torch.arange(ROWS), torch.arange(COLS), indexing="ij")
    pos = torch.stack([gy, gx], dim=-1).view(-1, 2).float().cuda()
    W = torch.nn.functional.normalize(torch.rand(K, L, device="cuda", generator=g), dim=1)
    sums = torch.zeros(2 * K + 1, dtype=torch.int64, device="cuda")
    nearest = torch.full((K,), -1, dtype=torch.int64, device="cuda")
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    for i in range(REPS):
        ops.map_stats(dist, bmu, pos, 2.25, i * B, sums[:K], sums[K:2 * K], sums[2 * K:], nearest, bad)
        ops.umatrix(W, pos, 2.25, ops.DIST_COSINE)
    torch.cuda.synchronize()
    assert int(bad.item()) == 0 and int(sums[:K].sum()) == REPS * B


def trace(path):
    rows = list(csv.DictReader(open(path)))
    dur = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3                     # noqa: E731
    K = ROWS * COLS
    moved = {"map_stats_kernel": B * K * 4, "umatrix_kernel": K * L * 4}
    for name, nbytes in moved.items():
        t = [dur(r) for r in sorted(rows, key=lambda r: int(r["Start_Timestamp"])) if name in r["Kernel_Name"]]
        assert len(t) == REPS, (name, len(t))
        t = t[WARM:]
        med = statistics.median(t)
        print(f"{name:18s} median {med:7.1f} us  min {min(t):7.1f}  max {max(t):7.1f}   {nbytes / 1e6:5.1f} MB once -> "
              f"{nbytes / med / 1e3:6.0f} GB/s = {100 * nbytes / med / 1e3 / (1e3 * HBM_TBS):.1f} % of {HBM_TBS:.0f} TB/s")


def wall(batches, repeats):
    import torch
    import bench
    from vit_som_amd import ViTSOM
    from vit_som_amd.evaluation import evaluate_clustering, evaluate_map_quality
    cfg = bench.c3_config(B)
    torch.manual_seed(0)
    model = ViTSOM(cfg, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(1)
    loader = [(torch.rand(B, 3, 32, 32, device="cuda", generator=g), torch.randint(0, 10, (B,), device="cuda", generator=g))
              for _ in range(batches)]
    arms = {"evaluate_clustering": lambda: evaluate_clustering(model, cfg, loader),
            "evaluate_map_quality": lambda: evaluate_map_quality(model, cfg, loader)}
    times = {k: [] for k in arms}
    stdout, sys.stdout = sys.stdout, open(os.devnull, "w")              # the evaluators print their own line
    try:
        for rep in range(repeats + 1):                                  # the first round warms both arms up
            for name, fn in arms.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                if rep:
                    times[name].append((time.perf_counter() - t0) * 1e3)
    finally:
        sys.stdout = stdout
    for name, t in times.items():
        print(f"{name:22s} " + " ".join(f"{v:7.2f}" for v in t) + f"   median {statistics.median(t):7.2f} ms  min {min(t):7.2f}  max {max(t):7.2f}"
              f"  ({batches} batches of {B})")
    a, b = times["evaluate_map_quality"], times["evaluate_clustering"]
    print(f"ratio of medians map_quality / clustering {statistics.median(a) / statistics.median(b):.4f}; "
          f"spread (max - min) / median: map_quality {(max(a) - min(a)) / statistics.median(a):.4f}, "
          f"clustering {(max(b) - min(b)) / statistics.median(b):.4f}")


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "wall"
    if mode == "kernels":
        kernels()
    elif mode == "trace":
        trace(sys.argv[2])
    else:
        wall(int(sys.argv[2]) if len(sys.argv) > 2 else 20, int(sys.argv[3]) if len(sys.argv) > 3 else 5)
