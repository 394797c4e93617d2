"""One Lloyd iteration (vsom_kmeans_assign + vsom_kmeans_update) at the CIFAR-10 recon shape, and a whole
KMeans(n_init=10) fit, timed on the device.

    python tools/kmeans_bench.py [--n 50000] [--d 3072] [--k 10] [--iters 50] [--sklearn]

Bytes per iteration = X once (N*D*4) + labels / prev labels / mind + the slabs written and read back; the X-only
floor at 8 TB/s is N*D*4 / 8e12 (77 us at the default shape).  --sklearn also times sklearn's fit on the host CPUs."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=50000)
    ap.add_argument("--d", type=int, default=3072)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--sklearn", action="store_true")
    a = ap.parse_args()
    from vit_som_amd import KMeans, ops
    N, D, k = a.n, a.d, a.k
    g = torch.Generator(device="cuda").manual_seed(0)
    means = torch.randn(k, D, device="cuda", generator=g) * 3.0
    X = means[torch.randint(0, k, (N,), device="cuda", generator=g)] + torch.randn(N, D, device="cuda", generator=g)
    C = X[:k].clone()
    Cn = torch.empty_like(C)
    ws = torch.empty(ops.kmeans_workspace_bytes(N, D, k), dtype=torch.uint8, device="cuda")
    lab = torch.full((N,), -1, dtype=torch.int64, device="cuda")
    lab2 = torch.empty_like(lab)
    mind = torch.empty(N, dtype=torch.float32, device="cuda")
    counts = torch.empty(k, dtype=torch.int64, device="cuda")
    status = torch.empty(4, dtype=torch.float64, device="cuda")

    def one():
        ops.kmeans_assign(X, C, lab2, lab, mind, ws)
        ops.kmeans_update(C, Cn, N, mind, counts, status, ws)

    for _ in range(5):
        one()
    torch.cuda.synchronize()
    e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    e[0].record()
    for _ in range(a.iters):
        ops.kmeans_assign(X, C, lab2, lab, mind, ws)
    e[1].record()
    e[2].record()
    for _ in range(a.iters):
        one()
    e[3].record()
    torch.cuda.synchronize()
    t_assign = e[0].elapsed_time(e[1]) / a.iters * 1e3
    t_iter = e[2].elapsed_time(e[3]) / a.iters * 1e3
    G = min(256, -(-N // 32), max(1, (128 << 20) // (k * D * 4 + k * 4)))   # workgroups of vsom_kmeans_assign
    G = -(-N // -(-N // G))                                                   # rows split evenly: the ones launched
    x_bytes = N * D * 4
    moved = x_bytes + N * 8 * 2 + N * 4 + 2 * G * k * D * 4
    res = {"N": N, "D": D, "k": k, "assign_us": round(t_assign, 1), "iteration_us": round(t_iter, 1),
           "bytes_per_iter": moved, "GBps_iter": round(moved / t_iter / 1e3, 1), "GBps_X_only": round(x_bytes / t_iter / 1e3, 1),
           "floor_us_8TBps": round(x_bytes / 8e12 * 1e6, 1), "floor_us_6.29TBps": round(x_bytes / 6.29e12 * 1e6, 1)}
    torch.cuda.synchronize()
    t0 = time.time()
    km = KMeans(k, random_state=0, n_init=10).fit(X)
    torch.cuda.synchronize()
    res["fit_n_init10_s"] = round(time.time() - t0, 3)
    res["fit_n_iter_last_best"] = km.n_iter_
    if a.sklearn:
        from sklearn.cluster import KMeans as SK
        Xh = X.cpu().numpy()
        t0 = time.time()
        SK(n_clusters=k, random_state=0, n_init=10).fit(Xh)
        res["sklearn_fit_s"] = round(time.time() - t0, 2)
        res["host_cpus"] = len(os.sched_getaffinity(0))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
