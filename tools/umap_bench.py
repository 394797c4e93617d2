"""The exact kNN of the HIP UMAP (vsom_umap_knn) and a whole UMAP(metric='cosine').fit_transform, timed on the device
at the shapes of visualize_umap_progression: MNIST clustering latents (70 000 x 196*16) and CIFAR (60 000 x 64*192).

    python tools/umap_bench.py [--shapes 70000x3136,60000x12288] [--k 15] [--reps 3] [--no-fit]

kNN FLOP = 2 N^2 D (the X X^T contraction; the top-k adds no FLOP), reported against the 157.3 TF f32 matrix-core
peak.  The fit is timed in phases: kNN, host graph (sigma / rho, membership, set operations), init (spectral) and
layout (all epochs).  Data: a rank-32 signal plus noise (clustered, like real latents).  One JSON line per shape."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_F32_TF = 157.3


def _data(N, D, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    X = torch.randn(N, 32, device="cuda", generator=g) @ torch.randn(32, D, device="cuda", generator=g)
    return X.add_(0.1 * torch.randn(N, D, device="cuda", generator=g)).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="70000x3136,60000x12288")
    ap.add_argument("--k", type=int, default=15)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-fit", action="store_true")
    a = ap.parse_args()
    from vit_som_amd import UMAP, ops, umap as U
    for shape in a.shapes.split(","):
        N, D = (int(v) for v in shape.split("x"))
        X = _data(N, D)
        idx = torch.empty(N, a.k, dtype=torch.int64, device="cuda")
        dist = torch.empty(N, a.k, dtype=torch.float32, device="cuda")
        ops.umap_knn(X, a.k, ops.DIST_COSINE, idx, dist)                     # warm-up (and workspace)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            ops.umap_knn(X, a.k, ops.DIST_COSINE, idx, dist)
        e1.record()
        torch.cuda.synchronize()
        knn_s = e0.elapsed_time(e1) / a.reps / 1e3
        tf = 2.0 * N * N * D / knn_s / 1e12
        res = {"N": N, "D": D, "k": a.k, "knn_s": round(knn_s, 4), "knn_TFLOPs": round(tf, 1),
               "knn_pct_of_f32_peak": round(100.0 * tf / PEAK_F32_TF, 1)}
        if not a.no_fit:
            m = UMAP(n_neighbors=a.k, min_dist=0.1, metric="cosine", random_state=42)
            torch.cuda.synchronize()
            t0 = time.time()
            m.fit_transform(X)
            torch.cuda.synchronize()
            res["fit_transform_s"] = round(time.time() - t0, 2)
            # phases, from the fitted object's host pieces
            t0 = time.time()
            G = U.fuzzy_simplicial_set(m._knn_indices, m._knn_dists, 1.0, 1.0)[0]
            res["host_graph_s"] = round(time.time() - t0, 2)
            t0 = time.time()
            m._initial(X, G.astype(np.float32), np.random.RandomState(42))
            res["init_s"] = round(time.time() - t0, 2)
            res["n_epochs"] = m._n_epochs
            res["graph_nnz"] = int(m.graph_.nnz)
        print(json.dumps(res), flush=True)
        del X, idx, dist
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
