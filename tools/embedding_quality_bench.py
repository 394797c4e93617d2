"""Timing of trustworthiness / continuity at the evaluation shape (profiles/r13_embedding_quality.txt).

    python tools/embedding_quality_bench.py [--out profiles/r13_embedding_quality.txt] [--repeats 7] [--host-n 3000]

kernels: vsom_knn_ranks (N = 10 000 rows, D = 12 288, k = 15, cosine; the neighbour table is the rows' own nearest 2-D
neighbours) against vsom_umap_knn at the same N, D and k -- the same contraction, the existing kernel: the yardstick -- and
the D = 2 rank pass (euclidean), alternated in one process, one warm-up round, device events around each call; reported per
call, as (row, row) pairs per second and, for D = 12 288, as a share of the 157.3 TF f32 matrix-core peak (FLOP = 2 x pairs
x D: the contraction alone).
end to end: embedding_quality(X, E) (both directions: two searches and two rank passes, the counts copied to the host and
folded there) by wall clock around calls that end in a device synchronise.
for scale: sklearn.manifold.trustworthiness on the host at --host-n rows of the same data (an N x N fp64 distance matrix
and a full argsort per row: what it can still hold), next to the device call at that size.
Everything is printed and written to --out."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_F32_TF = 157.3
N, D, K = 10000, 12288, 15


def _stats(t):
    med = statistics.median(t)
    return med, min(t), max(t), (max(t) - min(t)) / med


def _row(say, name, t, unit="ms"):
    med, lo, hi, spread = _stats(t)
    say(f"{name:24s} " + " ".join(f"{v:9.3f}" for v in t) + f"   median {med:9.3f}  min {lo:9.3f}  max {hi:9.3f}  spread {spread:.4f}  ({unit})")
    return med


def data():
    import torch
    g = torch.Generator(device="cuda").manual_seed(0)
    X = torch.randn(N, 32, device="cuda", generator=g) @ torch.randn(32, D, device="cuda", generator=g)
    X.add_(0.1 * torch.randn(N, D, device="cuda", generator=g))                         # clustered, like real latents
    E = (X[:, :2] / X[:, :2].std() + 0.3 * torch.randn(N, 2, device="cuda", generator=g)).contiguous()   # a 2-D picture of it
    return X, E


def kernels(X, E, repeats, say):
    import torch
    from vit_som_amd import ops
    idx, dist = torch.empty(N, K + 1, dtype=torch.int64, device="cuda"), torch.empty(N, K + 1, device="cuda")
    ops.umap_knn(E, K + 1, ops.DIST_EUCLIDEAN, idx, dist)
    nbr_e = idx[:, 1:].contiguous()                                                      # neighbours in E, to be ranked in X
    ops.umap_knn(X, K + 1, ops.DIST_COSINE, idx, dist)
    nbr_x = idx[:, 1:].contiguous()                                                      # neighbours in X, to be ranked in E
    less, tied = (torch.empty(N, K, dtype=torch.int32, device="cuda") for _ in range(2))
    ui, ud = torch.empty(N, K, dtype=torch.int64, device="cuda"), torch.empty(N, K, device="cuda")
    arms = {"vsom_knn_ranks D=12288": lambda: ops.knn_ranks(X, nbr_e, ops.DIST_COSINE, less, tied),
            "vsom_umap_knn D=12288": lambda: ops.umap_knn(X, K, ops.DIST_COSINE, ui, ud),
            "vsom_knn_ranks D=2": lambda: ops.knn_ranks(E, nbr_x, ops.DIST_EUCLIDEAN, less, tied),
            "vsom_umap_knn D=2": lambda: ops.umap_knn(E, K, ops.DIST_EUCLIDEAN, ui, ud)}
    times = {name: [] for name in arms}
    for rep in range(repeats + 1):                                                      # the first round warms every arm up
        for name, fn in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if rep:
                times[name].append(e0.elapsed_time(e1))
    say(f"## kernels: N {N}, k {K}; D 12288 cosine, D 2 euclidean; ms per call (device events; vsom_knn_ranks includes the host "
        f"wrapper's range check of the table, one reduction and synchronise), {repeats} repeats after one warm-up round, alternated")
    pairs = N * N
    rate = {}
    for name in arms:
        med = _row(say, name, times[name])
        rate[name] = pairs / (med * 1e-3)
        line = f"{'':24s} {pairs / 1e6:.0f} M pairs -> {rate[name] / 1e9:.3f} G pairs/s"
        if "12288" in name:
            tf = 2.0 * pairs * D / (med * 1e-3) / 1e12
            line += f", {tf:.1f} TF = {100 * tf / PEAK_F32_TF:.1f} % of the {PEAK_F32_TF} TF f32 matrix peak"
        say(line)
    say(f"pairs per second, vsom_knn_ranks / vsom_umap_knn: D=12288 {rate['vsom_knn_ranks D=12288'] / rate['vsom_umap_knn D=12288']:.4f}, "
        f"D=2 {rate['vsom_knn_ranks D=2'] / rate['vsom_umap_knn D=2']:.4f}")


def end_to_end(X, E, repeats, say):
    import torch
    from vit_som_amd.embedding_quality import embedding_quality
    times, got = [], []
    for rep in range(repeats + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        q = embedding_quality(X, E, n_neighbors=K, metric="cosine")
        torch.cuda.synchronize()
        if rep:
            times.append((time.perf_counter() - t0) * 1e3)
        got.append((q.trust_penalty, q.cont_penalty))
    say(f"## end to end: embedding_quality(X [{N}, {D}], E [{N}, 2], n_neighbors={K}, metric='cosine'); wall ms, {repeats} repeats "
        f"after one warm-up call")
    _row(say, "embedding_quality", times)
    say(f"trustworthiness {q.trustworthiness:.6f}, continuity {q.continuity:.6f}; every call the same penalties: {len(set(got)) == 1}")


def host_scale(X, E, n, say):
    import numpy as np
    import torch
    from sklearn.manifold import trustworthiness as sk_trust
    from vit_som_amd.embedding_quality import trustworthiness
    Xs, Es = X[:n].contiguous(), E[:n].contiguous()
    Xh, Eh = Xs.cpu().numpy().astype(np.float64), Es.cpu().numpy().astype(np.float64)
    t0 = time.perf_counter()
    want = sk_trust(Xh, Eh, n_neighbors=K, metric="cosine")
    host = time.perf_counter() - t0
    trustworthiness(Xs, Es, n_neighbors=K, metric="cosine")                              # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    got = trustworthiness(Xs, Es, n_neighbors=K, metric="cosine")
    torch.cuda.synchronize()
    dev = time.perf_counter() - t0
    say(f"## for scale: sklearn.manifold.trustworthiness(metric='cosine') on the host at N {n}, D {D} (one call, wall): {host:.3f} s "
        f"-> {want:.6f}; trustworthiness() on the device at that size: {dev * 1e3:.3f} ms -> {got:.6f} (difference {abs(got - want):.2e}: "
        f"fp32 against fp64 distances)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13_embedding_quality.txt"))
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--host-n", type=int, default=3000)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("embedding_quality_bench: no GPU; a timing taken anywhere else says nothing")
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)
    X, E = data()
    kernels(X, E, a.repeats, say)
    end_to_end(X, E, a.repeats, say)
    if a.host_n > 0:
        host_scale(X, E, a.host_n, say)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
