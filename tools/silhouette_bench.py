"""Timing of the silhouette coefficient at the evaluation shape (profiles/r14_silhouette.txt).

    python tools/silhouette_bench.py [--out profiles/r14_silhouette.txt] [--repeats 7] [--host-n 3000]

kernels: vsom_silhouette (N = 10 000 rows; C = 10 and C = 1 600 clusters; the labels sorted -- long runs of equal adjacent
labels, one atomic per row and 64 columns -- and shuffled -- a run head in almost every lane) against vsom_knn_ranks (k = 15)
at the same N and D: the same contraction with an epilogue of comparable work, the yardstick.  D = 12 288 (cosine), D = 192
and D = 2 (euclidean), alternated in one process, one warm-up round, device events around each call; reported per call,
as (row, row) pairs per second and, for D = 12 288, as a share of the 157.3 TF f32 matrix-core peak (FLOP = 2 x pairs x D:
the contraction alone).  Both wrappers end in one host synchronisation (the rank pass checks its table, the silhouette
reads its status), inside the timed span.
the row sort: cluster_silhouette on shuffled labels with sort_rows on and off, wall clock around calls that end in a device
synchronise: the A/B behind the wrapper's default.
for scale: sklearn.metrics.silhouette_score on the host at --host-n rows of the same data, next to the device call.
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


def _row(say, name, t, unit="ms"):
    med = statistics.median(t)
    say(f"{name:34s} " + " ".join(f"{v:9.3f}" for v in t) + f"   median {med:9.3f}  min {min(t):9.3f}  max {max(t):9.3f}  "
        f"spread {(max(t) - min(t)) / med:.4f}  ({unit})")
    return med


def data():
    import torch
    g = torch.Generator(device="cuda").manual_seed(0)
    X = torch.randn(N, 32, device="cuda", generator=g) @ torch.randn(32, D, device="cuda", generator=g)
    X.add_(0.1 * torch.randn(N, D, device="cuda", generator=g))                         # clustered, like real latents
    return X


def labels(C):
    import torch
    g = torch.Generator(device="cuda").manual_seed(C)
    y = torch.randint(0, C, (N,), device="cuda", generator=g)
    return {"sorted": torch.sort(y).values.contiguous(), "shuffled": y}


def kernels(X, repeats, say):
    import torch
    from vit_som_amd import ops
    arms = {}
    for d, metric, name in ((D, ops.DIST_COSINE, "cosine"), (192, ops.DIST_EUCLIDEAN, "euclidean"), (2, ops.DIST_EUCLIDEAN, "euclidean")):
        A = X if d == D else X[:, :d].contiguous()
        g = torch.Generator(device="cuda").manual_seed(d)
        nbr = torch.randint(0, N, (N, K), device="cuda", generator=g)
        less, tied = (torch.empty(N, K, dtype=torch.int32, device="cuda") for _ in range(2))
        arms[f"vsom_knn_ranks D={d}"] = (lambda A=A, nbr=nbr, less=less, tied=tied, metric=metric: ops.knn_ranks(A, nbr, metric, less, tied))
        for C in (10, 1600):
            for order, y in labels(C).items():
                if d != D and (C, order) not in ((10, "sorted"), (10, "shuffled")):
                    continue
                arms[f"vsom_silhouette D={d} C={C} {order}"] = (lambda A=A, y=y, metric=metric, C=C: ops.silhouette(A, y, metric, C))
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
    say(f"## kernels: N {N}, k {K}; D 12288 cosine, D 192 and D 2 euclidean; ms per call (device events; both wrappers include one "
        f"host synchronisation), {repeats} repeats after one warm-up round, alternated")
    pairs = N * N
    med = {}
    for name in arms:
        med[name] = _row(say, name, times[name])
        line = f"{'':34s} {pairs / 1e6:.0f} M pairs -> {pairs / (med[name] * 1e-3) / 1e9:.3f} G pairs/s"
        if "12288" in name:
            tf = 2.0 * pairs * D / (med[name] * 1e-3) / 1e12
            line += f", {tf:.1f} TF = {100 * tf / PEAK_F32_TF:.1f} % of the {PEAK_F32_TF} TF f32 matrix peak"
        say(line)
    say("time per call, vsom_silhouette / vsom_knn_ranks at the same D:")
    for name in arms:
        if "silhouette" in name:
            d = name.split("D=")[1].split()[0]
            say(f"  {name:34s} {med[name] / med[f'vsom_knn_ranks D={d}']:.4f}")


def row_sort(X, repeats, say):
    import torch
    from vit_som_amd.silhouette import cluster_silhouette
    say(f"## the row sort: cluster_silhouette(X [{N}, {D}], shuffled labels, metric='cosine'), sort_rows on / off; wall ms, {repeats} "
        f"repeats after one warm-up call, alternated; the sorted copy of X is {N * D * 4 / 2 ** 20:.0f} MiB")
    for C in (10, 1600):
        y = labels(C)["shuffled"]
        times, scores = {True: [], False: []}, set()
        for rep in range(repeats + 1):
            for sort in (True, False):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                r = cluster_silhouette(X, y, metric="cosine", sort_rows=sort)
                torch.cuda.synchronize()
                if rep:
                    times[sort].append((time.perf_counter() - t0) * 1e3)
                scores.add(r.score)
        on, off = _row(say, f"C={C} sort_rows=True", times[True]), _row(say, f"C={C} sort_rows=False", times[False])
        say(f"{'':34s} on / off {on / off:.4f}; score {r.score:.6f}, the same value from every call: {len(scores) == 1}")


def host_scale(X, n, say):
    import numpy as np
    import torch
    from sklearn.metrics import silhouette_score as sk_score
    from vit_som_amd.silhouette import silhouette_score
    Xs, y = X[:n].contiguous(), labels(10)["shuffled"][:n].contiguous()
    Xh, yh = Xs.cpu().numpy().astype(np.float64), y.cpu().numpy()
    t0 = time.perf_counter()
    want = sk_score(Xh, yh, metric="cosine")
    host = time.perf_counter() - t0
    silhouette_score(Xs, y, metric="cosine")                                             # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    got = silhouette_score(Xs, y, metric="cosine")
    torch.cuda.synchronize()
    dev = time.perf_counter() - t0
    say(f"## for scale: sklearn.metrics.silhouette_score(metric='cosine') on the host at N {n}, D {D}, 10 clusters (one call, wall; "
        f"the copy of the rows to the host not counted): {host:.3f} s -> {want:.6f}; silhouette_score() on the device at that size: "
        f"{dev * 1e3:.3f} ms -> {got:.6f} (difference {abs(got - want):.2e}: fp32 against fp64 distances)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14_silhouette.txt"))
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--host-n", type=int, default=3000)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("silhouette_bench: no GPU; a timing taken anywhere else says nothing")
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)
    X = data()
    kernels(X, a.repeats, say)
    row_sort(X, a.repeats, say)
    if a.host_n > 0:
        host_scale(X, a.host_n, say)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
