"""HDBSCAN (csrc/knn.hip's HDBSCAN section, vit_som_amd/hdbscan.py) at the sizes users run, on one GPU.

    python tools/hdbscan_bench.py [--out FILE] [--repeats 7] [--rows 10000] [--big-rows 70000] [--host-n 3000]

one round: ops.hdbscan_nearest (the first round: every row its own component) against ops.dbscan_neighbours at the same
shape -- the same contraction with another epilogue, the yardstick -- at (N, 12 288) and (N, 2), both metrics, both entries
timed in the same process, alternated after one warm-up round, device events around single calls.
merge step: ops.hdbscan_merge after that round, device events; the state is rebuilt (untimed) before every repeat.
rounds: the rounds a whole tree takes on a ten-blob set and on a chain of N points at unit spacing in shuffled order.
host: the time of everything after the tree (hdbscan.tree_to_labels: sort, single linkage, condensed tree, selection,
labels) on the edges of a fit, wall clock, at (N, 2) and (--big-rows, 2).
whole fit: HDBSCAN(min_cluster_size=50).fit, wall clock around calls that end in a device synchronise.
host, for scale: sklearn.cluster.HDBSCAN on --host-n rows, one call, with the adjusted Rand index between the two.
Everything is printed and written to --out."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from dbscan_bench import _blobs, _chain, _row, _timed  # noqa: E402  (the DBSCAN benchmark's fixtures and timing loop)

MIN_SAMPLES = 5


def _state(N):
    import torch
    from vit_som_amd import ops
    new = lambda dtype, *shape: torch.empty(*shape, dtype=dtype, device="cuda")      # noqa: E731
    s = dict(comp=new(torch.int32, N), edges=new(torch.int32, N, 3), record=new(torch.int32, 4), best=new(torch.int64, N),
             work=new(torch.int64, ops.hdbscan_work(N)), sq=new(torch.float32, N))
    ops.hdbscan_init(s["comp"], s["edges"], s["record"])
    return s


def _core(X, metric):
    import torch
    from vit_som_amd import ops
    N = X.shape[0]
    idx = torch.empty(N, MIN_SAMPLES, dtype=torch.int64, device="cuda")
    dist = torch.empty(N, MIN_SAMPLES, dtype=torch.float32, device="cuda")
    ops.umap_knn(X, MIN_SAMPLES, metric, idx, dist)
    return dist[:, MIN_SAMPLES - 1].contiguous()


def one_round(N, D, repeats, say):
    import torch
    from vit_som_amd import k_distances, ops
    X = _blobs(N, D)
    new = lambda dtype, *shape: torch.empty(*shape, dtype=dtype, device="cuda")      # noqa: E731
    sq, adj, count, status = new(torch.float32, N), new(torch.int64, N, ops.dbscan_words(N)), new(torch.int32, N), new(torch.int64, 2)
    say(f"## one round: X f32 [{N}, {D}]; vsom_hdbscan_nearest (first round, min_samples {MIN_SAMPLES}) against vsom_dbscan_neighbours; ms per "
        f"call (device events), {repeats} repeats after one warm-up round, alternated; then vsom_hdbscan_merge after that round")
    for name, metric in (("euclidean", ops.DIST_EUCLIDEAN), ("cosine", ops.DIST_COSINE)):
        eps = float(k_distances(X, 4, name)[N // 2])
        core, s = _core(X, metric), _state(N)
        arms = {"nearest": lambda: ops.hdbscan_nearest(X, metric, core, s["comp"], s["sq"], s["best"], s["record"]),
                "neighbours": lambda: ops.dbscan_neighbours(X, metric, eps, sq, adj, count, status)}
        times = _timed(arms, repeats)
        a = _row(say, f"vsom_hdbscan_nearest {name}", times["nearest"])
        b = _row(say, f"vsom_dbscan_neighbours {name}", times["neighbours"])
        spread = max((max(t) - min(t)) / statistics.median(t) for t in times.values())
        say(f"{'':40s} nearest / neighbours = {a / b:.3f} (the larger spread {spread:.3f}); {N * N / (a * 1e-3) / 1e9:.2f} G pairs/s, "
            f"{2.0 * N * N * D / (a * 1e-3) / 1e12:.1f} TF")
        merges = []
        for rep in range(repeats + 1):
            ops.hdbscan_init(s["comp"], s["edges"], s["record"])
            ops.hdbscan_nearest(X, metric, core, s["comp"], s["sq"], s["best"], s["record"])
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            ops.hdbscan_merge(s["best"], s["comp"], s["edges"], s["work"], s["record"])
            e1.record()
            torch.cuda.synchronize()
            if rep:
                merges.append(e0.elapsed_time(e1))
        _row(say, f"vsom_hdbscan_merge {name}", merges)
        say(f"{'':40s} after it: components left / edges / bad rows / rounds {s['record'].tolist()}")
    return X


def rounds_needed(X, what, say):
    import torch
    from vit_som_amd import ops
    from vit_som_amd.hdbscan import round_limit, spanning_tree
    core = _core(X, ops.DIST_EUCLIDEAN)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    edges, rounds = spanning_tree(X, core, ops.DIST_EUCLIDEAN)
    wall = (time.perf_counter() - t0) * 1e3
    say(f"{what:40s} {rounds} rounds (limit {round_limit(X.shape[0])}, ceil(log2 N) + 1), {len(edges)} edges, {wall:.1f} ms wall for the rounds "
        f"(one host read each)")


def fits(X, repeats, say, mcs=50):
    import torch
    from vit_som_amd import HDBSCAN
    from vit_som_amd.hdbscan import tree_to_labels
    N = X.shape[0]
    times, last = [], None
    for rep in range(repeats + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        hd = HDBSCAN(min_cluster_size=mcs, min_samples=MIN_SAMPLES).fit(X)
        torch.cuda.synchronize()
        if rep:
            times.append((time.perf_counter() - t0) * 1e3)
        assert last is None or torch.equal(last, hd.labels_), "two fits differ"
        last = hd.labels_
    _row(say, f"HDBSCAN.fit [{N}, {X.shape[1]}]", times)
    lo, hi, w = hd._edges
    host = []
    for _ in range(min(repeats, 3)):
        t0 = time.perf_counter()
        tree_to_labels(lo, hi, w, N, mcs)
        host.append((time.perf_counter() - t0) * 1e3)
    _row(say, f"  of which host tree / condense / labels", host)
    say(f"{'':40s} {hd.n_clusters_} clusters, {hd.n_noise_} noise rows, {hd.n_rounds_} rounds; every repeat gave the same labels")


def host_part(say, n, D):
    import numpy as np
    import torch
    from sklearn.cluster import HDBSCAN as SK
    from sklearn.metrics import adjusted_rand_score
    from vit_som_amd import HDBSCAN
    X = _blobs(n, D)
    Xh = X.cpu().numpy().astype(np.float64)
    t0 = time.perf_counter()
    sk = SK(min_cluster_size=50, min_samples=MIN_SAMPLES, algorithm="brute").fit(Xh)
    host = time.perf_counter() - t0
    HDBSCAN(min_cluster_size=50, min_samples=MIN_SAMPLES).fit(X)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    hd = HDBSCAN(min_cluster_size=50, min_samples=MIN_SAMPLES).fit(X)
    torch.cuda.synchronize()
    dev = time.perf_counter() - t0
    mine = hd.labels_.cpu().numpy()
    say(f"## for scale: N {n}, D {D}, euclidean, min_cluster_size 50, min_samples {MIN_SAMPLES}, one call each, wall ({os.cpu_count()} CPUs "
        f"visible): sklearn.cluster.HDBSCAN(algorithm='brute') on the host {host:.2f} s; this fit {dev * 1e3:.1f} ms; adjusted Rand index "
        f"{adjusted_rand_score(sk.labels_, mine):.6f}, noise rows {int((sk.labels_ < 0).sum())} (sklearn) / {int((mine < 0).sum())} (this fit)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--rows", type=int, default=10000)
    ap.add_argument("--big-rows", type=int, default=70000)
    ap.add_argument("--host-n", type=int, default=3000)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "this benchmark measures the GPU; there is no CPU path"
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
    N = a.rows
    say(f"# HDBSCAN on one GPU ('{torch.cuda.get_device_name(0)}')")
    flat = one_round(N, 2, a.repeats, say)
    X = one_round(N, 12288, a.repeats, say)
    say("## rounds: the whole tree, euclidean, from core distances already computed")
    rounds_needed(X, f"ten blobs [{N}, 12288]", say)
    rounds_needed(flat, f"ten blobs [{N}, 2]", say)
    chain = _chain(N)
    order = torch.randperm(N, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    rounds_needed(chain[order].contiguous(), f"chain of {N} points, shuffled", say)
    say(f"## whole fit: HDBSCAN(min_cluster_size=50, min_samples={MIN_SAMPLES}).fit: neighbour search, rounds, the host reads, the host tree, "
        f"labels back on the device; wall ms")
    fits(X, min(a.repeats, 5), say)
    fits(flat, min(a.repeats, 5), say)
    del X
    torch.cuda.empty_cache()
    if a.big_rows:
        fits(_blobs(a.big_rows, 2), 3, say)
    if a.host_n:
        host_part(say, a.host_n, 12288)


if __name__ == "__main__":
    main()
