"""DBSCAN (csrc/knn.hip's DBSCAN section, vit_som_amd/dbscan.py) at the sizes users run, on one GPU.

    python tools/dbscan_bench.py [--out FILE] [--repeats 7] [--rows 10000] [--host-n 3000]

neighbours pass: ops.dbscan_neighbours against ops.knn_ranks at k = 15 -- the same contraction with a heavier epilogue, the
yardstick -- at (N, 12 288) and (N, 2), both metrics, both entries timed in the same process, alternated after one warm-up
round, device events around single calls.  Pairs per second are counted from the shape (N^2 pairs, 2 D FLOP each).
components: ops.dbscan_init + the ops.dbscan_round calls until one moves nothing + ops.dbscan_finish, wall clock around the
loop (it ends in a host read per call), on a blob set and on a chain of N points at unit spacing in shuffled order; the
number of round calls is printed.
whole fit: DBSCAN(eps, min_samples=5).fit on the blob set, wall clock around calls that end in a device synchronise.
host, for scale: sklearn.cluster.DBSCAN on --host-n rows, one call.
Everything is printed and written to --out."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

K_RANKS = 15


def _row(say, name, t, unit="ms"):
    med = statistics.median(t)
    say(f"{name:40s} " + " ".join(f"{v:9.3f}" for v in t) + f"   median {med:9.3f}  min {min(t):9.3f}  max {max(t):9.3f}  "
        f"spread {(max(t) - min(t)) / med:.4f}  ({unit})")
    return med


def _blobs(N, D, seed=0, k=10):
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed + N + D)
    centres = 3.0 * torch.randn(k, D, device="cuda", generator=g)
    which = torch.randint(0, k, (N,), device="cuda", generator=g)
    X = centres[which] + torch.randn(N, D, device="cuda", generator=g)
    far = torch.rand(N, device="cuda", generator=g) < 0.05          # one row in twenty is an outlier, three times as far out
    X[far] = centres[which[far]] + 3.0 * torch.randn(int(far.sum()), D, device="cuda", generator=g)
    return X.contiguous()


def _timed(arms, repeats):
    import torch
    times = {name: [] for name in arms}
    for rep in range(repeats + 1):                                 # the first round warms every arm up
        for name, fn in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if rep:
                times[name].append(e0.elapsed_time(e1))
    return times


def neighbours_pass(N, D, repeats, say):
    import torch
    from vit_som_amd import k_distances, ops
    X = _blobs(N, D)
    new = lambda dtype, *shape: torch.empty(*shape, dtype=dtype, device="cuda")      # noqa: E731
    sq, adj, count, status = new(torch.float32, N), new(torch.int64, N, ops.dbscan_words(N)), new(torch.int32, N), new(torch.int64, 2)
    idx, dist = new(torch.int64, N, K_RANKS + 1), new(torch.float32, N, K_RANKS + 1)
    less, tied = new(torch.int32, N, K_RANKS), new(torch.int32, N, K_RANKS)
    say(f"## neighbours pass: X f32 [{N}, {D}], adj {N * ops.dbscan_words(N) * 8 / 2 ** 20:.1f} MiB of bits; vsom_dbscan_neighbours against "
        f"vsom_knn_ranks at k = {K_RANKS}; ms per call (device events), {repeats} repeats after one warm-up round, alternated")
    for name, metric in (("euclidean", ops.DIST_EUCLIDEAN), ("cosine", ops.DIST_COSINE)):
        eps = float(k_distances(X, 4, name)[N // 2])
        ops.umap_knn(X, K_RANKS + 1, metric, idx, dist)
        nbr = idx[:, 1:].contiguous()
        arms = {"neighbours": lambda: ops.dbscan_neighbours(X, metric, eps, sq, adj, count, status),
                "ranks": lambda: ops.knn_ranks(X, nbr, metric, less, tied)}
        times = _timed(arms, repeats)
        a = _row(say, f"vsom_dbscan_neighbours {name}", times["neighbours"])
        b = _row(say, f"vsom_knn_ranks {name}", times["ranks"])
        spread = max((max(t) - min(t)) / statistics.median(t) for t in times.values())
        st = status.tolist()
        say(f"{'':40s} neighbours / ranks = {a / b:.3f} (the larger spread {spread:.3f}); {N * N / (a * 1e-3) / 1e9:.2f} G pairs/s, "
            f"{2.0 * N * N * D / (a * 1e-3) / 1e12:.1f} TF; eps {eps:.6g}: {st[1]} set bits ({st[1] / N:.1f} per row), {st[0]} bad rows")
    return X


def _chain(N):
    """A chain of N points at unit spacing, every point within 1 of its two neighbours in the chain and of nobody else:
    folded into a strip 100 wide (rows 2 apart, one connecting point between two rows), because a straight chain of 10 000
    unit steps has squared norms of 1e8, which fp32 does not hold exactly -- the expansion |x|^2 + |y|^2 - 2 x.y then
    misplaces pairs (the offset-heavy case DBSCAN's docstring sends to metric='precomputed')."""
    import torch
    pts, r = [], 0
    while len(pts) < N:
        xs = range(100) if r % 2 == 0 else range(99, -1, -1)
        pts += [(x, 2 * r, 0) for x in xs]
        pts.append((99 if r % 2 == 0 else 0, 2 * r + 1, 0))
        r += 1
    return torch.tensor(pts[:N], dtype=torch.float32, device="cuda")


def components(X, eps, metric, what, repeats, say, min_samples=5):
    import torch
    from vit_som_amd import ops
    from vit_som_amd.dbscan import ROUNDS_PER_CALL
    N = X.shape[0]
    new = lambda dtype, *shape: torch.empty(*shape, dtype=dtype, device="cuda")      # noqa: E731
    sq, adj, count, status = new(torch.float32, N), new(torch.int64, N, ops.dbscan_words(N)), new(torch.int32, N), new(torch.int64, 2)
    core, root, changed = new(torch.uint8, N), new(torch.int32, N), new(torch.int32, 1)
    labels, record = new(torch.int64, N), new(torch.int32, 4)
    ops.dbscan_neighbours(X, metric, eps, sq, adj, count, status)
    times, calls = [], 0
    for rep in range(repeats + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ops.dbscan_init(count, min_samples, core, root)
        calls = 0
        while True:
            ops.dbscan_round(adj, core, root, ROUNDS_PER_CALL, changed)
            calls += 1
            if not int(changed.item()):
                break
        ops.dbscan_finish(adj, core, root, labels, record)
        torch.cuda.synchronize()
        if rep:
            times.append((time.perf_counter() - t0) * 1e3)
    _row(say, f"components, {what}", times)
    say(f"{'':40s} {calls} vsom_dbscan_round calls of {ROUNDS_PER_CALL} rounds (the last one moves nothing); clusters / core / border / noise "
        f"{record.tolist()}; {int(status[1])} set bits")


def fits(X, eps, repeats, say):
    import torch
    from vit_som_amd import DBSCAN
    times, last = [], None
    for rep in range(repeats + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        db = DBSCAN(eps=eps, min_samples=5).fit(X)
        torch.cuda.synchronize()
        if rep:
            times.append((time.perf_counter() - t0) * 1e3)
        assert last is None or torch.equal(last, db.labels_), "two fits differ"
        last = db.labels_
    _row(say, f"DBSCAN.fit [{X.shape[0]}, {X.shape[1]}]", times)
    say(f"{'':40s} {db.n_clusters_} clusters, {db.n_noise_} noise rows, {db.n_round_calls_} round calls; every repeat gave the same labels")


def host_part(say, n, D):
    import numpy as np
    import torch
    from sklearn.cluster import DBSCAN as SK
    from vit_som_amd import DBSCAN, k_distances
    X = _blobs(n, D)
    eps = float(k_distances(X, 4)[n // 2])
    Xh = X.cpu().numpy().astype(np.float64)
    t0 = time.perf_counter()
    sk = SK(eps=eps, min_samples=5).fit(Xh)
    host = time.perf_counter() - t0
    DBSCAN(eps=eps, min_samples=5).fit(X)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    db = DBSCAN(eps=eps, min_samples=5).fit(X)
    torch.cuda.synchronize()
    dev = time.perf_counter() - t0
    differ = int((db.labels_.cpu().numpy() != sk.labels_).sum())
    say(f"## for scale: N {n}, D {D}, euclidean, one call each, wall ({os.cpu_count()} CPUs visible): sklearn.cluster.DBSCAN on the host "
        f"{host:.2f} s; this fit {dev * 1e3:.1f} ms; {differ} of {n} labels differ (eps is a distance the set attains in fp32, so the "
        f"pairs at eps fall on either side in fp64: no margin is promised here)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--rows", type=int, default=10000)
    ap.add_argument("--host-n", type=int, default=3000)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "this benchmark measures the GPU; there is no CPU path"
    from vit_som_amd import k_distances, ops
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
    N = a.rows
    say(f"# DBSCAN on one GPU ('{torch.cuda.get_device_name(0)}')")
    neighbours_pass(N, 2, a.repeats, say)
    X = neighbours_pass(N, 12288, a.repeats, say)
    eps = float(k_distances(X, 4)[N // 2])
    say(f"## components: ops.dbscan_init, the round calls to the fixed point, ops.dbscan_finish; min_samples 5; wall ms around the loop "
        f"(one host read per round call), {a.repeats} repeats after one warm-up")
    components(X, eps, ops.DIST_EUCLIDEAN, f"blobs [{N}, 12288]", a.repeats, say)
    chain = _chain(N)
    order = torch.randperm(N, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    components(chain[order].contiguous(), 1.0, ops.DIST_EUCLIDEAN, f"chain of {N} points, shuffled", a.repeats, say, min_samples=2)
    components(chain.flip(0).contiguous(), 1.0, ops.DIST_EUCLIDEAN, f"chain of {N} points, reversed", a.repeats, say, min_samples=2)
    components(chain, 1.0, ops.DIST_EUCLIDEAN, f"chain of {N} points, in order", a.repeats, say, min_samples=2)
    say(f"## whole fit: DBSCAN(eps={eps:.6g}, min_samples=5).fit: buffers, neighbours pass, components, labels, the host reads; wall ms")
    fits(X, eps, min(a.repeats, 5), say)
    del X
    torch.cuda.empty_cache()
    if a.host_n:
        host_part(say, a.host_n, 12288)


if __name__ == "__main__":
    main()
