"""Agglomerative clustering (csrc/agglomerative.hip, vit_som_amd/agglomerative.py) at the sizes users run, on one GPU.

    python tools/agglomerative_bench.py [--out FILE] [--repeats 7] [--rows 1600 10000] [--host-n 3000] [--no-model]

distance pass: ops.agglo_distances at (N, 12 288) per metric, device events around each call, the arms alternated after one
warm-up round.  Its work is counted from the shape: the upper-triangle 64 x 64 tiles it computes, D columns each, and per
pair and column the fp64 vector instructions of the metric (euclidean: a subtraction and an FMA; manhattan: a subtraction
and an addition; cosine: one FMA, and the two norms' FMAs shared by four pairs), set against the fp64 vector rate (78.6 TF
= 39.3 T instructions/s, an FMA counted as two FLOP).
merge loop: ops.agglo_merge per linkage on a copy of the matrix (the loop overwrites it; the copy is not timed), device events
around the one call that enqueues all N - 1 steps; per-step time, the share of steps that searched a slot other than the merged
one again, and how many slots they searched.  At N = 1 600 also under the 40 x 40 grid's connectivity.
model (skipped with --no-model): evaluate_map_clusters on the flagship ViT-SOM (bench.py's c3 config) over a synthetic loader,
wall clock around calls that end in a device synchronise.
host, for scale: scipy's linkage on --host-n rows, one call each.
Everything is printed and written to --out."""
import argparse
import copy
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

D = 12288
FP64_INSTR = 39.3e12                                  # fp64 vector instructions per second at the 78.6 TF peak
INSTR = {"euclidean": 2.0, "manhattan": 2.0, "cosine": 1.5}
LINKAGES = ("ward", "average", "complete", "single")


def _row(say, name, t, unit="ms"):
    med = statistics.median(t)
    say(f"{name:34s} " + " ".join(f"{v:10.3f}" for v in t) + f"   median {med:10.3f}  min {min(t):10.3f}  max {max(t):10.3f}  "
        f"spread {(max(t) - min(t)) / med:.4f}  ({unit})")
    return med


def _rows(N):
    import torch
    g = torch.Generator(device="cuda").manual_seed(N)
    X = torch.randn(N, D, device="cuda", generator=g)
    X.add_(5.0 * torch.randn(D, device="cuda", generator=g))       # column means large against the spread, as latents have
    return X


def _timed(arms, repeats):
    import torch
    times = {name: [] for name in arms}
    for rep in range(repeats + 1):                                 # the first round warms every arm up
        for name, (prepare, fn) in arms.items():
            prepare()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if rep:
                times[name].append(e0.elapsed_time(e1))
    return times


def distance_pass(N, repeats, say):
    import torch
    from vit_som_amd import ops
    X = _rows(N)
    out = torch.empty(N, N, dtype=torch.float64, device="cuda")
    status = torch.zeros(2, dtype=torch.int32, device="cuda")
    code = {"euclidean": ops.AGGLO_EUCLIDEAN, "manhattan": ops.AGGLO_MANHATTAN, "cosine": ops.AGGLO_COSINE}
    arms = {m: ((lambda: None), (lambda m=m: ops.agglo_distances(X, code[m], m == "euclidean", out, status))) for m in code}
    times = _timed(arms, repeats)
    tiles = (N + 63) // 64
    pairs = tiles * (tiles + 1) // 2 * 64 * 64
    say(f"## distance pass: X f32 [{N}, {D}], out fp64 [{N}, {N}] ({N * N * 8 / 2 ** 20:.0f} MiB); {tiles * (tiles + 1) // 2} tiles of 64 x 64 pairs; "
        f"ms per call (device events), {repeats} repeats after one warm-up round, alternated")
    for m in code:
        med = _row(say, f"vsom_agglo_distances {m}", times[m])
        rate = pairs * D * INSTR[m] / (med * 1e-3)
        say(f"{'':34s} {pairs * D / (med * 1e-3) / 1e12:.3f} T (pair, column) terms/s; {INSTR[m]} fp64 instructions per term -> "
            f"{rate / 1e12:.2f} T instructions/s = {rate / FP64_INSTR:.3f} of the fp64 vector rate")
    return X, out


def merge_loop(N, X, M0, repeats, say, grid=None):
    import torch
    from vit_som_amd import ops
    status2 = torch.zeros(2, dtype=torch.int32, device="cuda")
    children = torch.empty(N - 1, 2, dtype=torch.int32, device="cuda")
    heights = torch.empty(N - 1, dtype=torch.float64, device="cuda")
    status = torch.zeros(ops.AGGLO_STATUS, dtype=torch.int32, device="cuda")
    code = {"ward": ops.AGGLO_WARD, "average": ops.AGGLO_AVERAGE, "complete": ops.AGGLO_COMPLETE, "single": ops.AGGLO_SINGLE}
    saved = {False: M0.clone()}                                    # euclidean; Ward takes the squared one
    ops.agglo_distances(X, ops.AGGLO_EUCLIDEAN, True, M0, status2)
    saved[True] = M0.clone()
    adj = None
    if grid is not None:
        r = torch.arange(grid[0] * grid[1], device="cuda")
        dy, dx = (r[:, None] // grid[1] - r[None, :] // grid[1]).abs(), (r[:, None] % grid[1] - r[None, :] % grid[1]).abs()
        adj = ((dy <= 1) & (dx <= 1) & (r[:, None] != r[None, :])).to(torch.uint8)
    ws = torch.empty(ops.agglo_workspace_bytes(N, adj is not None), dtype=torch.uint8, device="cuda")

    def prepare(link):
        ops.agglo_matrix(ws, N).copy_(saved[link == "ward"])
        if adj is not None:
            ops.agglo_adjacency(ws, N).copy_(adj)
    arms = {link: ((lambda link=link: prepare(link)),
                   (lambda link=link: ops.agglo_merge(ws, N, code[link], adj is not None, children, heights, status)))
            for link in LINKAGES}
    t0 = time.perf_counter()
    times = _timed(arms, repeats)
    say(f"## merge loop: N {N}{'' if grid is None else f', connectivity of the {grid[0]} x {grid[1]} grid (8 neighbours)'}; euclidean distances "
        f"of the rows above; ms per call of vsom_agglo_merge ({3 * (N - 1) + 2} launches, device events), {repeats} repeats after one "
        f"warm-up round, alternated; workspace {ws.numel() / 2 ** 20:.0f} MiB")
    for link in LINKAGES:
        med = _row(say, f"vsom_agglo_merge {link}", times[link])
        prepare(link)
        ops.agglo_merge(ws, N, code[link], adj is not None, children, heights, status)
        st = status.cpu().tolist()
        say(f"{'':34s} {med / (N - 1) * 1e3:.2f} us per step; {st[2]} of {N - 1} steps ({st[2] / (N - 1):.3f}) searched slots other than the "
            f"merged one again, {st[1]} slots in all ({st[1] / max(st[2], 1):.1f} per such step, {st[1] / (N - 1):.2f} per step); "
            f"steps without a pair: {st[0]}")
    say(f"(this section took {time.perf_counter() - t0:.1f} s of wall time with its copies)")


def fits(X, repeats, say):
    import torch
    from vit_som_amd import AgglomerativeClustering
    N = X.shape[0]
    times, last = {"ward": [], "average": []}, {}
    for rep in range(repeats + 1):
        for link in times:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ac = AgglomerativeClustering(10, linkage=link).fit(X)
            torch.cuda.synchronize()
            if rep:
                times[link].append((time.perf_counter() - t0) * 1e3)
            same = last.get(link)
            if same is not None:
                assert same == (ac.children_.tobytes(), ac.distances_.tobytes()), "two fits differ"
            last[link] = (ac.children_.tobytes(), ac.distances_.tobytes())
    say(f"## whole fits: AgglomerativeClustering(10, linkage=...).fit(X [{N}, {D}]): workspace, distance pass, merge loop, the one copy, the "
        f"host cut; wall ms around calls that end in a device synchronise, {repeats} repeats after one warm-up call; every repeat "
        f"gave the same bits")
    for link in times:
        _row(say, f"fit {link}", times[link])


def model_part(say, repeats, n_images=10000):
    import torch
    import bench
    import vit_som_amd
    from vit_som_amd.evaluation import evaluate_clustering, evaluate_map_clusters
    from vit_som_amd.train import synthetic_loaders
    cfg = bench.c3_config(500)
    torch.manual_seed(0)
    m = vit_som_amd.ViTSOM(copy.deepcopy(cfg), device="cuda:0")
    m.eval()
    train, _, _ = synthetic_loaders(cfg, n_train=n_images, n_val=500, n_test=500)
    k = int(cfg["data"]["num_classes"]) or 10
    times = {"evaluate_map_clusters": [], "evaluate_clustering": []}
    for rep in range(repeats + 1):
        for name in times:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if name == "evaluate_map_clusters":
                r = evaluate_map_clusters(m, cfg, train, n_clusters=k)
            else:
                evaluate_clustering(m, cfg, train)
            torch.cuda.synchronize()
            if rep:
                times[name].append((time.perf_counter() - t0) * 1e3)
    say(f"## model: flagship ViT-SOM (bench.py c3: 40 x 40 cosine map on 12 288-wide latents, untrained encoder), {r.n_samples} synthetic "
        f"images in batches of 500; evaluate_map_clusters(n_clusters={k}) = Ward on the unit-length prototypes under the grid's "
        f"connectivity + the loader pass; evaluate_clustering = the loader pass alone; wall ms, {repeats} repeats after one warm-up")
    for name in times:
        _row(say, name, times[name])
    say(f"units per cluster {r.units_per_cluster.tolist()}")


def host_part(say, n):
    import numpy as np
    import torch
    from scipy.cluster.hierarchy import linkage
    from vit_som_amd import AgglomerativeClustering
    X = _rows(n)
    Xh = X.cpu().numpy().astype(np.float64)
    say(f"## for scale: N {n}, D {D}, euclidean, one call each, wall ({os.cpu_count()} CPUs visible)")
    for link in ("ward", "average"):
        t0 = time.perf_counter()
        Z = linkage(Xh, link)
        host = time.perf_counter() - t0
        AgglomerativeClustering(10, linkage=link).fit(X)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ac = AgglomerativeClustering(10, linkage=link).fit(X)
        torch.cuda.synchronize()
        dev = time.perf_counter() - t0
        same = bool((ac.children_ == Z[:, :2].astype(np.int64)).all())
        say(f"{link:8s} scipy.cluster.hierarchy.linkage on the host {host:.2f} s; this fit {dev * 1e3:.1f} ms; the same children: {same}; "
            f"largest relative height difference {float(np.abs(ac.distances_ - Z[:, 2]).max() / Z[-1, 2]):.2e}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--rows", type=int, nargs="+", default=[1600, 10000])
    ap.add_argument("--host-n", type=int, default=3000)
    ap.add_argument("--no-model", action="store_true")
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
    say(f"# agglomerative clustering on one GPU ('{torch.cuda.get_device_name(0)}'); D {D}")
    for N in a.rows:
        X, M = distance_pass(N, a.repeats, say)
        from vit_som_amd import ops
        ops.agglo_distances(X, ops.AGGLO_EUCLIDEAN, False, M, torch.zeros(2, dtype=torch.int32, device="cuda"))
        merge_loop(N, X, M, a.repeats, say)
        if N == 1600:
            ops.agglo_distances(X, ops.AGGLO_EUCLIDEAN, False, M, torch.zeros(2, dtype=torch.int32, device="cuda"))
            merge_loop(N, X, M, a.repeats, say, grid=(40, 40))
        del M
        fits(X, min(a.repeats, 5), say)
        del X
        torch.cuda.empty_cache()
    if not a.no_model:
        model_part(say, min(a.repeats, 5))
    if a.host_n:
        host_part(say, a.host_n)


if __name__ == "__main__":
    main()
