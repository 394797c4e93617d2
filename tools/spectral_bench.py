"""Spectral embedding (csrc/spectral.hip, vit_som_amd/spectral.py) at the sizes users run, on one GPU.

    python tools/spectral_bench.py [--out FILE] [--repeats 7] [--rows 10000 70000] [--host-n 3000]

product: ops.spectral_spmm at l = 10 and 32 on the kNN graph (k = 15) of N blob rows, against the bytes it must move --
indptr, indices and data once, s and the rows of Y1 once each (the gathers beyond that are re-reads that caches can serve),
Y0 and the output once -- with the rate of a device copy of a buffer of that many bytes measured in the same run, alternated.
pass and fit: one filter pass of degree 20 (20 products), and SpectralEmbedding(2).fit on the precomputed graph (the solver
alone) and from the rows (search and host assembly included), wall clock around calls that end in a device synchronise.
UMAP's init: umap.spectral_init with the host path (ARPACK) against the device path on the same fuzzy graph, alternated
in one process, when the graph is connected.
host, for scale: sklearn.manifold.SpectralEmbedding on --host-n rows, one call, never beyond that size.
Everything is printed and written to --out, with what was not measured."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

K = 15


def _row(say, name, t, unit="ms"):
    med = statistics.median(t)
    say(f"{name:44s} " + " ".join(f"{v:9.3f}" for v in t) + f"   median {med:9.3f}  min {min(t):9.3f}  max {max(t):9.3f}  "
        f"spread {(max(t) - min(t)) / med:.4f}  ({unit})")
    return med


def _blobs(N, D=16, seed=0, k=10):
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed + N + D)
    centres = 2.0 * torch.randn(k, D, device="cuda", generator=g)
    which = torch.randint(0, k, (N,), device="cuda", generator=g)
    return (centres[which] + torch.randn(N, D, device="cuda", generator=g)).contiguous()


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


def _wall(fn, repeats):
    import torch
    out = []
    for rep in range(repeats + 1):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if rep:
            out.append(1e3 * (time.perf_counter() - t))
    return out


def product(graph, repeats, say):
    import torch
    N, nnz = graph.N, graph.indices.shape[0]
    say(f"## product: N {N}, nnz {nnz} ({nnz / N:.1f} a row, longest {int((graph.indptr[1:] - graph.indptr[:-1]).max())}, "
        f"{graph.n_heavy} rows past one chunk); ms per call (device events), {repeats} repeats after one warm-up round, alternated")
    for l in (10, 32):
        Y1, Y0, out = (torch.randn(N, l, dtype=torch.float64, device="cuda") for _ in range(3))
        need = 8 * (N + 1) + 16 * nnz + 8 * N + 3 * 8 * N * l                      # the CSR arrays, s, and Y1, Y0 and the output once each
        gathered = 8 * nnz * l                                                     # what the gathers ask for, served by caches or not
        src = torch.empty(need // 2, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)
        t = _timed({"spmm": lambda: graph.apply(Y1, Y0, 1.3, -0.5, 0.7, out), "copy": lambda: dst.copy_(src)}, repeats)
        a = _row(say, f"l {l:2d} vsom_spectral_spmm", t["spmm"])
        b = _row(say, f"l {l:2d} copy of {need / 2 ** 20:.1f} MiB (read + write)", t["copy"])
        say(f"    must move {need / 2 ** 20:.1f} MiB -> {need / a / 1e6:.1f} GB/s; the copy moves the same bytes at {need / b / 1e6:.1f} GB/s; "
            f"ratio of times {a / b:.2f}; the gathers ask for {gathered / 2 ** 20:.1f} MiB more, {(need + gathered) / a / 1e6:.1f} GB/s with them")


def solver(N, repeats, say):
    import torch
    from vit_som_amd import SpectralEmbedding
    from vit_som_amd import spectral as S
    X = _blobs(N)
    t0 = time.perf_counter()
    A = S.knn_affinity(X, K)
    torch.cuda.synchronize()
    say(f"## N {N}: kNN search and host assembly of the graph, one call: {1e3 * (time.perf_counter() - t0):.1f} ms")
    graph = S.DeviceGraph.from_scipy(A, X.device)
    product(graph, repeats, say)
    l = 2 + 1 + S.OVERSAMPLE
    V = torch.randn(N, l, dtype=torch.float64, device="cuda")
    bufs = [torch.empty_like(V) for _ in range(3)]
    say(f"## N {N}: filter pass and whole fits; ms (wall clock, ends in a synchronise), {repeats} repeats after one warm-up")
    _row(say, f"one filter pass, degree 20, l {l}", _wall(lambda: S.chebyshev_filter(graph.apply, V, bufs, l, 0.0, 20), repeats))
    fits = []
    import warnings
    with warnings.catch_warnings():
        warnings.filterwarnings("ignore", message=S.DISCONNECTED)
        _row(say, "SpectralEmbedding(2) precomputed: solver", _wall(lambda: fits.append(
            SpectralEmbedding(2, affinity="precomputed", random_state=0).fit(A)), repeats))
        _row(say, "SpectralEmbedding(2) from rows: all", _wall(lambda: SpectralEmbedding(2, n_neighbors=K, random_state=0).fit(X), repeats))
    se = fits[-1]
    say(f"    {se.n_iter_} passes, max residual {float(se.residuals_.max()):.2e}, {se.n_connected_components_} graph components")


def umap_init(N, repeats, say):
    import numpy as np
    import scipy.sparse.csgraph
    import torch
    from vit_som_amd import UMAP
    from vit_som_amd import umap as UM
    X = _blobs(N, k=1)
    G = UMAP(n_neighbors=K, random_state=0, n_epochs=1, init="random").fit(X).graph_
    comps = scipy.sparse.csgraph.connected_components(G, directed=False)[0]
    say(f"## UMAP init at N {N}: spectral_init on the fuzzy graph ({comps} components); ms (wall clock), alternated, {repeats} repeats")
    if comps != 1:
        say("    not measured: the graph is not connected, both inits take the host path")
        return
    host, dev = [], []
    for rep in range(repeats + 1):
        for out, device in ((host, None), (dev, X.device)):
            torch.cuda.synchronize()
            t = time.perf_counter()
            UM.spectral_init(G, 2, np.random.RandomState(0), None, device)
            torch.cuda.synchronize()
            if rep:
                out.append(1e3 * (time.perf_counter() - t))
    a = _row(say, "init='spectral' (ARPACK, host)", host)
    b = _row(say, "init='spectral_device'", dev)
    say(f"    host / device {a / b:.2f}")


def host_scale(N, say):
    import warnings
    import numpy as np
    from sklearn.manifold import SpectralEmbedding as Sk
    X = _blobs(N).cpu().numpy().astype(np.float64)
    t = time.perf_counter()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        Sk(2, affinity="nearest_neighbors", n_neighbors=K, random_state=0).fit(X)
    say(f"## host, for scale: sklearn.manifold.SpectralEmbedding(2, nearest_neighbors, k = {K}) at N {N}, one call: "
        f"{1e3 * (time.perf_counter() - t):.1f} ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--rows", type=int, nargs="+", default=[10000, 70000])
    ap.add_argument("--host-n", type=int, default=3000)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("spectral_bench.py measures on the GPU; there is none")
    if a.host_n > 3000:
        raise SystemExit("--host-n beyond 3000 is not timed: sklearn's solver takes minutes there")
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)
    say(f"# spectral_bench.py on {torch.cuda.get_device_name(0)}; rows {a.rows}, k {K}, {a.repeats} repeats")
    for N in a.rows:
        solver(N, a.repeats, say)
    for N in a.rows:
        umap_init(N, a.repeats, say)
    host_scale(a.host_n, say)
    say("## not measured: kernel times by profiler, counters, more than one GPU, N beyond the largest --rows, sklearn beyond "
        f"{a.host_n} rows, the 16-byte load path (there is none)")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
