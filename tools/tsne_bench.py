"""Timing of the on-device t-SNE at the sizes users run (profiles/r18_tsne.txt).

    python tools/tsne_bench.py [--out profiles/r18_tsne.txt] [--repeats 7] [--rows 10000 60000] [--no-sklearn]

kernels: the launches of a fit at N rows on their own -- vsom_tsne_repulsion, vsom_tsne_step without and with its record,
vsom_tsne_affinities, and for scale the neighbour search in front of it -- alternated in one process, one warm-up round,
device events around each single call.  The repulsion is given as pairs per second and as a share of the f32 vector rate:
its inner loop issues 10 vector instructions per pair (two subtractions, a multiply, three fused multiply-adds, two
additions, a multiply and a reciprocal), set against the 78.6 T lane-instructions per second behind the 157.3 TFLOPS of
the data sheet (a fused multiply-add counted as two there, as one here; the reciprocal issues at a quarter of the rate,
which this share does not credit).
end to end: TSNE().fit (1 000 iterations, the host graph, the search and the PCA init included) by wall clock around calls
that end in a device synchronise, and the share of it that lies outside the repulsion launches.
sklearn (skipped with --no-sklearn): TSNE(method='barnes_hut') on the host once at N = 3 000, for scale.
Everything is printed and written to --out."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LANE_INSTR_PER_S = 157.3e12 / 2
INSTR_PER_PAIR = 10
D = 64


def _row(say, name, t, unit="ms"):
    med = statistics.median(t)
    say(f"{name:34s} " + " ".join(f"{v:9.4f}" for v in t) + f"   median {med:9.4f}  min {min(t):9.4f}  max {max(t):9.4f}  "
        f"spread {(max(t) - min(t)) / med:.4f}  ({unit})")
    return med


def data(N, device="cuda"):
    """Ten blobs in D = 64 columns: centres 4 N(0, 1), unit noise."""
    import torch
    g = torch.Generator(device=device).manual_seed(0)
    centres = 4.0 * torch.randn(10, D, device=device, generator=g)
    lab = torch.randint(0, 10, (N,), device=device, generator=g)
    return (centres[lab] + torch.randn(N, D, device=device, generator=g)).contiguous()


def at_size(N, repeats, say):
    import torch
    from vit_som_amd import TSNE, ops
    from vit_som_amd.tsne import _Graph
    X = data(N)
    dev = X.device
    est = TSNE()
    k = est._validate(N)
    P = est.affinities(X, k)
    graph = _Graph(P, dev)
    g = torch.Generator(device=dev).manual_seed(1)
    Y = (10.0 * torch.randn(N, 2, device=dev, generator=g)).contiguous()
    Yout, upd, gains = torch.empty_like(Y), torch.zeros_like(Y), torch.ones_like(Y)
    idx = torch.empty(N, k + 1, dtype=torch.int64, device=dev)
    dist = torch.empty(N, k + 1, dtype=torch.float32, device=dev)
    ops.umap_knn(X, k + 1, ops.DIST_EUCLIDEAN, idx, dist)
    cond = torch.empty(N, k, dtype=torch.float64, device=dev)
    beta = torch.empty(N, dtype=torch.float64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    lr = max(N / 12.0 / 4.0, 50.0)
    arms = {"repulsion": lambda: ops.tsne_repulsion(Y, graph.rep, graph.sumq, graph.zpart),
            "step": lambda: ops.tsne_step(graph.indptr, graph.indices, graph.data, Y, Yout, upd, gains, graph.rep, graph.zpart, 1.0,
                                          0.8, lr, graph.part, record=False),
            "step with its record": lambda: ops.tsne_step(graph.indptr, graph.indices, graph.data, Y, Yout, upd, gains, graph.rep,
                                                          graph.zpart, 1.0, 0.8, lr, graph.part, record=True),
            "affinities": lambda: ops.tsne_affinities(dist, 30.0, cond, beta, status, knn_idx=idx),
            f"neighbour search (D = {D})": lambda: ops.umap_knn(X, k + 1, ops.DIST_EUCLIDEAN, idx, dist)}
    times = {name: [] for name in arms}
    for r in range(repeats + 1):                                                         # the first round warms every arm up
        for name, fn in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if r:
                times[name].append(e0.elapsed_time(e1))
    say(f"## kernels: N {N}, k {k}, {P.nnz} edges in the joint P; ms per call (device events), {repeats} repeats after one warm-up "
        f"round, alternated")
    med = {name: _row(say, name, times[name]) for name in arms}
    pairs = N * (N - 1)
    rate = pairs / (med["repulsion"] * 1e-3)
    say(f"repulsion: {pairs:.3e} pairs in {med['repulsion'] * 1e3:.1f} us = {rate:.3e} pairs/s = {INSTR_PER_PAIR} x that = "
        f"{100 * rate * INSTR_PER_PAIR / LANE_INSTR_PER_S:.1f} % of the f32 vector instruction rate ({LANE_INSTR_PER_S:.3e} lane-instructions/s); "
        f"{(N + 63) // 64} workgroups of 1024 threads on 256 CUs")
    say(f"one iteration, sum of the medians: {(med['repulsion'] + med['step']) * 1e3:.1f} us (repulsion + step), "
        f"{(med['repulsion'] + med['step with its record']) * 1e3:.1f} us with the record")
    wall, its, kls = [], [], []
    for r in range(repeats + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fit = TSNE(random_state=0).fit(X)
        torch.cuda.synchronize()
        if r:
            wall.append((time.perf_counter() - t0) * 1e3)
            its.append(fit.n_iter_ + 1)
            kls.append(fit.kl_divergence_)
    say(f"## end to end: TSNE(random_state=0).fit(X [{N}, {D}]) (perplexity 30, 1 000 iterations at most); wall ms, {repeats} repeats "
        f"after one warm-up fit")
    w = _row(say, "fit", wall)
    in_rep = its[0] * med["repulsion"]
    t0 = time.perf_counter()
    est.affinities(X, k)
    torch.cuda.synchronize()
    aff = (time.perf_counter() - t0) * 1e3
    say(f"that fit: {its[0]} iterations ({'the same' if len(set(its)) == 1 else 'NOT the same'} in every repeat), KL {kls[0]:.4f} "
        f"({'the same bits' if len(set(kls)) == 1 else 'NOT the same'} in every repeat); {w / its[0] * 1e3:.1f} us per iteration all in; "
        f"{its[0]} repulsion launches at their median = {in_rep:.1f} ms: {100 * (w - in_rep) / w:.1f} % of the fit lies outside the "
        f"repulsion; search, affinities and host graph (steps 1-3, one call, wall) {aff:.1f} ms")


def sklearn_once(say):
    import numpy as np
    import torch
    from sklearn.manifold import TSNE as SkTSNE
    from sklearn.manifold import trustworthiness
    from vit_som_amd import TSNE
    import vit_som_amd
    X = data(3000)
    Xh = X.cpu().numpy()
    t0 = time.perf_counter()
    sk = SkTSNE(method="barnes_hut", random_state=0)
    Eh = sk.fit_transform(Xh)
    host = time.perf_counter() - t0
    TSNE(random_state=0).fit(X)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ours = TSNE(random_state=0).fit(X)
    torch.cuda.synchronize()
    dev = time.perf_counter() - t0
    rows = np.arange(0, 3000, 2)
    t_sk = trustworthiness(Xh[rows], Eh[rows], n_neighbors=15)
    t_us = vit_som_amd.trustworthiness(X, ours.embedding_.contiguous(), n_neighbors=15)
    say(f"## for scale: N 3000, D {D}, one call each, wall: sklearn TSNE(method='barnes_hut') on the host ({os.cpu_count()} CPUs visible) "
        f"{host:.2f} s, KL {sk.kl_divergence_:.4f}, trustworthiness (k = 15, every second row) {t_sk:.4f}; this fit {dev * 1e3:.1f} ms, "
        f"KL {ours.kl_divergence_:.4f}, trustworthiness (k = 15, all rows) {t_us:.4f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18_tsne.txt"))
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--rows", type=int, nargs="+", default=[10000, 60000])
    ap.add_argument("--no-sklearn", action="store_true")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tsne_bench: no GPU; a timing taken anywhere else says nothing")
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    arch = getattr(torch.cuda.get_device_properties(0), "gcnArchName", "?").split(":")[0]
    say(f"# t-SNE on one MI355X ({arch}; torch reports the device name {torch.cuda.get_device_name(0)!r}): "
        f"tools/tsne_bench.py --repeats {a.repeats}")
    for N in a.rows:
        at_size(N, a.repeats, say)
    if not a.no_sklearn:
        sklearn_once(say)
    say("## the chain of an iteration is two launches (repulsion, step); a third launch was not tried, so there is no A/B of "
        "it here.")
    say("## not measured: kernel times from a profiler trace and counters (the figures above are device events around one "
        "call, launch overhead included: at N = 10 000 that overhead is not small against the kernel); the in-kernel clock; "
        "more than one GPU; N beyond 60 000; real latents (the rows are synthetic blobs); cosine; a fit under a launch tape.")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
