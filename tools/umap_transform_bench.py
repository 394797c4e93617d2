"""UMAP.transform timed on the device: the one-launch layout (vsom_umap_transform_layout) alone, and transform() end to
end split into search (vsom_knn_query), host graph (transform_graph, with the copies of the kNN table) and layout, for M
new rows placed into a fit of N rows; for scale the fit's own layout (n_epochs launches of vsom_umap_epoch) from the same
process.

    python tools/umap_transform_bench.py [--train 10000] [--dim 12288] [--new 1600,10000,40000] [--k 15] [--reps 5] [--out FILE]

Data: a rank-32 signal plus noise (clustered, like real latents), new rows from the same distribution.  Device phases
by device events, host phases by a host clock after a synchronise; every phase is warmed once and repeated --reps times:
min / median / max in milliseconds.  One JSON line per M."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _data(N, D, seed):
    g = torch.Generator(device="cuda").manual_seed(1)
    basis = torch.randn(32, D, device="cuda", generator=g)
    g = torch.Generator(device="cuda").manual_seed(seed)
    X = torch.randn(N, 32, device="cuda", generator=g) @ basis
    return X.add_(0.1 * torch.randn(N, D, device="cuda", generator=g)).contiguous()


def _stats(ms):
    return {"min": round(min(ms), 3), "median": round(float(np.median(ms)), 3), "max": round(max(ms), 3)}


def _device_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return _stats(out)


def _host_ms(fn, reps):
    fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return _stats(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--train", type=int, default=10000)
    ap.add_argument("--dim", type=int, default=12288)
    ap.add_argument("--new", default="1600,10000,40000")
    ap.add_argument("--k", type=int, default=15)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from vit_som_amd import UMAP, ops, umap as U
    lines = []

    def emit(res):
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)

    Xtr = _data(a.train, a.dim, seed=2)
    m = UMAP(n_neighbors=a.k, min_dist=0.1, metric="cosine", random_state=42)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    m.fit(Xtr)
    torch.cuda.synchronize()
    fit_s = time.perf_counter() - t0

    # the fit's layout: n_epochs launches over the pruned graph, as fit() issues them
    P, eps, eps_neg = U.make_schedule(m.graph_, m._n_epochs, m.negative_sample_rate)
    dev_t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()                      # noqa: E731
    indptr, indices, eps_d, eps_neg_d = dev_t(P.indptr.astype(np.int64)), dev_t(P.indices.astype(np.int64)), dev_t(eps), dev_t(eps_neg)

    def fit_layout():
        nxt, nxt_neg = eps_d.clone(), eps_neg_d.clone()
        Y = [m.embedding_.clone(), torch.empty_like(m.embedding_)]
        for n in range(m._n_epochs):
            alpha = 1.0 if n == 0 else 1.0 - (n - 1) / float(m._n_epochs)
            ops.umap_epoch(indptr, indices, eps_d, nxt, eps_neg_d, nxt_neg, Y[0], Y[1], m._a, m._b, 1.0, alpha, n, m._layout_seed)
            Y.reverse()
    emit({"fit": {"N": a.train, "D": a.dim, "k": a.k, "n_epochs": m._n_epochs, "edges": int(P.nnz), "fit_s": round(fit_s, 2),
                  "layout_ms": _device_ms(fit_layout, a.reps)}})

    for M in (int(v) for v in a.new.split(",")):
        X = _data(M, a.dim, seed=3)
        n_epochs = U.transform_n_epochs(None, M)
        idx = torch.empty(M, a.k, dtype=torch.int64, device="cuda")
        dist = torch.empty(M, a.k, dtype=torch.float32, device="cuda")
        search = _device_ms(lambda: ops.knn_query(X, Xtr, a.k, U.METRICS["cosine"], idx, dist), a.reps)
        host = {}

        def graph():
            host["w"], host["eps"] = U.transform_graph(idx.cpu().numpy(), dist.cpu().numpy(), 1.0, n_epochs)
            host["wd"], host["epsd"] = torch.from_numpy(host["w"]).cuda(), torch.from_numpy(host["eps"]).cuda()
        graph_ms = _host_ms(graph, a.reps)
        Y = torch.empty(M, 2, dtype=torch.float32, device="cuda")
        status = torch.zeros(1, dtype=torch.int32, device="cuda")
        ws = ops.umap_transform_workspace(M, a.k, "cuda")
        layout = _device_ms(lambda: ops.umap_transform_layout(idx, host["wd"], host["epsd"], m.embedding_, Y, m._a, m._b, 1.0, 0.25,
                                                              n_epochs, 0, n_epochs, 5, m._layout_seed, status, ws), a.reps)
        finite = np.isfinite(host["eps"])
        samples = float((n_epochs / host["eps"][finite]).sum())             # attractions, about; 5 repulsions follow each
        whole = _host_ms(lambda: m.transform(X), a.reps)
        assert int(status.item()) == 0 and bool(torch.isfinite(Y).all())
        emit({"M": M, "N": a.train, "D": a.dim, "k": a.k, "n_epochs": n_epochs, "live_edges": int(finite.sum()),
              "attractions_about": int(samples), "search_ms": search, "host_graph_ms": graph_ms, "layout_ms": layout,
              "transform_ms": whole, "layout_over_search": round(layout["median"] / search["median"], 3)})
        del X, idx, dist, Y, ws
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
