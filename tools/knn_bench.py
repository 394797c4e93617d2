"""Timing of the kNN probe at the benchmark's evaluation shape (profiles/r11_knn.txt).

    python tools/knn_bench.py [--out profiles/r11_knn.txt] [--repeats 7] [--train 50000] [--test 10000] [--no-e2e]

kernels: vsom_knn_query (Nq = 10 000 queries, one bank buffer of Nb = 4096 rows, D = 12 288, k = 20, cosine) against
vsom_umap_knn (N = 10 000 among itself, same D and k) -- the existing kernel is the yardstick -- alternated in one
process, one warm-up round, device events around each call; reported per call, as (query, bank row) pairs per second and
as a share of the 157.3 TF f32 matrix-core peak (FLOP = 2 x pairs x D: the contraction; norms, top-k and merge add none).
end to end: evaluate_knn (bank = a training loader, queries = a test loader) next to evaluate_kmeans on the same test
loader, on a ViT-SOM of the benchmark architecture with random weights and resident synthetic CIFAR-shaped batches of 512,
alternated, wall clock around calls that end in a device synchronise.  Everything is printed and written to --out."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_F32_TF = 157.3
NQ, NB, D, K, N_UMAP, B = 10000, 4096, 12288, 20, 10000, 512


def _stats(t):
    med = statistics.median(t)
    return med, min(t), max(t), (max(t) - min(t)) / med


def kernels(repeats, say):
    import torch
    from vit_som_amd import ops
    g = torch.Generator(device="cuda").manual_seed(0)
    X = torch.randn(N_UMAP, 32, device="cuda", generator=g) @ torch.randn(32, D, device="cuda", generator=g)
    X.add_(0.1 * torch.randn(N_UMAP, D, device="cuda", generator=g))                    # clustered, like real latents
    Q, bank = X[:NQ], (torch.randn(NB, 32, device="cuda", generator=g) @ torch.randn(32, D, device="cuda", generator=g)).contiguous()
    qi, qd = torch.empty(NQ, K, dtype=torch.int64, device="cuda"), torch.empty(NQ, K, device="cuda")
    ui, ud = torch.empty(N_UMAP, K, dtype=torch.int64, device="cuda"), torch.empty(N_UMAP, K, device="cuda")
    arms = {"vsom_knn_query": (lambda: ops.knn_query(Q, bank, K, ops.DIST_COSINE, qi, qd), NQ * NB),
            "vsom_umap_knn": (lambda: ops.umap_knn(X, K, ops.DIST_COSINE, ui, ud), N_UMAP * N_UMAP)}
    times = {name: [] for name in arms}
    for rep in range(repeats + 1):                                                      # the first round warms both arms up
        for name, (fn, _) in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if rep:
                times[name].append(e0.elapsed_time(e1))
    say(f"## kernels: Nq {NQ}, Nb {NB}, D {D}, k {K}, cosine; vsom_umap_knn at N {N_UMAP}; ms per call (device events), "
        f"{repeats} repeats after one warm-up round, alternated")
    rate = {}
    for name, (_, pairs) in arms.items():
        med, lo, hi, spread = _stats(times[name])
        rate[name] = pairs / (med * 1e-3)
        tf = 2.0 * pairs * D / (med * 1e-3) / 1e12
        say(f"{name:16s} " + " ".join(f"{v:8.3f}" for v in times[name]) + f"   median {med:8.3f}  min {lo:8.3f}  max {hi:8.3f}  "
            f"spread {spread:.4f}")
        say(f"{'':16s} {pairs / 1e6:.2f} M pairs -> {rate[name] / 1e9:.3f} G pairs/s, {tf:.1f} TF = {100 * tf / PEAK_F32_TF:.1f} % of the "
            f"{PEAK_F32_TF} TF f32 matrix peak")
    say(f"pairs per second, vsom_knn_query / vsom_umap_knn: {rate['vsom_knn_query'] / rate['vsom_umap_knn']:.4f}")


def end_to_end(n_train, n_test, repeats, say):
    import torch
    import bench
    from vit_som_amd import ViTSOM
    from vit_som_amd.evaluation import evaluate_kmeans, evaluate_knn
    cfg = bench.c3_config(B)
    torch.manual_seed(0)
    model = ViTSOM(cfg, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(1)
    templates = torch.randn(10, 3, 32, 32, device="cuda", generator=g)

    def loader(n):
        out = []
        for i in range(0, n, B):
            y = torch.randint(0, 10, (min(B, n - i),), device="cuda", generator=g)
            out.append((templates[y] + 0.5 * torch.randn(len(y), 3, 32, 32, device="cuda", generator=g), y))
        return out
    train, test = loader(n_train), loader(n_test)
    acc = []
    arms = {"evaluate_knn": lambda: acc.append(evaluate_knn(model, cfg, train, test, num_labels=10).accuracy),
            "evaluate_kmeans": lambda: evaluate_kmeans(model, cfg, test)}
    times = {name: [] for name in arms}
    stdout, sys.stdout = sys.stdout, open(os.devnull, "w")                              # the evaluators print their own line
    try:
        for rep in range(repeats + 1):
            for name, fn in arms.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                if rep:
                    times[name].append(time.perf_counter() - t0)
    finally:
        sys.stdout = stdout
    say(f"## end to end: ViT-SOM of the benchmark architecture (random weights), resident batches of {B}; evaluate_knn: bank "
        f"{n_train} training samples, {n_test} test queries, k 20, softmax, cosine, bank_rows 4096; evaluate_kmeans on the same "
        f"{n_test} test samples; wall seconds, {repeats} repeats after one warm-up round, alternated")
    for name in arms:
        med, lo, hi, spread = _stats(times[name])
        say(f"{name:16s} " + " ".join(f"{v:8.3f}" for v in times[name]) + f"   median {med:8.3f}  min {lo:8.3f}  max {hi:8.3f}  "
            f"spread {spread:.4f}")
    say(f"kNN accuracy of the untrained encoder on the synthetic classes: {acc[-1]:.4f} (every repeat the same: {len(set(acc)) == 1})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11_knn.txt"))
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--train", type=int, default=50000)
    ap.add_argument("--test", type=int, default=10000)
    ap.add_argument("--no-e2e", action="store_true")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("knn_bench: no GPU; a timing taken anywhere else says nothing")
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)
    kernels(a.repeats, say)
    if not a.no_e2e:
        end_to_end(a.train, a.test, max(a.repeats // 2, 3), say)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
