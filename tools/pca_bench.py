"""Timing of the on-device PCA at the evaluation shape (profiles/r15_pca.txt).

    python tools/pca_bench.py [--out profiles/r15_pca.txt] [--repeats 7] [--host-n 10000]

kernels: every entry of csrc/pca.hip at N = 10 000 rows, D = 12 288, basis widths l = 10 (n_components = 2: the map picture
and the linear initialisation) and l = 72 (n_components = 64: the latent spectrum), alternated in one process, one warm-up
round, device events around each call; reported per call and, for the two contractions, against the two bounds computed
from the shape: the bytes of X over the 6 TB/s copy rate and 2 N D l FLOP over the 157.3 TF f32 matrix-core peak (the
contraction computes whole 128 x 64 tiles, so the FLOP actually issued are those of l rounded up to the tile).
one pass: project + backproject + gram (steps 3 of pca.py); fit: PCA.fit with its default ten passes, wall clock around a
call that ends in a device synchronise (every pass copies two [l, l] matrices to the host and waits for them); transform
and inverse_transform likewise.
for scale: sklearn.decomposition.PCA(svd_solver="randomized") on the host at --host-n rows of the same data (one call,
wall; the copy of the rows to the host not counted), and the two spectra side by side.
Everything is printed and written to --out."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_F32_TF = 157.3
COPY_TBS = 6.0
N, D = 10000, 12288
WIDTHS = (10, 72)


def _row(say, name, t, unit="ms"):
    med = statistics.median(t)
    say(f"{name:34s} " + " ".join(f"{v:9.3f}" for v in t) + f"   median {med:9.3f}  min {min(t):9.3f}  max {max(t):9.3f}  "
        f"spread {(max(t) - min(t)) / med:.4f}  ({unit})")
    return med


def data():
    import torch
    g = torch.Generator(device="cuda").manual_seed(0)
    X = (torch.randn(N, 64, device="cuda", generator=g) * (0.85 ** torch.arange(64, device="cuda"))) @ torch.randn(64, D, device="cuda", generator=g)
    X.add_(0.05 * torch.randn(N, D, device="cuda", generator=g))
    X.add_(5.0 * torch.randn(D, device="cuda", generator=g))                            # a column mean large against the spread
    return X


def kernels(X, repeats, say):
    import torch
    from vit_som_amd import ops
    mean, var = ops.pca_colstats(X)
    arms = {"vsom_pca_colstats": lambda: ops.pca_colstats(X, mean, var)}
    for l in WIDTHS:
        g = torch.Generator(device="cuda").manual_seed(l)
        B = torch.randn(l, D, device="cuda", generator=g) / D ** 0.5
        Ybuf = torch.empty(N, (l + 3) // 4 * 4, device="cuda")
        Y, Zt, out = Ybuf[:, :l], torch.empty(l, D, device="cuda"), torch.empty(l, D, device="cuda")
        GH = torch.empty(2, l, l, dtype=torch.float64, device="cuda")
        T = torch.randn(l, l, dtype=torch.float64, device="cuda", generator=g)
        rec = torch.empty(1600, D, device="cuda")
        ops.pca_project(X, mean, B, None, Y)
        ops.pca_backproject(Y, X, mean, Zt)
        arms[f"vsom_pca_project l={l}"] = lambda B=B, Y=Y: ops.pca_project(X, mean, B, None, Y)
        arms[f"vsom_pca_backproject l={l}"] = lambda Y=Y, Zt=Zt: ops.pca_backproject(Y, X, mean, Zt)
        arms[f"vsom_pca_gram l={l}"] = lambda B=B, Zt=Zt, GH=GH: ops.pca_gram(Zt, GH[0], B, GH[1])
        arms[f"vsom_pca_rotate l={l}"] = lambda T=T, Zt=Zt, out=out: ops.pca_rotate(T, Zt, out)
        arms[f"vsom_pca_reconstruct l={l} M=1600"] = lambda Y=Y, B=B, rec=rec: ops.pca_reconstruct(Y[:1600], None, B, mean, rec)
        arms[f"one pass l={l}"] = lambda B=B, Y=Y, Zt=Zt, GH=GH: (ops.pca_project(X, mean, B, None, Y), ops.pca_backproject(Y, X, mean, Zt),
                                                                  ops.pca_gram(Zt, GH[0], B, GH[1]))
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
    say(f"## kernels: N {N}, D {D}; ms per call (device events), {repeats} repeats after one warm-up round, alternated")
    x_ms = N * D * 4 / (COPY_TBS * 1e12) * 1e3
    for name in arms:
        med = _row(say, name, times[name])
        if "project" in name:
            l = int(name.split("l=")[1])
            flop_ms = 2.0 * N * D * l / (PEAK_F32_TF * 1e12) * 1e3
            say(f"{'':34s} bounds from the shape: X once at {COPY_TBS} TB/s {x_ms:.3f} ms, 2 N D l FLOP at {PEAK_F32_TF} TF {flop_ms:.3f} ms "
                f"-> {max(x_ms, flop_ms) / med:.3f} of the larger bound; {N * D * 4 / (med * 1e-3) / 1e12:.2f} TB/s of X")
        elif name == "vsom_pca_colstats":
            say(f"{'':34s} X twice at {COPY_TBS} TB/s {2 * x_ms:.3f} ms -> {2 * x_ms / med:.3f} of that bound")


def solver(X, repeats, host_n, say):
    import numpy as np
    import torch
    from vit_som_amd import PCA
    say(f"## the solver: wall ms around calls that end in a device synchronise, {repeats} repeats after one warm-up call")
    fitted = {}
    for k in (2, 64):
        times = {"fit": [], "transform": [], "inverse_transform": []}
        for rep in range(repeats + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            p = PCA(n_components=k).fit(X)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            Y = p.transform(X)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            p.inverse_transform(Y[:1600])
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            if rep:
                for key, v in zip(times, (t1 - t0, t2 - t1, t3 - t2)):
                    times[key].append(v * 1e3)
        for key, t in times.items():
            _row(say, f"n_components={k} {key}" + (" (1600 rows)" if key == "inverse_transform" else ""), t)
        say(f"{'':34s} residuals: max {float(p.residuals_.max()):.2e}; PC1+PC2 {float(p.explained_variance_ratio_[:2].sum()):.4f} of the variance")
        fitted[k] = p
    if host_n > 0:
        from sklearn.decomposition import PCA as SkPCA
        Xh = X[:host_n].cpu().numpy()
        t0 = time.perf_counter()
        sk = SkPCA(n_components=64, svd_solver="randomized", random_state=0).fit(Xh)
        host = time.perf_counter() - t0
        p = fitted[64] if host_n >= N else PCA(n_components=64).fit(X[:host_n].contiguous())
        ev = p.explained_variance_.cpu().numpy()
        say(f"## for scale: sklearn PCA(n_components=64, svd_solver='randomized') on the host at N {min(host_n, N)}, D {D} (one call, wall; "
            f"the copy of the rows to the host not counted): {host:.3f} s; largest |eigenvalue difference| / lambda_1 against the "
            f"device fit: {float(np.max(np.abs(ev - sk.explained_variance_)) / sk.explained_variance_[0]):.2e} (the randomized solver's "
            f"own error included)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_pca.txt"))
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--host-n", type=int, default=N)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("pca_bench: no GPU; a timing taken anywhere else says nothing")
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)
    X = data()
    kernels(X, a.repeats, say)
    solver(X, a.repeats, a.host_n, say)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
