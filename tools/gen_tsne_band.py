"""Generate tests/golden/tsne_fit_band.json: the band of final KL divergence and trustworthiness that the numpy restatement
of t-SNE (tests/tsne_ref.py, float32 state) itself spans on the whole-fit case of tests/test_tsne_gpu.py, over five runs
whose initial Y is perturbed by 1e-6 relative.  t-SNE's descent amplifies such a perturbation into a different local
optimum; the device fit is held to this band, not to coordinates.  Runs on the CPU (about two minutes):

    python tools/gen_tsne_band.py

The file holds the inputs by seed and shape and the results only."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import tsne_ref as R  # noqa: E402

CASE = dict(N=600, D=50, centres=6, data_seed=7, perplexity=30.0, max_iter=1000, n_neighbors=15, runs=5, perturbation=1e-6,
            perturbation_seed=100)


def one_metric(metric):
    from sklearn.manifold import trustworthiness
    c = CASE
    X, _ = R.blobs(c["N"], c["D"], c["centres"], c["data_seed"])
    k = int(min(c["N"] - 1, 63, np.floor(3 * c["perplexity"])))
    idx, dist = R.exact_knn(X, k, metric)
    d = R.squared_f32(dist) if metric == "euclidean" else dist
    P = R.joint_p(idx, R.conditional_p(d, c["perplexity"])[0])
    Y0 = R.pca_init(X)
    kls, trusts, iters = [], [], []
    for r in range(c["runs"]):
        rs = np.random.RandomState(c["perturbation_seed"] + r)
        Y = (Y0 * (1.0 + c["perturbation"] * rs.standard_normal(Y0.shape))).astype(np.float32)
        Y, _, last = R.fit(P, Y, max_iter=c["max_iter"])
        kl = R.kl_and_grad(P, Y)[0]                          # recomputed in fp64 from the final embedding
        t = float(trustworthiness(X.astype(np.float64), Y.astype(np.float64), n_neighbors=c["n_neighbors"], metric=metric))
        print(f"{metric} run {r}: KL {kl:.6f}, trustworthiness {t:.6f}, last iteration {last}", flush=True)
        kls.append(kl); trusts.append(t); iters.append(int(last))
    return dict(kl=kls, trustworthiness=trusts, last_iteration=iters)


def main():
    out = dict(CASE)
    out["runs"] = {m: one_metric(m) for m in ("euclidean", "cosine")}
    out["runs_per_metric"] = CASE["runs"]
    path = os.path.join(ROOT, "tests", "golden", "tsne_fit_band.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
