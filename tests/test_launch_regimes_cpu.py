"""tests/launch_regimes.py without a GPU: every row's regime really is selected (by the host library's size queries and by
the constants in the sources, read from the lines the row names), the table hits every regime it declares on both sides of
every threshold, and the label checks of the GPU file keep at least 90 % of their rows on the references alone."""
import os

import numpy as np
import pytest

import launch_regimes as LR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vit_som_amd", "csrc")
IDS = [f"{r.regime}-{LR.row_id(r)}" for r in LR.ROWS]


def test_table_hits_every_regime_on_both_sides_of_every_threshold():
    assert {r.regime for r in LR.ROWS} == LR.REGIMES
    assert len({(r.entry, r.shape) for r in LR.ROWS}) == len(LR.ROWS)
    for pair in {r.pair for r in LR.ROWS}:
        sides = {r.side for r in LR.ROWS if r.pair == pair}
        assert sides == {"below", "past"}, (pair, sides)
    for r in LR.ROWS:
        assert r.const in LR.CONSTANTS and os.path.exists(os.path.join(CSRC, r.module)) and LR.CONSTANTS[r.const].file == r.module
        assert r.query is not None or LR.CONSTANTS[r.const].threshold is not None, r      # the regime shows somewhere
        if r.covered_by:
            path, name = r.covered_by.split("::")
            assert f"def {name.split('[')[0]}(" in open(os.path.join(ROOT, "tests", path)).read(), r.covered_by


@pytest.mark.parametrize("key", sorted(LR.CONSTANTS))
def test_constants_are_what_the_table_assumes(key):
    """A cap that somebody raises must fail here, not quietly move the shapes back under the threshold."""
    want = tuple(v for _, vals in LR.CONSTANTS[key].patterns for v in vals)
    assert LR.read_constant(key, CSRC) == want


@pytest.mark.parametrize("r", LR.ROWS, ids=IDS)
def test_shape_is_on_its_side_of_the_threshold(r):
    c = LR.CONSTANTS[r.const]
    if c.threshold is None:                           # pca_plan has no single threshold: test_plan_follows_from_the_sources
        assert r.plan and r.query
        return
    threshold = c.threshold(*LR.read_constant(r.const, CSRC))
    assert (r.size > threshold) == (r.side == "past"), (r.size, threshold)


@pytest.mark.parametrize("r", [r for r in LR.ROWS if r.query], ids=[i for i, r in zip(IDS, LR.ROWS) if r.query])
def test_query_shows_the_split(r):
    from vit_som_amd._lib import lib
    name, args, want = r.query
    assert getattr(lib, name)(*args) == want


@pytest.mark.parametrize("r", [r for r in LR.ROWS if r.plan], ids=[i for i, r in zip(IDS, LR.ROWS) if r.plan])
def test_plan_follows_from_the_sources(r):
    """The figures written into the table against the plan functions restated in launch_regimes.py, fed with the constants as
    the sources have them now."""
    k, p = LR.read_constant(r.const, CSRC), r.plan
    if r.entry in ("vsom_gmm_estep", "vsom_kmeans_assign"):
        groups, rows_per, steps, _, last_step = LR.row_steps(r.shape[0], k[0], (k[1] // 64) * k[2])
        assert (groups, rows_per, steps, last_step) == (p["groups"], p["rows_per"], p["steps"], p["last_step"])
        assert (steps > 1) == (r.side == "past")
        if r.entry == "vsom_gmm_estep":
            N, D, K = r.shape
            vec = 4 if D % 4 == 0 else 1
            dt = min((128 * 1024 // (2 * 8 * 4)) // (64 * vec) * (64 * vec), LR.cdiv(D, 64 * vec) * 64 * vec)     # row_tile_width
            assert (LR.cdiv(K, 8), LR.cdiv(D, dt), vec) == (p["chunks"], p["dtiles"], p["vec"])
            resident = p["chunks"] == 1 and p["dtiles"] == 1
            assert resident == ("resident" in r.regime or r.side == "below")
    elif r.entry in ("vsom_gmm_mstep", "vsom_gmm_params"):
        s = LR.read_constant("gmm.slabs", CSRC)
        assert LR.gmm_slab_rows(*r.shape, max_slabs=s[0], rows=s[1]) == p["slab_rows"]
        if r.entry == "vsom_gmm_mstep":
            assert (p["slab_rows"] > s[1]) == (r.side == "past")
    elif r.entry == "vsom_tsne_step":
        n_z = LR.cdiv(r.shape[0], k[2])
        assert (n_z, LR.cdiv(n_z, k[1])) == (p["n_z"], p["seg"]) and (p["seg"] > 1) == (r.side == "past")
    elif r.entry in ("vsom_probe_residual", "vsom_probe_linesearch"):
        assert LR.probe_row_plan(*r.shape, max_blocks=k[0]) == (p["rows_per"], p["blocks"])
        assert (p["rows_per"] > 16) == (r.side == "past")
    elif r.entry in ("vsom_lbfgs_dots", "vsom_probe_fold"):
        n = r.shape[0] if r.entry == "vsom_lbfgs_dots" else r.shape[0] * r.shape[1]
        assert LR.vec_plan(n, k[0], k[1]) == (p["chunks_per"], p["blocks"]) and (p["chunks_per"] > 1) == (r.side == "past")
    elif r.entry == "vsom_knn_query":
        assert LR.knn_query_plan(r.shape[0], r.shape[1], *k) == p
        assert (p["chunks"] < p["ct"]) == (p["most_tiles"] > 1) == (r.side == "past")
    elif r.entry == "vsom_bmu_manhattan_fwd":
        assert LR.l1_splits(*r.shape, most=k[0], want=k[2]) == p and p["per"] * (p["splits"] - 1) + p["last"] == p["nchunks"]
        assert (p["last"] < p["per"]) == (r.side == "past") and p["splits"] > 1
    else:
        assert r.entry in ("vsom_pca_project", "vsom_pca_backproject")
        N, D, l = r.shape
        assert LR.pca_plan(N, D, l, int(r.entry == "vsom_pca_backproject"), *k) == p
        assert p["per"] * (p["splits"] - 1) + p["last"] == p["ktiles"]
        if r.regime == "pca.even_split":
            assert p["last"] == p["per"] and p["splits"] > 1
        elif r.regime == "pca.short_last_split":
            assert 0 < p["last"] < p["per"] and 1 < p["splits"] < min(k[1], p["ktiles"])
        elif r.regime == "pca.splits_under_cap":
            assert 1 < p["splits"] < min(k[1], p["ktiles"]) and p["last"] < p["per"]
        else:
            assert p["splits"] == (1 if r.regime == "pca.single_split" else 2)


def test_bad_rows_sit_in_second_steps():
    for shape, bad in LR.ESTEP_BAD_ROWS:
        groups, rows_per, steps, last, _ = LR.row_steps(shape[0], 256)
        assert steps >= 2 and any(r.shape == shape for r in LR.rows_of("vsom_gmm_estep"))
        for row in bad:
            assert 32 <= row % rows_per < 64 and row < shape[0]                     # the second 32-row step of its workgroup
        assert any(row // rows_per == groups - 1 for row in bad) or shape == (8193, 8, 3)
    assert any(row // LR.row_steps(shape[0], 256)[1] == LR.row_steps(shape[0], 256)[0] - 1
               for shape, bad in LR.ESTEP_BAD_ROWS for row in bad)                  # one of them in a last workgroup


# ------------------------------------------------------------------ the label checks never pass empty
@pytest.mark.parametrize("r", LR.rows_of("vsom_kmeans_assign") + LR.rows_of("vsom_kmeans_update"), ids=LR.row_id)
def test_kmeans_label_check_keeps_its_rows(r):
    from test_kmeans_cpu import assign_oracle
    from test_kmeans_gpu import _data
    N, D, k = r.shape
    X, C = _data(N + D + k, N, D, k)
    _, ref_m, gap = assign_oracle(X.numpy(), C.numpy())
    share = float((gap > 1e-4 * np.maximum(ref_m, 1e-30)).mean())
    print(f"k-means {r.shape}: {share:.4f} of the rows have a clear fp64 gap")
    assert share >= LR.MIN_SHARE


@pytest.mark.parametrize("ctype", ["diag", "spherical"])
@pytest.mark.parametrize("r", LR.rows_of("vsom_gmm_estep"), ids=LR.row_id)
def test_gmm_label_check_keeps_its_rows(r, ctype):
    import gmm_ref as R
    N, D, K = r.shape
    X, means, prec, w = R.mixture_case(N, D, K, ctype)
    prec = prec.astype(np.float32).astype(np.float64)
    share = float((R.estep64(X, means, prec, w)["gap"] > R.GAP).mean())
    print(f"GMM {r.shape} {ctype}: {share:.4f} of the rows have a clear fp64 gap")
    assert share >= LR.MIN_SHARE


def test_torch_restatement_of_the_tsne_gradient_is_tsne_ref():
    """test_launch_regimes_gpu.kl_and_grad_torch (run on the device there) against tsne_ref.kl_and_grad, here on the host."""
    import torch
    import tsne_ref as R
    from launch_regimes import kl_and_grad_torch
    from vit_som_amd.tsne import joint_probabilities
    N = 300
    X, _ = R.blobs(N, 16, 5, 40 + N, scale=3.0)
    idx, dist = R.exact_knn(X, 63, "euclidean")
    Pd = np.asarray(joint_probabilities(idx, R.conditional_p(R.squared_f32(dist), 20.0)[0]).todense())
    Y = (3.0 * np.random.RandomState(N).standard_normal((N, 2))).astype(np.float32)
    for exaggeration in (12.0, 1.0):
        kl_r, grad_r = R.kl_and_grad(Pd, Y, exaggeration)
        kl_t, grad_t = kl_and_grad_torch(torch.from_numpy(Pd), torch.from_numpy(Y), exaggeration, torch.float64)
        assert abs(kl_t - kl_r) <= 1e-12 * abs(kl_r) and np.abs(grad_t - grad_r).max() <= 1e-12 * np.abs(grad_r).max()


@pytest.mark.parametrize("r", LR.rows_of("vsom_knn_query"), ids=LR.row_id)
def test_knn_index_check_keeps_its_rows(r):
    """The rows knn_checks.lists_against_fp64 compares index by index (clear fp64 gaps), on the GPU test's inputs."""
    from knn_checks import clear_rows, fp64_distances
    from test_knn_gpu import _randn
    Nq, Nb, D, k = r.shape
    Q, X = _randn(Nq, Nb, D)
    for metric in ("cosine", "euclidean"):
        ref, sqq, sqx = fp64_distances(Q, X, metric)
        share = float(clear_rows(ref, sqq, sqx, k, metric)[0].double().mean())
        print(f"kNN {r.shape} {metric}: {share:.4f} of the rows have clear fp64 gaps")
        assert share >= LR.MIN_SHARE
