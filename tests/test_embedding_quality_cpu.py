"""Trustworthiness / continuity without GPU compute: the restatement (embedding_quality_ref.py) against
sklearn.manifold.trustworthiness and on hand-checkable cases, the host arithmetic of embedding_quality.py, the argument
refusals of vsom_knn_ranks and the driver flag."""
import numpy as np
import pytest
import torch

import embedding_quality_ref as R


def fixture_a():
    """The integer fixture of the exact GPU test: (X [130, 8], E [130, 2], k)."""
    X = np.random.default_rng(2).integers(0, 1024, (130, 8))
    E = X[:, :2] + np.random.default_rng(311).integers(0, 512, (130, 2))
    return X, E, 15


def rows_distinct(D):
    """Every row's off-diagonal entries pairwise distinct."""
    N = D.shape[0]
    off = D[~np.eye(N, dtype=bool)].reshape(N, N - 1)
    return all(len(np.unique(r)) == N - 1 for r in off)


# ------------------------------------------------------------------ the restatement
def test_restatement_equals_sklearn_on_the_integer_fixture():
    import sklearn.manifold as sk
    X, E, k = fixture_a()
    DX, DE = R.sq_distances(X), R.sq_distances(E)
    assert rows_distinct(DX) and rows_distinct(DE)
    # float32 square roots keep the squared distances apart, so the device (which compares sqrtf values) sees no tie either
    assert rows_distinct(np.sqrt(DX.astype(np.float64)).astype(np.float32))
    assert rows_distinct(np.sqrt(DE.astype(np.float64)).astype(np.float32))
    t, c = R.trustworthiness(DX, DE, k), R.trustworthiness(DE, DX, k)
    assert t == sk.trustworthiness(X.astype(np.float64), E.astype(np.float64), n_neighbors=k) == 0.6860484064222382
    assert c == sk.trustworthiness(E.astype(np.float64), X.astype(np.float64), n_neighbors=k) == 0.7324610591900311
    for ties in ("max", "average"):
        assert R.trustworthiness(DX, DE, k, ties) == t and R.trustworthiness(DE, DX, k, ties) == c


@pytest.mark.parametrize("N,D,d,k,seed", [(60, 5, 2, 7, 0), (200, 16, 3, 20, 1)])
def test_restatement_equals_sklearn_on_real_data(N, D, d, k, seed):
    import sklearn.manifold as sk
    rng = np.random.default_rng(seed)
    X, E = rng.standard_normal((N, D)), rng.standard_normal((N, d))
    DX = np.sqrt(((X[:, None] - X[None]) ** 2).sum(-1))
    DE = np.sqrt(((E[:, None] - E[None]) ** 2).sum(-1))
    assert rows_distinct(DX) and rows_distinct(DE)
    want = sk.trustworthiness(X, E, n_neighbors=k)
    got = {ties: R.trustworthiness(DX, DE, k, ties) for ties in R.TIES}
    assert abs(got["min"] - want) <= 1e-12
    assert got["min"] == got["max"] == got["average"]


def test_counts_and_tie_policies_by_hand():
    # row 0 sees the others at 1, 1, 2, 2, 2, 5
    D = np.zeros((7, 7))
    D[0] = [0, 1, 1, 2, 2, 2, 5]
    nbr = np.full((7, 4), -1)
    nbr[0] = [4, 6, 0, -1]                                         # a tied row, the farthest, itself, empty
    less, tied = R.counts(D, nbr)
    assert less[0].tolist() == [2, 5, -1, -1] and tied[0].tolist() == [2, 0, -1, -1]
    assert R.ranks(less, tied, "min")[0, :2].tolist() == [3.0, 6.0]
    assert R.ranks(less, tied, "max")[0, :2].tolist() == [5.0, 6.0]
    assert R.ranks(less, tied, "average")[0, :2].tolist() == [4.0, 6.0]
    assert R.penalties(less, tied, 3, "min")[0] == 3.0 and R.penalties(less, tied, 3, "max")[0] == 5.0
    assert R.penalties(less, tied, 3, "average")[0] == 4.0
    assert R.neighbours(np.tile(D[0], (7, 1)), 3)[0].tolist() == [1, 2, 3]     # ties: the lower index first


def test_host_arithmetic_of_the_module_is_the_restatement():
    from vit_som_amd.embedding_quality import penalties_from_counts, score_from_penalty
    rng = np.random.default_rng(5)
    less = rng.integers(0, 40, (50, 6))
    tied = rng.integers(0, 4, (50, 6))
    less[3, 2] = tied[3, 2] = -1
    for ties in R.TIES:
        got = penalties_from_counts(less, tied, 6, ties)
        assert np.array_equal(np.asarray(got, dtype=np.float64), R.penalties(less, tied, 6, ties)), ties
        assert got.dtype == (np.float64 if ties == "average" else np.int64)
    assert score_from_penalty(1234, 130, 15) == R.score(1234, 130, 15)
    with pytest.raises(ValueError, match="ties"):
        penalties_from_counts(less, tied, 6, "first")


def test_value_errors_before_any_launch():
    from vit_som_amd import trustworthiness
    X, E = torch.zeros(10, 4), torch.zeros(10, 2)
    with pytest.raises(ValueError, match="on the GPU"):
        trustworthiness(X, E)


# ------------------------------------------------------------------ the C-ABI, host side
def test_workspace_bytes_is_host_arithmetic():
    from vit_som_amd._lib import lib
    f = lib.vsom_knn_ranks_workspace_bytes
    assert f(0, 1) == 0 and f(10, 0) == 0 and f(-3, 5) == 0
    assert f(10000, 15) >= 4 * 10000 + 8 * 10000 * 15                # the norms, a threshold and a neighbour per slot
    sizes = [f(N, 20) for N in (2, 127, 128, 129, 1000, 10000, 1000000)]
    assert all(b >= a for a, b in zip(sizes, sizes[1:]))


def test_argument_refusals_without_a_launch():
    """Bad calls are refused on the host before any launch (negative VSOM_E* codes); 16 stands for a non-null pointer."""
    from vit_som_amd._lib import last_error, lib
    big = 1 << 30

    def ranks(A=16, lda=4, N=4, D=4, metric=0, nbr=16, k=2, less=16, tied=16, ws=16, ws_bytes=big):
        return lib.vsom_knn_ranks(A, lda, N, D, metric, nbr, k, less, tied, ws, ws_bytes, None)

    for null in ("A", "nbr", "less", "tied"):
        assert ranks(**{null: None}) == -1 and "null" in last_error()
    assert ranks(k=65) == -3 and "k=65" in last_error()
    assert ranks(metric=7) == -3 and "metric 7" in last_error()
    assert ranks(metric=2) == -3                                   # manhattan
    assert ranks(ws_bytes=lib.vsom_knn_ranks_workspace_bytes(4, 2) - 1) == -4 and "workspace" in last_error()
    assert ranks(ws=None) == -4 and ranks(ws=24) == -4             # none; not 16-byte aligned
    assert ranks(lda=3) == -1 and ranks(D=0) == -1 and ranks(k=0) == -1 and ranks(N=1) == -1 and ranks(N=2 ** 31) == -1


def test_driver_flag_parses_and_defaults_to_off():
    import inspect
    from vit_som_amd import train
    assert train._parser().parse_args(["--config", "c.yaml"]).embedding_quality is False
    assert train._parser().parse_args(["--config", "c.yaml", "--embedding-quality"]).embedding_quality is True
    assert inspect.signature(train.main).parameters["embedding_quality"].default is False
