"""Silhouette without a GPU: the fp64 restatement (silhouette_ref.py) against sklearn, the restatement's device arithmetic
against its own definition, the wrapper's argument checks and sklearn's error texts, the C entry's argument checks."""
import numpy as np
import pytest
import torch

import silhouette_ref as R


def blobs(N, D, C, seed, spread=4.0):
    rng = np.random.default_rng(seed)
    y = rng.integers(0, C, N)
    y[:C] = np.arange(C)                                         # every cluster has a member
    return (rng.standard_normal((C, D)) * spread)[y] + rng.standard_normal((N, D)), y


def cases():
    X, y = blobs(150, 7, 5, 0)
    yield "blobs", X, y
    y1 = y.copy()
    y1[y1 == 4] = 0
    y1[17] = 4                                                   # cluster 4: one member
    yield "singleton", X, y1
    Xd = X.copy()
    Xd[40:60] = Xd[3]                                            # duplicate rows, in several clusters
    yield "duplicates", Xd, y
    yield "non-dense labels", X, np.array([-7, 3, 10 ** 12, 44, 45])[y]


@pytest.mark.parametrize("metric", [R.EUCLIDEAN, R.COSINE])
def test_restatement_equals_sklearn(metric):
    from sklearn.metrics import silhouette_samples, silhouette_score
    name = "euclidean" if metric == R.EUCLIDEAN else "cosine"
    for what, X, y in cases():
        s, a, b = R.silhouette_fp64(R.distances(X, metric), y)
        want = silhouette_samples(X.astype(np.float64), y, metric=name)
        assert np.abs(s - want).max() <= 1e-12, what
        assert abs(s.mean() - silhouette_score(X.astype(np.float64), y, metric=name)) <= 1e-12, what
        if what == "singleton":
            assert s[17] == 0.0 and (np.delete(s, 17) != 0).all()


@pytest.mark.parametrize("metric", [R.EUCLIDEAN, R.COSINE])
def test_device_arithmetic_of_the_restatement_follows_the_definition(metric):
    """Fixed point at 2^-40 of the bound and fp32 distances: within the rounding of those distances of the definition."""
    for what, X, y in cases():
        names, dense = np.unique(y, return_inverse=True)
        X32 = X.astype(np.float32)
        D32 = R.distances(X32, metric).astype(np.float32)
        S, got = R.device_restatement(D32, dense, len(names), (X32.astype(np.float64) ** 2).sum(1).max(), metric)
        s, a, b = R.silhouette_fp64(R.distances(X32, metric), dense)
        assert np.abs(got["sil"] - s).max() <= 4 * 2.0 ** -23, what
        assert abs(got["score"] - s.mean()) <= 4 * 2.0 ** -23
        assert got["status"] == [0, 0, len(names), int((np.bincount(dense) == 1).sum())]
        assert np.array_equal(got["counts"], np.bincount(dense))


def test_bound_exponent():
    """2^e > 4 sqrt(M) >= 2^(e - 1), for every float32 M including subnormals; a power of two scales e exactly."""
    rng = np.random.default_rng(0)
    M = np.concatenate([np.float32(2.0) ** rng.integers(-149, 128, 400) * rng.uniform(1, 2, 400).astype(np.float32),
                        np.float32([1e-45, 1.0, 4.0, 3.9999998, 3.4e38])])
    for m in M.astype(np.float32)[np.isfinite(M.astype(np.float32)) & (M.astype(np.float32) > 0)]:
        e = R.bound_exponent(m, R.EUCLIDEAN)
        assert 2.0 ** e > 4 * np.sqrt(float(m)) >= 2.0 ** (e - 1), m
        if 1e-20 < m < 1e20:
            assert R.bound_exponent(np.float32(m) * np.float32(2.0 ** 40), R.EUCLIDEAN) == e + 20
    assert R.bound_exponent(0.0, R.EUCLIDEAN) == 0 and R.bound_exponent(123.0, R.COSINE) == 2


class _FakeCuda(torch.Tensor):
    """A CPU tensor that says it lives on the GPU: enough for the argument checks that precede every launch."""
    @property
    def is_cuda(self):
        return True


def test_wrapper_argument_checks():
    from vit_som_amd import cluster_silhouette, silhouette_samples, silhouette_score
    from vit_som_amd.silhouette import check_number_of_labels
    X, y = torch.zeros(6, 3), torch.zeros(6, dtype=torch.int64)
    for fn in (silhouette_samples, silhouette_score, cluster_silhouette):
        with pytest.raises(ValueError, match="on the GPU"):
            fn(X, y)                                               # CPU tensor
        with pytest.raises(ValueError, match="metric must be one of"):
            fn(X, y, metric="manhattan")
        with pytest.raises(ValueError, match="on the GPU"):
            fn(X.numpy(), y)
    Xg = torch.zeros(6, 3).as_subclass(_FakeCuda)
    with pytest.raises(ValueError, match="float32"):
        silhouette_samples(torch.zeros(6, 3, dtype=torch.float64).as_subclass(_FakeCuda), y)
    with pytest.raises(ValueError, match=r"\[N, D\]"):
        silhouette_samples(torch.zeros(6).as_subclass(_FakeCuda), y)
    with pytest.raises(ValueError, match="labels must be an int64"):
        silhouette_samples(Xg, y.int())
    with pytest.raises(ValueError, match="labels must be an int64"):
        silhouette_samples(Xg, y.view(6, 1))
    with pytest.raises(ValueError, match=r"inconsistent numbers of samples: \[6, 5\]"):
        silhouette_samples(Xg, y[:5])
    # sklearn's text, word for word
    import sklearn.metrics
    for n_labels, n_samples in ((1, 6), (6, 6)):
        with pytest.raises(ValueError) as ours:
            check_number_of_labels(n_labels, n_samples)
        with pytest.raises(ValueError) as theirs:
            sklearn.metrics.silhouette_score(np.arange(2.0 * n_samples).reshape(n_samples, 2), np.arange(n_samples) % n_labels)
        assert str(ours.value) == str(theirs.value) == f"Number of labels is {n_labels}. Valid values are 2 to n_samples - 1 (inclusive)"
    check_number_of_labels(2, 3)
    check_number_of_labels(5, 6)


def test_entry_rejects_bad_calls_without_gpu():
    from vit_som_amd._lib import last_error, lib
    from vit_som_amd.ops import SILHOUETTE_MAX_N
    need = lib.vsom_silhouette_workspace_bytes(100, 5)
    ok = dict(X=16, ldx=8, N=100, D=8, metric=1, labels=16, C=5, sil=16, a=None, b=None, nearest=None, counts=16, cluster_mean=None,
              score=16, status=16, ws=256, ws_bytes=need, stream=None)

    def call(**kw):
        return lib.vsom_silhouette(*{**ok, **kw}.values())
    for name in ("X", "labels", "sil", "counts", "score", "status"):
        assert call(**{name: None}) == -1 and "null" in last_error(), name
    assert call(N=1) == -1 and call(N=0) == -1 and call(D=0) == -1 and call(ldx=7) == -1 and call(C=0) == -1 and call(C=-3) == -1
    assert "bad sizes" in last_error()
    big = SILHOUETTE_MAX_N + 1
    assert big == 1 << 22
    assert call(N=big, ws_bytes=lib.vsom_silhouette_workspace_bytes(big, 5)) == -3 and "2^63" in last_error()
    assert call(metric=2) == -3 and call(metric=-1) == -3 and "metric" in last_error()
    assert call(ws=None) == -4 and call(ws=264) == -4 and call(ws_bytes=need - 1) == -4 and call(ws_bytes=0) == -4
    assert "workspace" in last_error()


def test_workspace_bytes_is_monotone():
    from vit_som_amd._lib import lib
    f = lib.vsom_silhouette_workspace_bytes
    assert f(0, 5) == 0 and f(5, 0) == 0 and f(-1, -1) == 0
    Ns = [1, 2, 63, 64, 65, 127, 128, 129, 1000, 4096, 10000, 10001, (1 << 22) - 1]
    Cs = [1, 2, 7, 31, 32, 33, 300, 1600, 1601, 1 << 20]
    table = np.array([[f(n, c) for c in Cs] for n in Ns], dtype=np.float64)
    assert (table > 0).all() and (table % 256 == 0).all()
    assert (np.diff(table, axis=0) >= 0).all() and (np.diff(table, axis=1) >= 0).all()
    assert f(10000, 1600) >= 10000 * 1600 * 8 + 10000 * 4
