"""k-means for evaluate_kmeans, host side: a float64 numpy restatement of sklearn's Lloyd loop (the oracle of
tests/test_kmeans_gpu.py), checked against sklearn itself, plus the workspace arithmetic and argument checks of the
vsom_kmeans_* entries (no launch happens)."""
import numpy as np
import pytest


def assign_oracle(X, C):
    """labels (first argmin), mind, and the gap between the two smallest distances (fp64, direct differences)."""
    X, C = np.asarray(X, np.float64), np.asarray(C, np.float64)
    d = np.empty((X.shape[0], C.shape[0]))
    for j in range(C.shape[0]):
        d[:, j] = ((X - C[j]) ** 2).sum(axis=1)
    labels = d.argmin(axis=1)
    mind = d[np.arange(X.shape[0]), labels]
    if C.shape[0] > 1:
        two = np.partition(d, 1, axis=1)[:, :2]
        gap = two[:, 1] - two[:, 0]
    else:
        gap = np.full(X.shape[0], np.inf)
    return labels, mind, gap


def sums_counts(X, labels, k):
    X = np.asarray(X, np.float64)
    sums = np.zeros((k, X.shape[1]))
    np.add.at(sums, labels, X)
    return sums, np.bincount(labels, minlength=k)


def relocate_oracle(X, sums, counts, labels, mind):
    """_relocate_empty_clusters_dense (unit weights)."""
    empty = np.where(counts == 0)[0]
    n_empty = empty.shape[0]
    if n_empty == 0:
        return sums, counts
    sums, counts = sums.copy(), counts.copy()
    far = np.argpartition(mind, -n_empty)[:-n_empty - 1:-1]
    for new_c, f in zip(empty, far):
        old_c = labels[f]
        sums[old_c] -= X[f]
        sums[new_c] = X[f]
        counts[new_c] = 1
        counts[old_c] -= 1
    return sums, counts


def average_centers(sums, counts):
    """_average_centers (_k_means_common.pyx): in place, in cluster order; an empty cluster takes the current row of
    the first argmax of the counts (already averaged when that cluster comes first)."""
    new = np.array(sums, dtype=np.float64)
    a = int(np.argmax(counts))
    for j in range(new.shape[0]):
        if counts[j] > 0:
            new[j] *= 1.0 / counts[j]
        else:
            new[j] = new[a]
    return new


def donor_case(dtype=np.float64):
    """Data and init where the relocation empties the donor: the one member of cluster 1 is the farthest sample, so it
    moves to the empty cluster 2 and cluster 1 is left empty (placed on the heaviest cluster by _average_centers)."""
    rng = np.random.default_rng(9)
    X = np.concatenate([rng.normal(0.0, 1.0, (200, 2)), [[100.0, 0.0]]]).astype(dtype)
    C0 = np.array([[0.0, 0.0], [190.0, 0.0], [1e6, 0.0]], dtype=dtype)
    return X, C0


def lloyd_oracle(X, C0, max_iter=300, tol=1e-4):
    """_kmeans_single_lloyd with _tolerance -> (labels, inertia, centers, n_iter)."""
    X = np.asarray(X, np.float64)
    tol = np.mean(np.var(X, axis=0)) * tol if tol else 0.0
    centers = np.asarray(C0, np.float64).copy()
    k = centers.shape[0]
    labels_old = np.full(X.shape[0], -1)
    strict = False
    for it in range(max_iter):
        labels, mind, _ = assign_oracle(X, centers)
        sums, counts = sums_counts(X, labels, k)
        sums, counts = relocate_oracle(X, sums, counts, labels, mind)
        new = average_centers(sums, counts)
        shift = ((new - centers) ** 2).sum()
        centers = new
        if np.array_equal(labels, labels_old):
            strict = True
            break
        if shift <= tol:
            break
        labels_old = labels
    if not strict:
        labels, mind, _ = assign_oracle(X, centers)
    return labels, float(mind.sum()), centers, it + 1


def _blobs(seed, n, d, k, spread=1.0, scale=10.0):
    rng = np.random.default_rng(seed)
    means = rng.normal(0, scale, (k, d))
    y = rng.integers(0, k, n)
    return means[y] + rng.normal(0, spread, (n, d)), y


@pytest.mark.parametrize("seed,n,d,k,spread", [(0, 300, 5, 4, 3.0), (1, 500, 17, 7, 6.0), (2, 200, 3, 3, 8.0), (3, 120, 2, 1, 1.0)])
def test_lloyd_oracle_matches_sklearn(seed, n, d, k, spread):
    from sklearn.cluster import KMeans
    X, _ = _blobs(seed, n, d, k, spread=spread)
    C0 = X[np.random.default_rng(seed + 100).choice(n, k, replace=False)]
    ref = KMeans(n_clusters=k, init=C0, n_init=1, algorithm="lloyd").fit(X)
    labels, inertia, centers, n_iter = lloyd_oracle(X, C0)
    assert np.array_equal(labels, ref.labels_)
    assert n_iter == ref.n_iter_
    assert abs(inertia - ref.inertia_) <= 1e-12 * abs(ref.inertia_)
    assert np.allclose(centers, ref.cluster_centers_, rtol=1e-10, atol=1e-10)


def test_lloyd_oracle_relocates_like_sklearn():
    """A centre far from all data owns no sample in the first pass: relocation to the farthest point."""
    from sklearn.cluster import KMeans
    X, _ = _blobs(5, 400, 6, 3, spread=2.0)
    C0 = np.concatenate([X[:3], np.full((1, 6), 1e3)])
    ref = KMeans(n_clusters=4, init=C0, n_init=1, algorithm="lloyd").fit(X)
    labels, inertia, centers, n_iter = lloyd_oracle(X, C0)
    assert np.array_equal(labels, ref.labels_) and n_iter == ref.n_iter_
    assert abs(inertia - ref.inertia_) <= 1e-12 * abs(ref.inertia_)


def test_lloyd_oracle_empty_donor_like_sklearn():
    """_average_centers' rule for a cluster the relocation emptied."""
    from sklearn.cluster import KMeans
    X, C0 = donor_case()
    labels0, mind0, _ = assign_oracle(X, C0)
    sums, counts = sums_counts(X, labels0, 3)
    sums, counts = relocate_oracle(X, sums, counts, labels0, mind0)
    assert counts[1] == 0                                 # the case under test really happens
    ref = KMeans(n_clusters=3, init=C0, n_init=1, algorithm="lloyd", max_iter=1).fit(X)
    assert np.allclose(average_centers(sums, counts), ref.cluster_centers_, rtol=1e-12, atol=1e-12)
    ref = KMeans(n_clusters=3, init=C0, n_init=1, algorithm="lloyd").fit(X)
    labels, inertia, centers, n_iter = lloyd_oracle(X, C0)
    assert np.array_equal(labels, ref.labels_) and n_iter == ref.n_iter_
    assert abs(inertia - ref.inertia_) <= 1e-12 * abs(ref.inertia_)


def test_kmeans_workspace_bytes():
    from vit_som_amd._lib import lib
    # CIFAR recon: one workgroup per CU (256), slabs [256, 10, 3072] f32 + counts + changed + sums + shift partials
    ws = lib.vsom_kmeans_workspace_bytes(50000, 3072, 10)
    assert ws >= 256 * 10 * 3072 * 4 + 256 * 10 * 4 + 256 * 4 + 10 * 3072 * 4
    assert ws < 256 * 10 * 3072 * 4 + (1 << 20)
    assert ws % 256 == 0
    # large k * D: slabs capped near 128 MiB (fewer workgroups)
    big = lib.vsom_kmeans_workspace_bytes(1000, 12288, 200)
    assert 200 * 12288 * 4 * 2 <= big <= (129 << 20) + 200 * 12288 * 4 + (1 << 20)
    # few rows: one workgroup per 32 rows
    assert lib.vsom_kmeans_workspace_bytes(40, 8, 2) >= 2 * 2 * 8 * 4
    # the tolerance pass' fp64 partials fit even when the slabs are small
    assert lib.vsom_kmeans_workspace_bytes(64, 1000, 1) >= 64 * 2 * 1000 * 8
    assert lib.vsom_kmeans_workspace_bytes(0, 8, 2) == 0
    assert lib.vsom_kmeans_workspace_bytes(10, 8, 0) == 0


def test_kmeans_argument_validation_without_gpu():
    from vit_som_amd._lib import last_error, lib
    ws = lib.vsom_kmeans_workspace_bytes(100, 8, 4)
    a = 16                                                           # any non-null, 16-byte aligned value: never dereferenced
    assert lib.vsom_kmeans_assign(None, 8, 100, 8, a, 4, a, a, a, a, ws, None) == -1 and "null" in last_error()
    assert lib.vsom_kmeans_assign(a, 8, 100, 8, a, 0, a, a, a, a, ws, None) == -1                 # k < 1
    assert lib.vsom_kmeans_assign(a, 8, 3, 8, a, 4, a, a, a, a, ws, None) == -1                   # k > N
    assert lib.vsom_kmeans_assign(a, 7, 100, 8, a, 4, a, a, a, a, ws, None) == -1                 # ldx < D
    assert lib.vsom_kmeans_assign(a, 8, 100, 8, a, 4, a, a, a, a, ws - 1, None) == -4             # short workspace
    assert lib.vsom_kmeans_assign(a, 8, 100, 8, a, 4, a, a, a, None, ws, None) == -4              # no workspace
    big = lib.vsom_kmeans_workspace_bytes(5000, 8, 2000)
    assert lib.vsom_kmeans_assign(a, 8, 5000, 8, a, 2000, a, a, a, a, big, None) == -3            # k > 1024
    assert lib.vsom_kmeans_update(a, a, 100, 8, 4, a, a, None, a, ws, None) == -1                 # no status
    assert lib.vsom_kmeans_update(a, a, 100, 8, 4, a, a, a, a, ws, None) == -1 and "alias" in last_error()
    assert lib.vsom_kmeans_update(a, 32, 100, 8, 4, a, a, a, a, ws - 1, None) == -4
    assert lib.vsom_kmeans_relocate(a, 8, 100, 8, 4, a, a, 0, a, 32, a, a, a, ws, None) == -1      # no move
    assert lib.vsom_kmeans_relocate(a, 8, 100, 8, 4, a, a, 5, a, 32, a, a, a, ws, None) == -1      # more moves than clusters
    assert lib.vsom_kmeanspp_dist(a, 8, 100, 8, a, 0, None, a, a, None) == -1                     # no candidate
    assert lib.vsom_kmeanspp_dist(a, 8, 100, 8, a, 65, None, a, a, None) == -1                    # > 64 candidates
    assert lib.vsom_kmeanspp_dist(a, 4, 100, 8, a, 3, None, a, a, None) == -1                     # ldx < D
    assert lib.vsom_kmeans_colvar(a, 8, 100, 8, 4, None, a, ws, None) == -1
    assert lib.vsom_kmeans_colvar(a, 8, 100, 8, 4, a, a, 16, None) == -4
