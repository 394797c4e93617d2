"""The checks of a set of neighbour lists against fp64, written once: test_knn_gpu.py::test_query_against_fp64 holds
vsom_knn_query to them on N(0, 1) rows, test_eval_edges_gpu.py holds the good rows of every edge case to them, and
test_eval_edges_cpu.py runs them on the CPU restatement.  Pure torch: the lists may live on any device."""
import torch

FLOOR = 1e-5          # cosine: absolute on the distance; euclidean: on the squared distance, relative to |q|^2 + |x|^2


def fp64_distances(Q, X, metric):
    """(ref [Nq, Nb], sqq, sqx) in fp64: the squared euclidean distance, or the cosine distance (unclamped)."""
    Qd, Xd = Q.double(), X.double()
    sqq, sqx = (Qd * Qd).sum(1), (Xd * Xd).sum(1)
    G = Qd @ Xd.T
    if metric == "euclidean":
        return (sqq[:, None] + sqx[None, :] - 2.0 * G).clamp_min(0.0), sqq, sqx
    return 1.0 - G / (sqq.sqrt()[:, None] * sqx.sqrt()[None, :]), sqq, sqx


def clear_rows(ref, sqq, sqx, k, metric, tol=FLOOR):
    """(clear [Nq] bool, ri [Nq, k + 1]): the rows whose k + 1 smallest fp64 distances are pairwise further apart than the
    tolerance, and the fp64 top-(k + 1)."""
    rv, ri = torch.topk(ref, min(k + 1, ref.shape[1]), largest=False, sorted=True)
    if metric == "euclidean":
        sqj = sqx[ri]
        gap_tol = tol * (sqq[:, None] + torch.maximum(sqj[:, 1:], sqj[:, :-1]))
    else:
        gap_tol = torch.full_like(rv[:, 1:], tol)
    return ((rv[:, 1:] - rv[:, :-1]) > gap_tol).all(dim=1), ri


def distance_error(idx, dist, ref, sqq, sqx, metric):
    """The largest error of the returned distances against the fp64 distance of the index returned with each, in the
    unit of the tolerance (see FLOOR)."""
    mine = ref.gather(1, idx)
    if metric == "euclidean":
        return float(((dist.double() ** 2 - mine).abs() / (sqq[:, None] + sqx[idx]).clamp_min(1e-300)).max())
    return float((dist.double() - mine).abs().max())


def lists_against_fp64(idx, dist, Q, X, k, metric, tol=FLOOR, indices=True):
    """Full lists (idx int64 / dist f32 [Nq, k], Nb >= k) against fp64: indices are valid, the lists ascend by (distance,
    index), every returned distance agrees with the fp64 distance of its index (cosine `tol`; euclidean squared, `tol`
    (|q|^2 + |x|^2)), and on every clear row (clear_rows) the indices are the fp64 top-k exactly (`indices=False`: not
    compared, for data on which fp64 separates no row).  -> (share of clear rows, the distance error)."""
    Nb = X.shape[0]
    assert ((idx >= 0) & (idx < Nb)).all()
    assert (dist[:, 1:] >= dist[:, :-1]).all() and torch.isfinite(dist).all()
    same_d = dist[:, 1:] == dist[:, :-1]
    assert (~same_d | (idx[:, 1:] > idx[:, :-1])).all()              # equal distances: ascending index
    ref, sqq, sqx = fp64_distances(Q, X, metric)
    err = distance_error(idx, dist, ref, sqq, sqx, metric)
    assert err <= tol, err
    clear, ri = clear_rows(ref, sqq, sqx, k, metric, tol)
    if indices:
        assert torch.equal(idx[clear], ri[clear, :k])
    return float(clear.double().mean()), err
