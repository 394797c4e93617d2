"""The evaluation kernels on the MI355X at the numerical edges of eval_edges.py, through vit_som_amd.ops: the bad-row
contract of the kNN search in both modes (a NaN, an infinity or an overflowed norm is in no list, a bad query has none, and
every other list is bit for bit that of the call without the bad rows), rows at a common offset with exact copies, rows
scaled by powers of two, the neighbour ranks with bad rows, the softmax vote at latent-width distances, the k-means steps
at an offset and with bad rows, and the linear probe's residual on saturated logits.

A kernel's error e_k passes when e_k <= max(FLOOR, 4 e32) (eval_edges.py).  Every figure is printed as
`edge <case> <output> e_k e32 bound` before it is asserted: profiles/eval_numeric_edges.txt is that output."""
import math

import numpy as np
import pytest
import torch

import eval_edges as E
import knn_checks as KC
import knn_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _record(case, output, e_k, e32, floor):
    b = E.bound(floor, e32)
    print(f"edge {case} {output} e_k {e_k:.3e} e32 {e32:.3e} bound {b:.3e}")
    return b


def _query(Q, X, k, metric, poison=-7, **kw):
    from vit_som_amd import ops
    idx = torch.full((Q.shape[0], k), poison, dtype=torch.int64, device=DEV)
    dist = torch.full((Q.shape[0], k), float(poison), dtype=torch.float32, device=DEV)
    ops.knn_query(Q, X, k, E.METRIC_ID[metric], idx, dist, **kw)
    return idx, dist


def _umap(X, k, metric, poison=-7):
    from vit_som_amd import ops
    idx = torch.full((X.shape[0], k), poison, dtype=torch.int64, device=DEV)
    dist = torch.full((X.shape[0], k), float(poison), dtype=torch.float32, device=DEV)
    ops.umap_knn(X, k, E.METRIC_ID[metric], idx, dist)
    return idx, dist


def _search(inp, Q, X):
    return _umap(X, inp["k"], inp["metric"]) if inp["self_mode"] else _query(Q, X, inp["k"], inp["metric"])


def _strided(M):
    """The rows in a buffer of D + 1 columns, the padding NaN: the generic loads, which must never read it."""
    buf = torch.full((M.shape[0], M.shape[1] + 1), math.nan, device=DEV)
    buf[:, :M.shape[1]] = M
    return buf[:, :M.shape[1]]


def _good_rows_against_fp64(c, idx_del, dist_del, variant=""):
    """The fp64 checks of test_knn_gpu.py::test_query_against_fp64 (knn_checks.py) on the lists of the good rows."""
    inp = c.inp
    tol = E.bound(E.FLOOR["knn"], c.e32["d"])
    share, err = KC.lists_against_fp64(idx_del.cpu(), dist_del.cpu(), inp["Qg"], inp["Xk"], inp["k"], inp["metric"], tol=tol)
    _record(c.name + variant, "dist", err, c.e32["d"], E.FLOOR["knn"])
    assert share >= 0.5, share


# ------------------------------------------------------------------ (a) the search, bad rows
VARIANTS = [("tiles", "plain"), ("tiles", "strided"), ("tiles", "streamed"), ("elementwise", "plain")]


@pytest.mark.parametrize("metric", E.METRICS)
@pytest.mark.parametrize("kind", E.BAD_KINDS)
@pytest.mark.parametrize("shape,variant", VARIANTS)
def test_query_keeps_the_bad_row_contract(shape, variant, kind, metric):
    c = E.knn_bad_case(shape, kind, metric)
    inp = c.inp
    Q, X, k = inp["Q"].to(DEV), inp["X"].to(DEV), inp["k"]
    if variant == "strided":
        Q, X = _strided(Q), _strided(X)
        assert Q.stride(0) == Q.shape[1] + 1
    if variant == "streamed":                    # the bank folded in two pieces, bad rows 0, 63 and 64 in the first
        from vit_som_amd import ops
        idx, dist = _query(Q, X[:100], k, metric)
        ops.knn_query(Q, X[100:], k, E.METRIC_ID[metric], idx, dist, index_base=100, accumulate=True)
    else:
        idx, dist = _query(Q, X, k, metric)
    idx_del, dist_del = _query(inp["Qg"].to(DEV), inp["Xk"].to(DEV), k, metric, poison=-3)
    torch.cuda.synchronize()
    assert E.bad_row_contract(idx, dist, idx_del, dist_del, inp) == []
    _good_rows_against_fp64(c, idx_del, dist_del, "-" + variant)


@pytest.mark.parametrize("weights", [R.UNIFORM, R.DISTANCE, R.SOFTMAX])
def test_bad_queries_vote_minus_one_and_are_counted(weights):
    """The lists of the bad queries, fed to knn_vote: no prediction, counted in status[1]; and nothing is refused."""
    from vit_som_amd import ops
    c = E.knn_bad_case("tiles", "mixed", "euclidean")
    inp = c.inp
    idx, dist = _query(inp["Q"].to(DEV), inp["X"].to(DEV), inp["k"], "euclidean")
    labels = torch.randint(0, 10, (inp["X"].shape[0],), generator=torch.Generator().manual_seed(7)).to(DEV)
    pred = torch.full((idx.shape[0],), -5, dtype=torch.int64, device=DEV)
    scores = torch.full((idx.shape[0], 10), -5.0, dtype=torch.float64, device=DEV)
    status = torch.zeros(2, dtype=torch.int32, device=DEV)
    ops.knn_vote(idx, dist, labels, 10, weights, 0.07, pred, status, scores)
    assert status.tolist() == [0, len(inp["bad_q"])]
    assert (pred[inp["bad_q"]] == -1).all() and (scores[inp["bad_q"]] == 0).all()
    good = inp["good"].to(DEV)
    assert (pred[good] >= 0).all() and (scores[good].sum(1) > 0).all()


def test_classifier_reports_bad_queries_through_the_vote():
    from vit_som_amd import KNNClassifier
    c = E.knn_bad_case("tiles", "mixed", "cosine")
    inp = c.inp
    y = torch.randint(0, 10, (inp["X"].shape[0],), generator=torch.Generator().manual_seed(7)).to(DEV)
    clf = KNNClassifier(n_neighbors=inp["k"], weights="softmax", metric="cosine").fit(inp["X"].to(DEV), y)
    pred = clf.predict(inp["Q"].to(DEV))
    assert (pred[inp["bad_q"]] == -1).all() and (pred[inp["good"].to(DEV)] >= 0).all()
    assert clf._status.tolist() == [0, len(inp["bad_q"])] and clf.refused() == 0


# ------------------------------------------------------------------ (b) the self mode, bad rows
@pytest.mark.parametrize("metric", E.METRICS)
@pytest.mark.parametrize("kind", E.BAD_KINDS)
def test_umap_knn_keeps_the_bad_row_contract(kind, metric):
    c = E.umap_bad_case(kind, metric)
    inp = c.inp
    idx, dist = _umap(inp["X"].to(DEV), inp["k"], metric)
    idx_del, dist_del = _umap(inp["Xk"].to(DEV), inp["k"], metric, poison=-3)
    torch.cuda.synchronize()
    assert E.bad_row_contract(idx, dist, idx_del, dist_del, inp) == []
    _good_rows_against_fp64(c, idx_del, dist_del)


def test_callers_refuse_empty_slots():
    """UMAP.fit and the trustworthiness / continuity entry would turn an empty slot into a number: they raise, naming the count."""
    from vit_som_amd import UMAP, rank_penalties
    c = E.umap_bad_case("mixed", "euclidean")
    X = c.inp["X"].to(DEV)
    n_bad = len(c.inp["bad_x"])
    with pytest.raises(ValueError, match=f"{n_bad * (E.UMAP_K - 1)} neighbour slots are empty"):
        UMAP(n_neighbors=E.UMAP_K, n_epochs=5).fit(X)
    emb = torch.randn(X.shape[0], 2, generator=torch.Generator().manual_seed(1)).to(DEV)
    with pytest.raises(ValueError, match=f"{n_bad * 5} neighbour slots are empty"):
        rank_penalties(emb, X, 5)                                     # the neighbours come from the set with bad rows
    with pytest.raises(ValueError, match="could not be ranked"):
        rank_penalties(X, emb, 5)                                     # the ranks do


# ------------------------------------------------------------------ offset_dup and pow2, both modes
@pytest.mark.parametrize("self_mode", [False, True])
@pytest.mark.parametrize("metric", E.METRICS)
def test_offset_rows_with_exact_copies(metric, self_mode):
    """rows = 1000 + N(0, 1): every copy at exactly 0 and first, identical bank rows in index order, every returned distance
    within max(FLOOR, 4 e32) of the fp64 distance of its index.  (Indices are not compared with fp64: at this offset the
    tolerance is wider than the distances, DESIGN.md "kNN".)"""
    c = E.offset_dup_case(metric, self_mode)
    inp = c.inp
    idx, dist = _search(inp, inp["Q"].to(DEV), inp["X"].to(DEV))
    torch.cuda.synchronize()
    broken, together = E.offset_dup_violations(idx, dist, inp)
    assert broken == [] and together > 0
    tol = E.bound(E.FLOOR["knn"], c.e32["d"])
    idx, dist = idx.cpu(), dist.cpu()
    if self_mode:                                # the row itself is first whatever its index: the (distance, index) order begins after it
        assert torch.equal(idx[:, 0], torch.arange(idx.shape[0])) and (dist[:, 0] == 0).all()
        idx, dist = idx[:, 1:], dist[:, 1:]
    _, err = KC.lists_against_fp64(idx, dist, inp["Q"], inp["X"], idx.shape[1], metric, tol=tol, indices=False)
    _record(c.name, "dist", err, c.e32["d"], E.FLOOR["knn"])


@pytest.mark.parametrize("self_mode", [False, True])
def test_rows_scaled_by_powers_of_two_change_no_bit(self_mode):
    c = E.pow2_case(self_mode)
    inp = c.inp
    scaled = _search(inp, inp["Q"].to(DEV), inp["X"].to(DEV))
    plain = _search(inp, inp["Q0"].to(DEV), inp["X0"].to(DEV))
    assert torch.equal(scaled[0], plain[0]) and E.bits_equal(scaled[1].cpu(), plain[1].cpu())
    assert (scaled[0] >= 0).all()


# ------------------------------------------------------------------ (c) the ranks, bad rows
def _ranks(A, nbr, metric, poison=-7):
    from vit_som_amd import ops
    nbr = nbr.to(DEV).contiguous()
    less = torch.full(nbr.shape, poison, dtype=torch.int32, device=DEV)
    tied = torch.full(nbr.shape, poison - 1, dtype=torch.int32, device=DEV)
    ops.knn_ranks(A, nbr, E.METRIC_ID[metric], less, tied)
    return less.cpu(), tied.cpu()


@pytest.mark.parametrize("metric", E.METRICS)
@pytest.mark.parametrize("kind", E.BAD_KINDS)
def test_ranks_never_count_a_bad_row(kind, metric):
    """less and tied of every pair of good rows are those of the set with the bad rows deleted; a slot that names a bad row,
    and every slot of a bad row, has nothing to count: -1 in both."""
    c = E.ranks_case(kind)
    inp = c.inp
    less, tied = _ranks(inp["X"].to(DEV), inp["nbr"], metric)
    less_del, tied_del = _ranks(inp["Xk"].to(DEV), inp["nbr_del"], metric, poison=-3)
    keep, names_good = inp["keep"], inp["names_good"]
    assert torch.equal(less[keep], less_del) and torch.equal(tied[keep], tied_del)
    pairs = names_good & keep[:, None]
    assert (less[pairs] >= 0).all() and (tied[pairs] >= 0).all()
    assert (less[~pairs] == -1).all() and (tied[~pairs] == -1).all()


# ------------------------------------------------------------------ (d) the softmax vote
@pytest.mark.parametrize("kind", list(E.VOTE_RANGES))
def test_softmax_vote_at_latent_width_distances(kind):
    from vit_som_amd import ops
    c = E.vote_case(kind)
    inp, ref = c.inp, c.ref
    idx, dist, labels = inp["idx"].to(DEV), inp["dist"].to(DEV), inp["labels"].to(DEV)
    pred = torch.full((E.VOTE_NQ,), -5, dtype=torch.int64, device=DEV)
    scores = torch.full((E.VOTE_NQ, E.VOTE_CLASSES), -5.0, dtype=torch.float64, device=DEV)
    status = torch.zeros(2, dtype=torch.int32, device=DEV)
    ops.knn_vote(idx, dist, labels, E.VOTE_CLASSES, R.SOFTMAX, E.VOTE_T, pred, status, scores)
    pred, scores = pred.cpu(), scores.cpu()
    assert status.tolist() == [0, 0]
    assert (scores.sum(1) > 0).all() and (scores.max(1).values >= 1.0).all()      # no query is decided by an all-zero row
    e = c.metric["scores"](scores / scores.sum(1, keepdim=True), ref["scores"])
    _record(c.name, "scores", e, c.e32["scores"], E.FLOOR["vote"])
    assert e <= E.FLOOR["vote"]                                       # fp64 arithmetic: the floor itself, not the fp32 bound
    assert torch.equal(pred[inp["clear"]], ref["pred"][inp["clear"]])


# ------------------------------------------------------------------ (e) k-means
def _one_iteration(X, C):
    from vit_som_amd import ops
    N, D = X.shape
    k = C.shape[0]
    ws = torch.empty(ops.kmeans_workspace_bytes(N, D, k), dtype=torch.uint8, device=DEV)
    prev = torch.full((N,), -1, dtype=torch.int64, device=DEV)
    labels = torch.empty(N, dtype=torch.int64, device=DEV)
    mind = torch.empty(N, dtype=torch.float32, device=DEV)
    cnew = torch.empty(k, D, dtype=torch.float32, device=DEV)
    counts = torch.empty(k, dtype=torch.int64, device=DEV)
    status = torch.empty(4, dtype=torch.float64, device=DEV)
    ops.kmeans_assign(X, C, labels, prev, mind, ws)
    ops.kmeans_update(C, cnew, N, mind, counts, status, ws)
    torch.cuda.synchronize()
    return labels.cpu(), mind.cpu(), cnew.cpu(), counts.cpu(), status.cpu()


@pytest.mark.parametrize("i", range(len(E.KMEANS_SHAPES)))
def test_kmeans_at_an_offset(i):
    from vit_som_amd import ops
    c = E.kmeans_case(i, "offset")
    inp, ref = c.inp, c.ref
    N, D, k = E.KMEANS_SHAPES[i]
    X, C = inp["X"].to(DEV), inp["C"].to(DEV)
    labels, mind, _, _, status = _one_iteration(X, C)
    floor = E.FLOOR["kmeans"]
    own = ref["d"].gather(1, labels[:, None]).squeeze(1)              # fp64, to the centre the kernel chose
    e = {"mind": c.metric["mind"](mind, own)}
    T = inp["cand"].numel()
    dist = torch.full((T, N), math.nan, device=DEV)
    pots = torch.full((T,), math.nan, dtype=torch.float64, device=DEV)
    ops.kmeanspp_dist(X, inp["cand"].to(DEV), inp["closest"].to(DEV), dist, pots)
    e["pp"], e["pots"] = c.metric["pp"](dist.cpu(), ref["pp"]), c.metric["pots"](pots.cpu(), ref["pots"])
    var = torch.full((1,), math.nan, dtype=torch.float64, device=DEV)
    ws = torch.empty(ops.kmeans_workspace_bytes(N, D, k), dtype=torch.uint8, device=DEV)
    ops.kmeans_colvar(X, k, var, ws)
    e["colvar"] = c.metric["colvar"](var.cpu(), ref["colvar"])
    bounds = {out: _record(c.name, out, e[out], c.e32[out], floor) for out in e}
    e_inertia = abs(float(status[3]) - float(own.sum())) / float(own.sum())
    _record(c.name, "inertia", e_inertia, c.e32["pots"], floor)
    for out in e:
        assert e[out] <= bounds[out], (out, e[out], bounds[out])
    assert e_inertia <= E.bound(floor, c.e32["pots"])
    clear = inp["clear"]
    assert torch.equal(labels[clear], ref["labels"][clear]), int((labels[clear] != ref["labels"][clear]).sum())


@pytest.mark.parametrize("kind", ["nan", "overflow"])
@pytest.mark.parametrize("i", range(len(E.KMEANS_SHAPES)))
def test_kmeans_bad_rows_touch_nothing_else(i, kind):
    """With a bad row in the first workgroup's range and one in the last's: the labels and mind of every other row, and the
    centres and counts of the clusters the bad rows joined in neither run, are bit for bit those of the run on good rows;
    KMeans.fit refuses the set, naming the count."""
    from vit_som_amd import KMeans
    c = E.kmeans_case(i, kind)
    inp = c.inp
    C = inp["C"].to(DEV)
    labels, mind, cnew, counts, status = _one_iteration(inp["X"].to(DEV), C)
    labels0, mind0, cnew0, counts0, status0 = _one_iteration(inp["X_good"].to(DEV), C)
    bad = inp["bad"]
    others = torch.ones(labels.numel(), dtype=torch.bool)
    others[bad] = False
    assert torch.equal(labels[others], labels0[others]) and E.bits_equal(mind[others], mind0[others])
    assert not torch.isfinite(mind[bad]).any() and not math.isfinite(float(status[3])) and math.isfinite(float(status0[3]))
    untouched = torch.ones(C.shape[0], dtype=torch.bool)
    untouched[labels[bad]] = False
    untouched[labels0[bad]] = False
    assert untouched.sum() >= C.shape[0] - 2 * len(bad) and untouched.any()
    assert torch.equal(counts[untouched], counts0[untouched]) and E.bits_equal(cnew[untouched], cnew0[untouched])
    with pytest.raises(ValueError, match=f"{len(bad)} rows"):
        KMeans(C.shape[0], init=inp["C"].numpy(), max_iter=3).fit(inp["X"].to(DEV))
    with pytest.raises(ValueError, match=f"{len(bad)} rows"):
        KMeans(C.shape[0], n_init=1, max_iter=3).fit(inp["X"].to(DEV))


# ------------------------------------------------------------------ (f) the linear probe's residual
@pytest.mark.parametrize("kind", E.CE_KINDS)
@pytest.mark.parametrize("C", E.PROBE_CLASSES)
def test_probe_residual_on_saturated_logits(C, kind):
    from vit_som_amd import ops
    c = E.probe_case(C, kind)
    inp, ref = c.inp, c.ref
    N = inp["Z"].shape[0]
    Rd = torch.full((N, C), math.nan, device=DEV)
    loss = torch.full((1,), math.nan, dtype=torch.float64, device=DEV)
    gb = torch.full((C,), math.nan, dtype=torch.float64, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    pred = torch.full((N,), -7, dtype=torch.int64, device=DEV)
    ops.probe_residual(inp["Z"].to(DEV), inp["b"].to(DEV), inp["y"].to(DEV), Rd, loss, gb, status, pred)
    assert int(status) == 0
    e_R, e_loss = c.metric["R"](Rd.cpu(), ref["R"]), c.metric["loss"](loss.cpu(), ref["loss"])
    b_R = _record(c.name, "R", e_R, c.e32["R"], E.FLOOR["probe_R"])
    _record(c.name, "loss", e_loss, c.e32["loss"], E.FLOOR["probe_loss"])
    assert e_R <= b_R
    assert e_loss <= E.FLOOR["probe_loss"]                            # an fp64 sum: the floor itself, not the fp32 bound
    assert torch.equal(pred.cpu(), ref["pred"])
    assert np.abs(gb.cpu().numpy() - Rd.cpu().double().sum(0).numpy()).max() <= 1e-12 * N
