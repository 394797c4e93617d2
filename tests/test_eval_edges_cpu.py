"""The edge cases of the evaluation kernels (eval_edges.py), checked on the CPU: every case has its property, in fp64; every
fp32 yardstick is good enough to bound a kernel (e32 <= E32_MAX); wherever indices are compared one by one, fp64 alone
leaves at least half the rows clear; and the comparisons the GPU suite makes have teeth -- the kNN distance with the clamp
that swallows a NaN, the vote with the unshifted exponential and the k-means distance in the fp32 expansion form, fed to the
same checks, are all rejected, while the formulations the kernels document pass."""
import pytest
import torch

import eval_edges as E
import knn_checks as KC

SEARCH_BAD = [("knn", s, kind, m) for s in E.KNN_SHAPES for kind in E.BAD_KINDS for m in E.METRICS] + \
             [("umap", None, kind, m) for kind in E.BAD_KINDS for m in E.METRICS]


def _search_bad(which, shape, kind, metric):
    return E.knn_bad_case(shape, kind, metric) if which == "knn" else E.umap_bad_case(kind, metric)


def _all_cases():
    for spec in SEARCH_BAD:
        yield _search_bad(*spec)
    for self_mode in (False, True):
        for m in E.METRICS:
            yield E.offset_dup_case(m, self_mode)
        yield E.pow2_case(self_mode)
    for kind in E.BAD_KINDS:
        yield E.ranks_case(kind)
    for kind in E.VOTE_RANGES:
        yield E.vote_case(kind)
    for i in range(len(E.KMEANS_SHAPES)):
        for kind in E.KMEANS_KINDS:
            yield E.kmeans_case(i, kind)
    for C in E.PROBE_CLASSES:
        for kind in E.CE_KINDS:
            yield E.probe_case(C, kind)


def test_every_case_has_its_property_and_a_usable_yardstick():
    n = 0
    for c in _all_cases():
        assert c.prop and all(c.prop.values()), (c.name, c.prop)
        for out, e in c.e32.items():
            assert e <= E.E32_MAX, (c.name, out, e)                   # NaN fails too
        n += 1
    assert n == 24 + 6 + 4 + 2 + 6 + 8


def test_fp64_alone_leaves_half_the_rows_clear():
    """The cap of test_query_against_fp64, a condition on the inputs: where the GPU suite compares index by index (the good
    rows of the bad-row cases, the k-means labels at an offset) at least half the rows are clear."""
    for spec in SEARCH_BAD:
        c = _search_bad(*spec)
        assert c.clear_share >= 0.5, (c.name, c.clear_share)
    for i in range(len(E.KMEANS_SHAPES)):
        c = E.kmeans_case(i, "offset")
        assert c.clear_share >= 0.5, (c.name, c.clear_share)
    for kind in E.VOTE_RANGES:
        assert float(E.vote_case(kind).inp["clear"].double().mean()) >= 0.5


# ------------------------------------------------------------------ the distance clamp
def _restated(c, **kw):
    inp = c.inp
    full = E.restated_search(inp["Q"], inp["X"], inp["k"], inp["metric"], inp["self_mode"], **kw)
    deleted = E.restated_search(inp["Qg"], inp["Xk"], inp["k"], inp["metric"], inp["self_mode"], **kw)
    return full, deleted


@pytest.mark.parametrize("which,shape,kind,metric", SEARCH_BAD)
def test_the_bad_row_contract_rejects_the_clamp_that_swallows_a_nan(which, shape, kind, metric):
    """knn_distance restated in fp32: with the test for a pair without a distance before the clamps the contract holds and
    the good rows pass the fp64 checks; with fmaxf(NaN, 0) = 0 and no test (the kernel before the fix) it is broken."""
    c = _search_bad(which, shape, kind, metric)
    (idx, dist), (idx_del, dist_del) = _restated(c)
    assert E.bad_row_contract(idx, dist, idx_del, dist_del, c.inp) == []
    tol = E.bound(E.FLOOR["knn"], c.e32["d"])
    share, _ = KC.lists_against_fp64(idx_del, dist_del, c.inp["Qg"], c.inp["Xk"], c.inp["k"], metric, tol=tol)
    assert share >= 0.5
    (idx, dist), (idx_del, dist_del) = _restated(c, clamp_swallows_nan=True)
    broken = E.bad_row_contract(idx, dist, idx_del, dist_del, c.inp)
    assert any("bad bank row is listed" in b for b in broken) and any("bad query" in b for b in broken), broken
    # an overflowed norm against a finite row answers sqrt(inf) or 1 - x / inf = 1, not 0: such a row enters only the lists
    # of the bad queries (with a non-finite distance)
    if kind != "overflow":
        assert any("differs from the call" in b for b in broken), broken


@pytest.mark.parametrize("self_mode", [False, True])
@pytest.mark.parametrize("metric", E.METRICS)
def test_offset_dup_checks_on_the_restatement(metric, self_mode):
    c = E.offset_dup_case(metric, self_mode)
    idx, dist = E.restated_search(c.inp["Q"], c.inp["X"], c.inp["k"], metric, self_mode)
    broken, together = E.offset_dup_violations(idx, dist, c.inp)
    assert broken == [] and together > 0
    # a search that breaks ties by the HIGHER index is caught
    flipped = idx.clone()
    q, _ = c.inp["copies"][0]
    a = 1 if self_mode else 0
    flipped[q, a], flipped[q, a + 1] = idx[q, a + 1], idx[q, a]
    assert E.offset_dup_violations(flipped, dist, c.inp)[0]


@pytest.mark.parametrize("self_mode", [False, True])
def test_pow2_restatement_is_bitwise_invariant(self_mode):
    c = E.pow2_case(self_mode)
    scaled = E.restated_search(c.inp["Q"], c.inp["X"], c.inp["k"], "cosine", self_mode)
    plain = E.restated_search(c.inp["Q0"], c.inp["X0"], c.inp["k"], "cosine", self_mode)
    assert torch.equal(scaled[0], plain[0]) and E.bits_equal(scaled[1], plain[1])


# ------------------------------------------------------------------ the unshifted vote
@pytest.mark.parametrize("kind", list(E.VOTE_RANGES))
def test_the_vote_check_rejects_the_unshifted_exponential(kind):
    c = E.vote_case(kind)
    inp, ref = c.inp, c.ref
    floor = E.FLOOR["vote"]
    shifted64, _ = E.vote_eval(inp["idx"], inp["dist"], inp["labels"], E.VOTE_T, torch.float64)
    assert E.accepts(c.metric["scores"](shifted64, ref["scores"]), floor, 0.0)
    plain, raw = E.vote_eval(inp["idx"], inp["dist"], inp["labels"], E.VOTE_T, torch.float64, shift=False)
    e = c.metric["scores"](plain, ref["scores"])
    clear = inp["clear"]
    if kind == "euclidean_range":
        # every weight underflows: 0 / 0 scores, and the first argmax of an all-zero row is class 0
        assert not E.accepts(e, floor, c.e32["scores"])
        assert bool((raw == 0).all()) and not torch.equal(raw.argmax(1)[clear], ref["pred"][clear])
    else:
        assert E.accepts(e, floor, 0.0) and torch.equal(raw.argmax(1)[clear], ref["pred"][clear])     # the control: both forms agree


# ------------------------------------------------------------------ the k-means expansion form
@pytest.mark.parametrize("i", range(len(E.KMEANS_SHAPES)))
def test_the_kmeans_check_rejects_the_expansion_form(i):
    c = E.kmeans_case(i, "offset")
    inp, ref = c.inp, c.ref
    clear = inp["clear"]

    def verdict(expansion):
        out = E.kmeans_eval(inp["X_good"], inp["C"], inp["cand"], inp["closest"], torch.float32, expansion=expansion)
        lab, mind, _ = E.kmeans_labels(out["d"])
        own = ref["d"].gather(1, lab[:, None]).squeeze(1)            # the fp64 distance to the centre this form chose
        e = c.metric["mind"](mind, own)
        return E.accepts(e, E.FLOOR["kmeans"], c.e32["mind"]), bool(torch.equal(lab[clear], ref["labels"][clear])), e
    ok, same, e = verdict(False)
    assert ok and same, e
    ok, same, e = verdict(True)
    print(f"{c.name}: the expansion form is off by {e:.3e} against a bound of {E.bound(E.FLOOR['kmeans'], c.e32['mind']):.3e}")
    assert not ok or not same
