"""t-SNE on the device (tsne.hip, tsne.py) against the fp64 numpy restatement of tsne_ref.py: the affinities, the exact
repulsion, one step, a short trajectory, a whole fit held to the band the restatement itself spans, and the evaluation
entries on a tiny ViTSOM.

The yardstick for float32 results is the project's: error <= 4 * max(e32, 2^-23 * largest magnitude), e32 being the error
of the same computation done in plain float32 torch on the CPU."""
import copy
import json
import os

import numpy as np
import pytest
import torch

import memcheck as MC
import tsne_ref as R
from test_tsne_cpu import AFFINITY_CASES, affinity_rows

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U23 = 2.0 ** -23


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _yardstick(what, got, ref, plain32):
    """got, ref, plain32: arrays of one shape; ref in float64."""
    got, ref, plain32 = (np.asarray(a, dtype=np.float64) for a in (got, ref, plain32))
    mag = np.abs(ref).max()
    err, e32 = np.abs(got - ref).max(), np.abs(plain32 - ref).max()
    print(f"{what}: error {err:.3e}, e32 {e32:.3e}, largest magnitude {mag:.3e}, bound {4 * max(e32, U23 * mag):.3e}")
    assert err <= 4.0 * max(e32, U23 * mag), what


# ------------------------------------------------------------------ 4. affinities
def _table(N, k, seed, metric):
    """A neighbour table laid out as vsom_umap_knn leaves it (the row itself first at distance 0), from the fp64 search of
    the restatement: the very distances test_tsne_cpu.py checks for their margin to the tolerance."""
    X = affinity_rows(N, seed)
    idx, dist = R.exact_knn(X, k, metric)
    idx = np.concatenate([np.arange(N, dtype=np.int64)[:, None], idx], axis=1)
    dist = np.concatenate([np.zeros((N, 1), dtype=np.float32), dist], axis=1)
    return idx, dist


@pytest.mark.parametrize("metric", ["euclidean", "cosine"])
@pytest.mark.parametrize("N,k,perplexity,seed", AFFINITY_CASES)
def test_affinities_follow_the_bisection(N, k, perplexity, seed, metric):
    from vit_som_amd import ops
    idx, dist = _table(N, k, seed, metric)
    square = metric == "euclidean"
    d = R.squared_f32(dist[:, 1:]) if square else dist[:, 1:]
    betas, _, stop = R.bisection_trace(d, perplexity)
    dist_d, dist_h = MC.guarded_copy(_dev(dist))
    idx_d, idx_h = MC.guarded_copy(_dev(idx))
    P, Ph = MC.guarded((N, k), torch.float64, DEV)
    beta, bh = MC.guarded((N,), torch.float64, DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.tsne_affinities(dist_d, perplexity, P, beta, status, knn_idx=idx_d, first=1, square=square)
    assert int(status.item()) == 0
    for h in (Ph, bh):
        h.check(); h.all_written()
    dist_h.check(); idx_h.check()
    Pg, bg = P.cpu().numpy(), beta.cpu().numpy()
    assert np.abs(R.row_sums(Pg) - 1.0).max() <= 1e-12
    cols = np.arange(N)
    moved = 0
    for i in range(N):
        for t in (stop[i], stop[i] - 1, stop[i] + 1):
            if 0 <= t < R.N_STEPS and abs(bg[i] - betas[t, i]) <= 1e-12 * betas[t, i]:
                break
        else:
            raise AssertionError(f"row {i}: beta {bg[i]!r} is none of the iterates {betas[max(stop[i] - 1, 0):stop[i] + 2, i]} "
                                 f"around its stop at step {stop[i]}")
        moved += t != stop[i]
    want = R.conditional_p_at(d, bg)                          # the restated P at the iterate the device stopped at
    err = (np.abs(Pg - want) / want.max(axis=1, keepdims=True)).max()
    print(f"{metric} N={N} k={k}: {moved} rows stopped a step early or late, P error {err:.3e} of the row maximum, "
          f"stops {stop.min()}..{stop.max()}")
    assert err <= 1e-12
    assert moved <= 0.01 * N
    assert (d[17, :2] <= 1e-5).all()                          # the duplicates of row 17 lead its list
    # two calls, the same bits
    P2, beta2 = torch.empty_like(P), torch.empty_like(beta)
    ops.tsne_affinities(dist_d, perplexity, P2, beta2, status, knn_idx=idx_d, first=1, square=square)
    assert torch.equal(P2, P) and torch.equal(beta2, beta)


def test_affinities_count_bad_rows_and_leave_the_others_alone():
    from vit_som_amd import ops
    N, k, perplexity, seed = AFFINITY_CASES[1]
    idx, dist = _table(N, k, seed, "euclidean")
    clean = torch.empty(N, k, dtype=torch.float64, device=DEV), torch.empty(N, dtype=torch.float64, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.tsne_affinities(_dev(dist), perplexity, clean[0], clean[1], status, knn_idx=_dev(idx))
    bad_dist, bad_idx = dist.copy(), idx.copy()
    bad_dist[3, 5] = np.nan
    bad_idx[7, k] = -1                                        # an empty slot at the end of the list
    bad_dist[9, 2] = -1.0
    bad_dist[200, 1] = np.inf
    bad_dist[201, 60] = 3e19                                  # finite, its square is not
    bad_dist[11, 0] = np.nan                                  # the self slot is skipped: not a bad row
    bad = [3, 7, 9, 200, 201]
    P, Ph = MC.guarded((N, k), torch.float64, DEV)
    beta, bh = MC.guarded((N,), torch.float64, DEV)
    poison_P, poison_b = P.clone(), beta.clone()
    ops.tsne_affinities(_dev(bad_dist), perplexity, P, beta, status, knn_idx=_dev(bad_idx))
    assert int(status.item()) == len(bad)
    Ph.check(); bh.check()
    good = np.setdiff1d(np.arange(N), bad)
    gi, bi = _dev(good), _dev(np.array(bad))
    assert torch.equal(P[gi], clean[0][gi]) and torch.equal(beta[gi], clean[1][gi])
    assert torch.equal(P[bi].view(torch.int64), poison_P[bi].view(torch.int64))          # not written: still the poison
    assert torch.equal(beta[bi].view(torch.int64), poison_b[bi].view(torch.int64))


# ------------------------------------------------------------------ 5. repulsion
KINDS = ("initial", "late", "coincident", "two_clusters", "offset")


def _embedding(kind, N, seed):
    rs = np.random.RandomState(seed)
    z = rs.standard_normal((N, 2))
    if kind == "initial":
        Y = 1e-4 * z                                          # every q ~ 1, Z ~ N^2
    elif kind == "late":
        Y = 30.0 * z
    elif kind == "coincident":
        Y = np.full((N, 2), 0.375)                            # force exactly 0, Z = N (N - 1) exactly
    elif kind == "two_clusters":
        Y = z + np.where(np.arange(N)[:, None] % 2 == 0, 0.0, 1e4)
    else:
        Y = z + 1000.0                                        # the subtraction must come before the squaring
    return Y.astype(np.float32)


def _pairs(Yrows, Yall, first_row, dtype):
    """(sum_j q^2 (y_i - y_j) [n, 2], sum_j q [n]) over all j != i for rows [first_row, first_row + n) in torch at `dtype`."""
    dx = Yrows[:, 0:1].to(dtype) - Yall[:, 0].to(dtype)[None, :]
    dy = Yrows[:, 1:2].to(dtype) - Yall[:, 1].to(dtype)[None, :]
    q = 1.0 / (1.0 + (dx * dx + dy * dy))
    r = torch.arange(Yrows.shape[0], device=Yrows.device)
    q[r, r + first_row] = 0.0
    q2 = q * q
    return torch.stack([(q2 * dx).sum(1), (q2 * dy).sum(1)], dim=1), q.sum(1)


def _repulsion_fp64(Y):
    """The reference for all rows: float64 torch on the device, in row blocks (memory)."""
    reps, sums = [], []
    for b in range(0, Y.shape[0], 1024):
        r, s = _pairs(Y[b:b + 1024], Y, b, torch.float64)
        reps.append(r); sums.append(s)
    return torch.cat(reps).cpu().numpy(), torch.cat(sums).cpu().numpy()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("N", [2, 63, 64, 65, 257, 3000, 20011])
def test_repulsion_against_fp64(N, kind):
    from vit_som_amd import ops
    Yh = _embedding(kind, N, 1000 + N)
    Y, Yguard = MC.guarded_copy(_dev(Yh))
    rep, rh = MC.guarded((N, 2), torch.float64, DEV)
    sumq, sh = MC.guarded((N,), torch.float64, DEV)
    zpart, zh = MC.guarded((ops.tsne_repulsion_parts(N),), torch.float64, DEV)      # exactly the size of the query
    ops.tsne_repulsion(Y, rep, sumq, zpart)
    for h in (rh, sh, zh):
        h.check(); h.all_written()
    Yguard.check()
    rep_g, sum_g, Z = rep.cpu().numpy(), sumq.cpu().numpy(), float(zpart.sum().item())
    assert np.isfinite(rep_g).all() and np.isfinite(sum_g).all()
    # zpart is the sum of sumq over blocks of 64 rows in ascending row order
    for b in (0, (N - 1) // 64):
        z = 0.0
        for v in sum_g[64 * b:64 * b + 64]:
            z += v
        assert z == float(zpart[b].item())
    if kind == "coincident":
        assert not rep_g.any() and (sum_g == N - 1).all() and Z == N * (N - 1)
    else:
        rep_r, sum_r = _repulsion_fp64(Y)
        # e32 on the CPU: all rows up to 3 000, 512 rows spread over the set beyond
        rows = np.arange(N) if N <= 3000 else np.unique(np.linspace(0, N - 1, 512).astype(np.int64))
        Yc = torch.from_numpy(Yh)
        r32 = [(_pairs(Yc[i:i + 1], Yc, int(i), torch.float32)) for i in rows] if N > 3000 else None
        if r32 is None:
            rep32, sum32 = _pairs(Yc, Yc, 0, torch.float32)
        else:
            rep32, sum32 = torch.cat([r for r, _ in r32]), torch.cat([s for _, s in r32])
        _yardstick(f"{kind} N={N} forces", rep_g[rows], rep_r[rows], rep32.numpy())
        _yardstick(f"{kind} N={N} row sums of q", sum_g[rows], sum_r[rows], sum32.numpy())
        Zr = float(np.sum(sum_r))
        bound = 71 * 2.0 ** -24 + N * 2.0 ** -53              # include/vitsom_hip.h, vsom_tsne_repulsion
        print(f"{kind} N={N}: Z {Z:.9e}, relative error {abs(Z - Zr) / Zr:.3e}, bound {bound:.3e}")
        assert abs(Z - Zr) <= bound * Zr
    rep2, sumq2, zpart2 = torch.empty_like(rep), torch.empty_like(sumq), torch.empty_like(zpart)
    ops.tsne_repulsion(Y, rep2, sumq2, zpart2)
    assert torch.equal(rep2, rep) and torch.equal(sumq2, sumq) and torch.equal(zpart2, zpart)


# ------------------------------------------------------------------ 6. one step
_P_CACHE = {}


def _joint_p(N):
    """The joint P of clustered rows through the restatement's affinities and the product's host graph (computed once)."""
    if N not in _P_CACHE:
        from vit_som_amd.tsne import joint_probabilities
        X, _ = R.blobs(N, 16, 5, 40 + N, scale=3.0)
        idx, dist = R.exact_knn(X, 63, "euclidean")
        P = joint_probabilities(idx, R.conditional_p(R.squared_f32(dist), 20.0)[0])
        _P_CACHE[N] = (P, np.asarray(P.todense()))
    return _P_CACHE[N]


def _grad_f32(Pd, Y, exaggeration):
    """The gradient in plain float32 torch on the CPU."""
    Yc = torch.from_numpy(Y)
    P32 = torch.from_numpy((Pd * exaggeration).astype(np.float32))
    dx = Yc[:, 0:1] - Yc[:, 0][None, :]
    dy = Yc[:, 1:2] - Yc[:, 1][None, :]
    q = 1.0 / (1.0 + (dx * dx + dy * dy))
    q.fill_diagonal_(0.0)
    Z = q.sum()
    pq, q2 = P32 * q, q * q
    g = 4.0 * torch.stack([(pq * dx).sum(1) - (q2 * dx).sum(1) / Z, (pq * dy).sum(1) - (q2 * dy).sum(1) / Z], dim=1)
    return g.numpy().astype(np.float64)


def _device_step(P, Y, update, gains, exaggeration, momentum, lr):
    from vit_som_amd import ops
    from vit_som_amd.tsne import _Graph, read_record
    N = Y.shape[0]
    g = _Graph(P, DEV)
    Yin, Yin_h = MC.guarded_copy(_dev(Y))
    Yout, Yout_h = MC.guarded((N, 2), torch.float32, DEV)
    upd, upd_h = MC.guarded_copy(_dev(update))
    gn, gn_h = MC.guarded_copy(_dev(gains))
    part, part_h = MC.guarded((ops.tsne_step_parts(N),), torch.float64, DEV)
    ops.tsne_repulsion(Yin, g.rep, g.sumq, g.zpart)
    ops.tsne_step(g.indptr, g.indices, g.data, Yin, Yout, upd, gn, g.rep, g.zpart, exaggeration, momentum, lr, part, record=True)
    for h in (Yin_h, Yout_h, upd_h, gn_h, part_h):
        h.check()
    Yout_h.all_written(); part_h.all_written()
    assert torch.equal(Yin.cpu(), torch.from_numpy(Y))
    kl, gnorm = read_record(part)
    return Yout.cpu().numpy(), upd.cpu().numpy(), gn.cpu().numpy(), kl, gnorm


@pytest.mark.parametrize("N", [257, 3000])
def test_step_against_the_restatement(N):
    P, Pd = _joint_p(N)
    rs = np.random.RandomState(N)
    Y = (3.0 * rs.standard_normal((N, 2))).astype(np.float32)
    lr, momentum = 200.0, 0.8
    for exaggeration in (12.0, 1.0):
        kl_r, grad = R.kl_and_grad(Pd, Y, exaggeration)
        scale = np.abs(grad).max()
        update = (rs.standard_normal((N, 2)) * lr * scale).astype(np.float32)          # both signs, the size of a real update
        gains = rs.uniform(0.005, 2.0, size=(N, 2)).astype(np.float32)                 # some below the floor, some that fall below it
        gains[::7] = np.float32(0.0115)                                              # 0.8 x this is under the floor
        Y_r, u_r, g_r = R.update_step(Y, update, gains, grad, momentum, lr)
        Y_32, u_32, g_32 = R.update_step(Y, update, gains, _grad_f32(Pd, Y, exaggeration), momentum, lr)
        Y_d, u_d, g_d, kl_d, gn_d = _device_step(P, Y, update, gains, exaggeration, momentum, lr)
        _yardstick(f"N={N} exaggeration {exaggeration}: Y_out", Y_d, Y_r, Y_32)
        _yardstick(f"N={N} exaggeration {exaggeration}: update", u_d, u_r, u_32)
        sure = np.abs(update.astype(np.float64) * grad) >= 1e-30
        assert np.array_equal(g_d[sure], g_r[sure]) and (g_d >= np.float32(0.01)).all()
        _yardstick(f"N={N} exaggeration {exaggeration}: gains", g_d, g_r, g_32)
        gn_r = float(np.sqrt((grad * grad).sum()))
        print(f"N={N} exaggeration {exaggeration}: KL {kl_d:.12f} against {kl_r:.12f}, |grad| {gn_d:.9e} against {gn_r:.9e}")
        assert abs(kl_d - kl_r) <= 1e-6 * abs(kl_r) and abs(gn_d - gn_r) <= 1e-6 * gn_r
    # the exaggeration is honoured: the two KLs differ as the restatement's do
    assert kl_d != pytest.approx(R.kl_and_grad(Pd, Y, 12.0)[0], rel=1e-3)


# ------------------------------------------------------------------ 7. short trajectory
def _trajectory_case():
    """257 clustered rows on the device, their joint P as the estimator makes it, and the PCA init scaled by 1.0."""
    from vit_som_amd import PCA, TSNE
    Xh, _ = R.blobs(257, 16, 5, 77, scale=3.0)
    X = _dev(Xh)
    est = TSNE(perplexity=20.0)
    P = est.affinities(X, est._validate(257))
    E = PCA(n_components=2, random_state=0).fit_transform(X).cpu().numpy().astype(np.float32)
    Y0 = (E / np.std(E[:, 0])).astype(np.float32)             # sklearn's init without the 1e-4: the forces matter at once
    return X, est, P, Y0


def test_estimator_affinities_match_the_restatement_on_the_device_table():
    """Steps 1-3 through the device search: the restated bisection on the table the device found gives the same joint P."""
    _, est, P, _ = _trajectory_case()
    want = R.joint_p(est._knn_indices, R.conditional_p(R.squared_f32(est._knn_dists), 20.0)[0])
    got = np.asarray(P.todense())
    assert np.array_equal(got, got.T) and abs(got.sum() - 1.0) <= 1e-14
    assert np.abs(got - want).max() <= 1e-9 * want.max()      # a row may stop a step apart: |dP| <= 1e-5-ish of the gap, not of P
    assert (est._betas > 0).all() and est._knn_indices.shape == (257, 60)      # floor(3 x 20)


def test_small_set_takes_every_other_row_as_a_neighbour():
    """k = N - 1: the leave-one-out search, no self slot; the same affinities as the restatement gives on that table."""
    from vit_som_amd import TSNE
    Xh, _ = R.blobs(20, 8, 2, 5, scale=2.0)
    est = TSNE(perplexity=8.0)
    k = est._validate(20)
    assert k == 19
    P = est.affinities(_dev(Xh), k)
    assert est._knn_indices.shape == (20, 19)
    assert all(sorted(row.tolist()) == [j for j in range(20) if j != i] for i, row in enumerate(est._knn_indices))
    want = R.joint_p(est._knn_indices, R.conditional_p(R.squared_f32(est._knn_dists), 8.0)[0])
    assert np.abs(np.asarray(P.todense()) - want).max() <= 1e-9 * want.max()
    ref_idx, ref_dist = R.exact_knn(Xh, 19, "euclidean")
    assert np.abs(est._knn_dists - ref_dist).max() <= 1e-4 * ref_dist.max()


@pytest.mark.parametrize("N,perplexity,refused", [(20, 8.0, 20), (257, 5.0, 2)])
def test_fit_refuses_a_row_that_is_not_finite(N, perplexity, refused):
    """Both searches leave such a row without neighbours and list it for nobody; the affinities count every row whose list
    is incomplete and fit raises before anything is fitted.  At k = N - 1 the two bad rows leave EVERY list short."""
    from vit_som_amd import TSNE
    Xh, _ = R.blobs(N, 8, 2, 6, scale=2.0)
    Xh[3, 2] = np.nan
    Xh[7, 0] = np.inf
    est = TSNE(perplexity=perplexity)
    with pytest.raises(ValueError, match=f"{refused} rows have no complete list"):
        est.fit(_dev(Xh))
    assert not hasattr(est, "embedding_")


def test_short_trajectory_and_its_cuts(monkeypatch):
    from vit_som_amd import TSNE, ops
    from vit_som_amd.tsne import _Graph, descend
    es = MC.ExactScratch()
    monkeypatch.setattr(ops, "scratch", es)
    X, est, P, Y0 = _trajectory_case()
    lr, exag, mom, n = 50.0, 12.0, 0.5, 20
    graph = _Graph(P, DEV)

    def run(cuts):
        Y, upd, gn = _dev(Y0.copy()), torch.zeros(257, 2, device=DEV), torch.ones(257, 2, device=DEV)
        for b, e in zip(cuts[:-1], cuts[1:]):
            Y, last, stopped = descend(graph, Y, upd, gn, b, e, n, exag, mom, lr)
            assert last == e - 1 and not stopped
        return Y.clone(), upd, gn
    whole, cut = run([0, n]), run([0, 8, n])
    for a, b in zip(whole, cut):
        assert torch.equal(a, b)
    es.check()
    Pd = np.asarray(P.todense())
    Y_r = R.run(Pd, Y0.copy(), n, lr, exag, mom)[0]
    Y_32, u32, g32 = Y0.copy(), np.zeros_like(Y0), np.ones_like(Y0)
    for _ in range(n):                                        # the same trajectory with the gradient in plain float32
        Y_32, u32, g32 = R.update_step(Y_32, u32, g32, _grad_f32(Pd, Y_32, exag), mom, lr)
    _yardstick("20 iterations at N=257", whole[0].cpu().numpy(), Y_r, Y_32)
    # two fits, the same bits; a fit of 20 iterations is that trajectory
    fits = [TSNE(perplexity=20.0, max_iter=n, learning_rate=lr, init=_dev(Y0)).fit(X) for _ in range(2)]
    assert torch.equal(fits[0].embedding_, fits[1].embedding_) and fits[0].kl_divergence_ == fits[1].kl_divergence_
    assert torch.equal(fits[0].embedding_, whole[0]) and fits[0].n_iter_ == n - 1 and fits[0].learning_rate_ == lr
    assert fits[0].n_features_in_ == 16


# ------------------------------------------------------------------ 8. whole fit
@pytest.mark.parametrize("metric", ["euclidean", "cosine"])
def test_whole_fit_lands_in_the_band_of_the_restatement(metric, monkeypatch):
    import vit_som_amd
    from vit_som_amd import tsne
    band = json.load(open(os.path.join(ROOT, "tests", "golden", "tsne_fit_band.json")))
    Xh, _ = R.blobs(band["N"], band["D"], band["centres"], band["data_seed"])
    idx, dist = R.exact_knn(Xh, 63, metric)
    Pr = R.joint_p(idx, R.conditional_p(R.squared_f32(dist) if metric == "euclidean" else dist, band["perplexity"])[0])
    reads = []
    real = tsne.read_record
    monkeypatch.setattr(tsne, "read_record", lambda part: reads.append(real(part)) or reads[-1])
    X = _dev(Xh)
    est = vit_som_amd.TSNE(perplexity=band["perplexity"], metric=metric, max_iter=band["max_iter"], random_state=0)
    emb = est.fit_transform(X)
    assert emb.shape == (band["N"], 2) and emb.dtype == torch.float32 and bool(torch.isfinite(emb).all())
    assert est.n_iter_ <= band["max_iter"] - 1 and est.learning_rate_ == 50.0 and est.n_features_in_ == band["D"]
    assert est.kl_divergence_ == reads[-1][0]                 # the record's last check
    assert len(reads) == (est.n_iter_ + 1) // 50              # one read per 50 iterations: the only synchronisations
    kl = R.kl_and_grad(Pr, emb.cpu().numpy())[0]              # recomputed in fp64 against the restatement's own P
    trust = vit_som_amd.trustworthiness(X, emb.contiguous(), n_neighbors=band["n_neighbors"], metric=metric)
    runs = band["runs"][metric]
    kl_lo, kl_hi = min(runs["kl"]), max(runs["kl"])
    t_lo, t_hi = min(runs["trustworthiness"]), max(runs["trustworthiness"])
    print(f"{metric}: KL {kl:.4f} (reported {est.kl_divergence_:.4f}; band {kl_lo:.4f} .. {kl_hi:.4f}), trustworthiness {trust:.4f} "
          f"(band {t_lo:.4f} .. {t_hi:.4f}), {est.n_iter_ + 1} iterations")
    assert kl <= kl_hi + (kl_hi - kl_lo)
    assert trust >= t_lo - (t_hi - t_lo)
    assert abs(est.kl_divergence_ - kl) <= 0.02 * kl          # the record is the KL one update before the end


# ------------------------------------------------------------------ 9. evaluation entries and the driver
def test_evaluation_entries_and_driver(tmp_path, capsys):
    from helpers import load_golden
    from test_umap_gpu import _batches, _vitsom
    from vit_som_amd.evaluation import TSNEQualityReport, evaluate_tsne_quality, visualize_tsne_progression
    from vit_som_amd.train import main, synthetic_loaders
    m, cfg = _vitsom()
    batches = _batches(cfg)
    n = sum(len(y) for _, y in batches)
    emb, labels = visualize_tsne_progression(m, cfg, batches, epoch=3, output_dir=str(tmp_path))
    assert emb.shape == (n, 2) and emb.dtype == np.float32 and np.isfinite(emb).all()
    assert np.array_equal(labels, np.concatenate([y.numpy() for _, y in batches]))
    try:
        import matplotlib  # noqa: F401
        assert os.path.getsize(tmp_path / "som_tsne_epoch_3.png") > 0
    except ImportError:
        pass
    rep = evaluate_tsne_quality(m, cfg, batches)
    assert isinstance(rep, TSNEQualityReport) and rep.n_samples == n and rep.n_neighbors == 15
    assert 0.0 <= rep.trustworthiness <= 1.0 and 0.0 <= rep.continuity <= 1.0 and rep.kl_divergence > 0 and rep.n_iter <= 999
    assert np.array_equal(rep.embedding, emb) and rep.inference_time > 0          # the same deterministic fit
    assert "t-SNE Trustworthiness:" in capsys.readouterr().out
    _, cfg2 = load_golden("ref_cluster_tiny")
    cfg2 = copy.deepcopy(cfg2)
    cfg2["hyperparameters"]["batch_size"] = 16
    logs = []
    loaders = lambda c, r, w: synthetic_loaders(c, r, w, n_train=64, n_val=16, n_test=16)      # noqa: E731
    today = {"accuracy", "precision", "recall", "f1", "purity", "nmi", "run_duration", "inference_time"}
    met = main(cfg2, n_runs=1, max_epochs=1, make_loaders=loaders, model_states_dir=str(tmp_path / "a"), log=logs.append,
               tsne_quality=True)
    assert set(met) == today | {"tsne_trustworthiness", "tsne_kl"}
    (t,), (k,) = met["tsne_trustworthiness"], met["tsne_kl"]
    assert 0.0 <= t <= 1.0 and k > 0
    assert any("t-SNE quality: trustworthiness" in l for l in logs)
