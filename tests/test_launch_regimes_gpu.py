"""Every row of tests/launch_regimes.py on the MI355X, on both sides of its threshold.

1. Against fp64 by the module's own rule: the references, check functions and test bodies of the module's GPU file are
   imported and run unchanged at the row's shape (gmm_ref / test_gmm_gpu, test_kmeans_cpu's oracles, linear_probe_ref,
   pca_ref, tsne_ref, numeric_edges' evaluators, torch's AdamW).  No tolerance is set here.
2. Regime invariance, bit for bit: where an output depends on a row or an element alone (GMM resp / log_prob_norm / labels,
   k-means labels / mind, the probe's residual / probabilities / predictions, AdamW's p / m / v, l1_loss's dpred, LayerNorm's
   dx), the same rows or elements run again in calls that stay below the threshold and must give the same bits.  Slices start
   on 16-byte boundaries of the same buffer with the same row stride, so both runs take the same vector path; that
   precondition is asserted.  Sums whose order changes with the split are compared with fp64 only.

Every figure is printed before it is asserted."""
import functools

import numpy as np
import pytest
import torch

import gmm_ref as GR
import launch_regimes as LR

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    from vit_som_amd import ops as _ops
    return _ops


def _bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _slices(n, step):
    return [(a, min(a + step, n)) for a in range(0, n, step)]


def _even_slices(n, most, granule=4):
    """About equal pieces of at most `most` items that start on multiples of `granule` (k-means wants k <= N of every call)."""
    count = -(-n // most)
    step = -(-(-(-n // count)) // granule) * granule
    assert step <= most
    return _slices(n, step)


def _same_path(whole, part):
    """The slice takes the vector path of the whole: the same alignment class and the same row stride."""
    assert part.data_ptr() % 16 == whole.data_ptr() % 16
    assert part.dim() == 1 or part.shape[0] == 1 or part.stride(0) == whole.stride(0)


# ------------------------------------------------------------------ Gaussian mixtures: the E-step
def _tg():
    import test_gmm_gpu as TG
    return TG


@pytest.mark.parametrize("ctype", ["diag", "spherical"])
@pytest.mark.parametrize("r", LR.rows_of("vsom_gmm_estep"), ids=LR.row_id)
def test_gmm_estep(r, ctype):
    TG = _tg()
    N, D, K = r.shape
    X, means, prec, w, logc, ref, e32 = TG._case(N, D, K, ctype)
    share = float((ref["gap"] > GR.GAP).mean())
    print(f"estep {r.regime} {r.shape} {ctype}: {share:.4f} of the rows enter the label check")
    assert share >= LR.MIN_SHARE
    Xd = TG._dev(X, torch.float32)
    assert Xd.data_ptr() % 16 == 0
    full = TG._estep(Xd, means, prec, logc)
    TG._check_estep(f"estep {r.regime} {N}x{D}x{K} {ctype}", full, ref, e32, N)
    bare = TG._estep(Xd, means, prec, logc, want_resp=False, want_labels=False)             # resp and labels null
    TG._check_estep(f"estep {r.regime} {N}x{D}x{K} {ctype}, no resp", bare, ref, e32, N)
    assert _same_bits(bare["lpn"], full["lpn"]) and _same_bits(bare["estat"], full["estat"])
    # the same rows in calls of at most 8192: one step to a workgroup
    for a, b in _even_slices(N, LR.SLICE_ROWS):
        assert LR.row_steps(b - a, 256)[2] == 1
        _same_path(Xd, Xd[a:b])
        part = TG._estep(Xd[a:b], means, prec, logc)
        for key in ("resp", "lpn", "labels"):
            assert _same_bits(part[key], full[key][a:b]), (key, a, b)


@pytest.mark.parametrize("shape,bad", LR.ESTEP_BAD_ROWS, ids=lambda v: "x".join(map(str, v)))
def test_gmm_estep_refuses_rows_of_a_second_step(shape, bad):
    """A NaN row and an overflowing row in second steps (one of the table's in a last workgroup): estat[1] counts them, their
    labels are -1, and every other row keeps its bits."""
    TG = _tg()
    N, D, K = shape
    X, means, prec, w, logc, ref, e32 = TG._case(N, D, K, "diag")
    clean = X.copy()
    clean[list(bad)] = 0.0
    dirty = clean.copy()
    dirty[bad[0], D - 1], dirty[bad[1], 0] = np.nan, 3e38                                  # (3e38 - mu)^2 overflows f32
    a = TG._estep(TG._dev(clean, torch.float32), means, prec, logc)
    b = TG._estep(TG._dev(dirty, torch.float32), means, prec, logc)
    print(f"bad rows {bad} of {shape}: estat {b['estat']}, clean estat {a['estat']}")
    assert a["estat"][1] == 0 and b["estat"][1] == 2
    for row in bad:
        assert np.isnan(b["lpn"][row]) and np.isnan(b["resp"][row]).all() and b["labels"][row] == -1
    keep = np.ones(N, bool)
    keep[list(bad)] = False
    for key in ("lpn", "resp", "labels"):
        assert _same_bits(a[key][keep], b[key][keep]), key
    assert np.isfinite(b["estat"][0]) and abs(b["estat"][0] - b["lpn"][keep].sum()) <= 1e-12 * np.abs(b["lpn"][keep]).sum()


# ------------------------------------------------------------------ Gaussian mixtures: the M-step and the parameters
@pytest.mark.parametrize("ctype", ["diag", "spherical"])
@pytest.mark.parametrize("r", LR.rows_of("vsom_gmm_mstep") + LR.rows_of("vsom_gmm_params"), ids=LR.row_id)
def test_gmm_mstep_and_params(r, ctype):
    """The body of test_gmm_gpu.test_mstep_and_params_against_fp64 at the row's shape."""
    TG = _tg()
    N, D, K = r.shape
    X, means, prec, w = GR.mixture_case(N, D, K, ctype)
    resp, reg = TG._soft_resp(N, K), 1e-6
    nk, mu, cov = GR.mstep64(X, resp, reg, ctype)
    nk32, mu32, cov32 = GR.mstep32(X, resp, reg, ctype)
    got = TG._mstep_params(TG._dev(X, torch.float32), resp, means, reg, ctype)
    wref = nk / nk.sum()
    ref = dict(means=mu, cov=cov, weights=wref, prec=GR.full_prec(1.0 / cov, D), logc=GR.logc64(wref, 1.0 / cov, D))
    y32 = dict(means=mu32, cov=cov32, weights=nk32 / nk32.sum(), prec=GR.full_prec(1.0 / cov32, D),
               logc=GR.logc64(nk32 / nk32.sum(), 1.0 / cov32, D))
    for key in ref:
        e_k, e32 = GR.err(got[key], ref[key]), GR.err(y32[key], ref[key])
        print(f"mstep {r.regime} {N}x{D}x{K} {ctype}: {key} error {e_k:.3e}, plain fp32 {e32:.3e}, bound {GR.bound(GR.FLOOR, e32):.3e}")
        assert e_k <= GR.bound(GR.FLOOR, e32)
    rec = got["record"]
    assert np.isnan(rec[0]) and abs(rec[1] - nk.min()) <= 1e-6 * nk.min() and abs(rec[2] - cov.min()) <= GR.FLOOR * abs(cov).max()
    assert rec[3] == 0 and rec[4] == 0


# ------------------------------------------------------------------ k-means: assign and update
@pytest.mark.parametrize("r", LR.rows_of("vsom_kmeans_assign") + LR.rows_of("vsom_kmeans_update"), ids=LR.row_id)
def test_kmeans_assign_and_update(r):
    import test_kmeans_gpu as TK
    N, D, k = r.shape
    X, C = TK._data(N + D + k, N, D, k)
    prev = torch.randint(-1, k, (N,), generator=torch.Generator().manual_seed(1))
    Xd, Cd, pd = X.cuda(), C.cuda(), prev.cuda()
    out = TK._one_iteration(Xd, Cd, pd)
    TK._check_iteration(X.numpy(), C.numpy(), prev.numpy(), out, min_clear=LR.MIN_SHARE)
    # the figures _check_iteration holds to its 1e-5 (it prints nothing): against fp64, next to the same sums in plain fp32
    from test_kmeans_cpu import average_centers, sums_counts
    labels, mind, cnew = out[0], out[1], out[2]
    own = ((X.double() - C.double()[labels]) ** 2).sum(1).numpy()
    own32 = ((X - C[labels]) ** 2).sum(1).numpy()
    ref_c = average_centers(*sums_counts(X.numpy(), labels, k))
    c32 = torch.zeros(k, D).index_add_(0, torch.from_numpy(labels), X).numpy() / np.maximum(np.bincount(labels, minlength=k), 1)[:, None]
    filled = np.bincount(labels, minlength=k) > 0
    print(f"kmeans {r.regime} {N}x{D}x{k}: mind error {GR.err(mind, own):.3e}, plain fp32 {GR.err(own32, own):.3e}; centre error "
          f"{GR.err(cnew[filled], ref_c[filled]):.3e}, plain fp32 {GR.err(c32[filled], ref_c[filled]):.3e}; bound 1.000e-05")
    for a, b in _even_slices(N, LR.SLICE_ROWS) if r.entry == "vsom_kmeans_assign" else []:
        assert LR.row_steps(b - a, 256)[2] == 1
        _same_path(Xd, Xd[a:b])
        part = TK._one_iteration(Xd[a:b], Cd, pd[a:b].contiguous())
        assert _same_bits(part[0], out[0][a:b]) and _same_bits(part[1], out[1][a:b]), (a, b)


# ------------------------------------------------------------------ t-SNE: one step
@functools.lru_cache(maxsize=None)
def _tsne_p(N):
    """The joint P of clustered rows as test_tsne_gpu._joint_p builds it, the fp64 neighbour search done on the device."""
    import tsne_ref as R
    from vit_som_amd.tsne import joint_probabilities
    X, _ = R.blobs(N, 16, 5, 40 + N, scale=3.0)
    Xd = torch.from_numpy(X).to(DEV).double()
    D = torch.cdist(Xd, Xd)
    D.fill_diagonal_(float("inf"))
    dist, idx = torch.topk(D, 63, dim=1, largest=False, sorted=True)
    return joint_probabilities(idx.cpu().numpy(), R.conditional_p(R.squared_f32(dist.float().cpu().numpy()), 20.0)[0])


@pytest.mark.parametrize("r", LR.rows_of("vsom_tsne_step"), ids=LR.row_id)
def test_tsne_step(r, ops):
    """The body of test_tsne_gpu.test_step_against_the_restatement, the dense fp64 terms computed on the device."""
    import test_tsne_gpu as TT
    import tsne_ref as R
    N, = r.shape
    assert (ops.tsne_repulsion_parts(N) > 64) == (r.side == "past")
    P = _tsne_p(N)
    Pd = torch.from_numpy(np.asarray(P.todense())).to(DEV)
    rs = np.random.RandomState(N)
    Y = (3.0 * rs.standard_normal((N, 2))).astype(np.float32)
    Yd = torch.from_numpy(Y).to(DEV)
    lr, momentum = 200.0, 0.8
    for exaggeration in (12.0, 1.0):
        kl_r, grad = LR.kl_and_grad_torch(Pd, Yd, exaggeration, torch.float64)
        _, grad32 = LR.kl_and_grad_torch(Pd, Yd, exaggeration, torch.float32)
        scale = np.abs(grad).max()
        update = (rs.standard_normal((N, 2)) * lr * scale).astype(np.float32)
        gains = rs.uniform(0.005, 2.0, size=(N, 2)).astype(np.float32)
        gains[::7] = np.float32(0.0115)
        Y_r, u_r, g_r = R.update_step(Y, update, gains, grad, momentum, lr)
        Y_32, u_32, g_32 = R.update_step(Y, update, gains, grad32, momentum, lr)
        Y_d, u_d, g_d, kl_d, gn_d = TT._device_step(P, Y, update, gains, exaggeration, momentum, lr)
        TT._yardstick(f"N={N} exaggeration {exaggeration}: Y_out", Y_d, Y_r, Y_32)
        TT._yardstick(f"N={N} exaggeration {exaggeration}: update", u_d, u_r, u_32)
        sure = np.abs(update.astype(np.float64) * grad) >= 1e-30
        assert np.array_equal(g_d[sure], g_r[sure]) and (g_d >= np.float32(0.01)).all()
        TT._yardstick(f"N={N} exaggeration {exaggeration}: gains", g_d, g_r, g_32)
        gn_r = float(np.sqrt((grad * grad).sum()))
        print(f"N={N} exaggeration {exaggeration}: KL {kl_d:.12f} against {kl_r:.12f}, |grad| {gn_d:.9e} against {gn_r:.9e}")
        assert abs(kl_d - kl_r) <= 1e-6 * abs(kl_r) and abs(gn_d - gn_r) <= 1e-6 * gn_r


# ------------------------------------------------------------------ the linear probe
def _residual_outputs(ops, Zd, b, yd):
    N, C = Zd.shape
    R = torch.full((N, C + 1), float("nan"), device=DEV)[:, :C]
    loss, gb = torch.empty(1, dtype=torch.float64, device=DEV), torch.empty(C, dtype=torch.float64, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    pred, prob = torch.full((N,), -7, dtype=torch.int64, device=DEV), torch.full((N, C), float("nan"), dtype=torch.float64, device=DEV)
    ops.probe_residual(Zd, b, yd, R, loss, gb, status, pred, prob)
    return R, pred, prob


@pytest.mark.parametrize("r", LR.rows_of("vsom_probe_residual"), ids=LR.row_id)
def test_probe_residual(r, ops):
    import test_linear_probe_gpu as TP
    N, C = r.shape
    TP.test_residual_against_fp64(N, C)
    Z, y, b = TP._logits(N, C, seed=N + C)
    Zd, yd, bd = TP._padded(Z, 3), TP._dev(y), TP._dev(b)
    whole = _residual_outputs(ops, Zd, bd, yd)
    for lo, hi in _slices(N, 16384):
        assert LR.probe_row_plan(hi - lo, C)[0] <= 16
        _same_path(Zd, Zd[lo:hi])
        part = _residual_outputs(ops, Zd[lo:hi], bd, yd[lo:hi])
        for got, want in zip(part, whole):
            assert _same_bits(got, want[lo:hi]), (lo, hi)


@pytest.mark.parametrize("r", LR.rows_of("vsom_probe_linesearch"), ids=LR.row_id)
def test_probe_linesearch(r):
    import test_linear_probe_gpu as TP
    TP.test_linesearch_ladder_against_fp64(*r.shape)


@pytest.mark.parametrize("r", LR.rows_of("vsom_lbfgs_dots"), ids=LR.row_id)
def test_lbfgs_dots_and_combine(r):
    import test_linear_probe_gpu as TP
    TP.test_lbfgs_direction_is_the_two_loop_recursion(*r.shape)


@pytest.mark.parametrize("r", LR.rows_of("vsom_probe_fold"), ids=LR.row_id)
def test_probe_fold(r):
    import test_linear_probe_gpu as TP
    TP.test_fold_and_gradient(*r.shape)


# ------------------------------------------------------------------ PCA: project and backproject
PCA_SHAPES = sorted({r.shape for r in LR.rows_of("vsom_pca_project") + LR.rows_of("vsom_pca_backproject")})


@pytest.mark.parametrize("shape", PCA_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_pca_project_and_backproject(shape):
    """Exactly, on integers (a split that drops or repeats a k-tile shows bit for bit), and within the rule on floats."""
    import test_pca_gpu as TC
    TC.test_project_and_backproject_are_exact_on_integers(*shape)
    TC.test_kernels_within_the_rule(*shape)


# ------------------------------------------------------------------ AdamW
ADAMW_WD = (0.05, 0.0, 0.01, 0.03)


def _adamw_case(n):
    g0 = torch.Generator().manual_seed(n % 1000)
    p, gr = torch.randn(n, generator=g0), torch.randn(n, generator=g0)
    which = torch.randint(0, len(ADAMW_WD), (n // 256,), generator=g0)                      # no period: a wrong chunk index shows
    return p, gr, which, torch.tensor(ADAMW_WD)[which]


def _adamw_torch(p, gr, which, steps):
    """torch.optim.AdamW as in test_ops_gpu.test_adamw_step, one parameter group per weight-decay value."""
    el = which.repeat_interleave(256)
    idx = [torch.nonzero(el == j).squeeze(1) for j in range(len(ADAMW_WD))]
    leaves = [p[i].clone().requires_grad_(True) for i in idx]
    opt = torch.optim.AdamW([{"params": [l], "weight_decay": w} for l, w in zip(leaves, ADAMW_WD)], lr=3e-3, betas=(0.9, 0.999))
    for _ in range(steps):
        for l, i in zip(leaves, idx):
            l.grad = gr[i] * 0.5
        opt.step()
    out = torch.empty_like(p)
    for l, i in zip(leaves, idx):
        out[i] = l.detach()
    return out


@pytest.mark.parametrize("r", LR.rows_of("vsom_adamw_step"), ids=LR.row_id)
def test_adamw_flat(r, ops):
    n, = r.shape
    p, gr, which, wd = _adamw_case(n)
    pd, gd, wdd = p.to(DEV), gr.to(DEV), wd.to(DEV)
    m, v = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    # the same elements as two sub-arenas with their own wd_chunk slices, each below the threshold
    cut = (n // 2) // 256 * 256
    ps, ms, vs = pd.clone(), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    for step in (1, 2):
        ops.adamw_step(pd, gd, m, v, wdd, 3e-3, 0.9, 0.999, 1e-8, step, grad_scale=0.5)
        for a, b in ((0, cut), (cut, n)):
            assert (b - a) <= 8388608 and (b - a) % 256 == 0
            _same_path(pd, ps[a:b])
            ops.adamw_step(ps[a:b], gd[a:b], ms[a:b], vs[a:b], wdd[a // 256:b // 256], 3e-3, 0.9, 0.999, 1e-8, step, grad_scale=0.5)
        assert _same_bits(pd, ps) and _same_bits(m, ms) and _same_bits(v, vs), step
    ref = _adamw_torch(p, gr, which, 2)
    err = float((pd.cpu() - ref).abs().max())
    print(f"adamw {r.regime} n={n}: |p - torch.optim.AdamW| max {err:.3e} (test_adamw_step's rule: allclose with atol 2e-7)")
    assert torch.allclose(pd.cpu(), ref, atol=2e-7)


@pytest.mark.parametrize("r", LR.rows_of("vsom_adamw_step_planes"), ids=LR.row_id)
def test_adamw_planes(r, ops):
    """test_ops_gpu.test_adamw_step_planes_is_the_flat_step_plus_the_split with the arena outside the slice past 2^23."""
    n, = r.shape
    R, L, lead = 70, 136, 768
    padded = (R * L + 255) // 256 * 256
    assert (n - padded > 8388608) == (r.side == "past")
    p, gr, which, wd = _adamw_case(n)
    p, gr = p.clone(), gr.clone()
    p[lead + R * L:lead + padded] = 0; gr[lead + R * L:lead + padded] = 0
    pa, pb, gd, wdd = p.to(DEV), p.to(DEV), gr.to(DEV), wd.to(DEV)
    ma, va, mb, vb = (torch.zeros(n, device=DEV) for _ in range(4))
    planes, ref = ops.bmu_planes_alloc(R, L, DEV), ops.bmu_planes_alloc(R, L, DEV)
    planes.zero_(); ref.zero_()
    for step in (1, 2):
        ops.adamw_step(pa, gd, ma, va, wdd, 3e-3, 0.9, 0.999, 1e-8, step, grad_scale=0.5)
        ops.adamw_step(pb, gd, mb, vb, wdd, 3e-3, 0.9, 0.999, 1e-8, step, grad_scale=0.5, planes=(lead, R, L, planes))
        assert _same_bits(pa, pb) and _same_bits(ma, mb) and _same_bits(va, vb), step
        ops.bmu_planes_from(pb[lead:lead + R * L].view(R, L), ref)
        assert torch.equal(planes, ref), step


# ------------------------------------------------------------------ fill, scale_by, scaled_mul
@pytest.mark.parametrize("r", LR.rows_of("vsom_fill") + LR.rows_of("vsom_scale_by") + LR.rows_of("vsom_scaled_mul"), ids=LR.row_id)
def test_fill_scale_by_scaled_mul(r, ops):
    n, = r.shape
    g0 = torch.Generator().manual_seed(5)
    a, b = torch.randn(n, generator=g0), torch.randn(n, generator=g0)
    s = torch.tensor([0.375], device=DEV)
    if r.entry == "vsom_fill":
        t = torch.full((n + 64,), float("nan"), device=DEV)
        ops.fill(t[:n], 2.5)
        assert bool((t[:n] == 2.5).all()) and bool(torch.isnan(t[n:]).all())
    elif r.entry == "vsom_scale_by":
        t = a.to(DEV)
        ops.scale_by(t, s)
        assert _same_bits(t, a * 0.375)                          # one f32 product, rounded once
    else:
        out = torch.full((n,), float("nan"), device=DEV)
        ops.scaled_mul(out, a.to(DEV), b.to(DEV), s, 0.5)
        assert _same_bits(out, (torch.tensor(0.375) * 0.5) * a * b)              # v * a[i] * b[i], each product rounded once


# ------------------------------------------------------------------ L1
@pytest.mark.parametrize("r", LR.rows_of("vsom_l1_loss"), ids=LR.row_id)
def test_l1_loss(r, ops):
    import numeric_edges as NE
    import test_numeric_edges_gpu as TN
    n, = r.shape
    TN.test_l1_loss_edges(ops, n)
    c = NE.l1_case(n)
    pd, td = c.inp["pred"].to(DEV), c.inp["target"].to(DEV)
    loss, dp = torch.zeros(1, device=DEV), torch.full((n,), float("nan"), device=DEV)
    ops.l1_loss(pd, td, loss, dpred=dp, grad_scale=0.25)
    for a, b in _slices(n, 1048576):
        _same_path(pd, pd[a:b])
        part, ls = torch.full((b - a,), float("nan"), device=DEV), torch.zeros(1, device=DEV)
        ops.l1_loss(pd[a:b], td[a:b], ls, dpred=part, grad_scale=0.25)
        assert _same_bits(part, dp[a:b]), (a, b)


@pytest.mark.parametrize("r", LR.rows_of("vsom_l1_unpatchify"), ids=LR.row_id)
def test_l1_unpatchify(r, ops):
    import test_numeric_edges_gpu as TN
    TN.test_l1_unpatchify_edges(ops, r.shape)


# ------------------------------------------------------------------ LayerNorm backward
@pytest.mark.parametrize("r", LR.rows_of("vsom_layernorm_bwd"), ids=LR.row_id)
def test_layernorm_bwd(r, ops):
    import numeric_edges as NE
    import test_numeric_edges_gpu as TN
    rows, cols = r.shape
    TN.test_layernorm_edges(ops, r.shape, "mixed")
    c = NE.layernorm_case(r.shape, "mixed")
    x, gamma, beta, dy, resid = (c.inp[k].to(DEV) for k in ("x", "gamma", "beta", "dy", "resid"))
    y, mean, rstd = torch.empty(rows, cols, device=DEV), torch.empty(rows, device=DEV), torch.empty(rows, device=DEV)
    ops.layernorm_fwd(x, gamma, beta, y, mean, rstd, NE.LN_EPS)
    dx, dg, db = torch.full((rows, cols), float("nan"), device=DEV), torch.empty(cols, device=DEV), torch.empty(cols, device=DEV)
    ops.layernorm_bwd(dy, x, mean, rstd, gamma, resid, dx, dg, db)
    for a, b in _slices(rows, 4096):
        if cols % 4 == 0:
            _same_path(x, x[a:b]); _same_path(dy, dy[a:b]); _same_path(resid, resid[a:b])       # (the element kernel has one path)
        part = torch.full((b - a, cols), float("nan"), device=DEV)
        ops.layernorm_bwd(dy[a:b], x[a:b], mean[a:b], rstd[a:b], gamma, resid[a:b], part, dg, db)
        assert _same_bits(part, dx[a:b]), (a, b)


# ------------------------------------------------------------------ contingency and last_label
@pytest.mark.parametrize("r", LR.rows_of("vsom_contingency") + LR.rows_of("vsom_last_label"), ids=LR.row_id)
def test_contingency_and_last_label(r, ops):
    n, = r.shape
    g0 = torch.Generator().manual_seed(n % 997)
    na, nb = 37, 11
    a, b = torch.randint(0, na, (n,), generator=g0), torch.randint(0, nb, (n,), generator=g0)
    a[n - 1], b[n - 2] = na, -1                                   # two pairs out of range, in the part past the threshold
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    ok = ((a >= 0) & (a < na) & (b >= 0) & (b < nb)).numpy()
    if r.entry == "vsom_contingency":
        t = torch.zeros(na, nb, dtype=torch.int64, device=DEV)
        ops.contingency(a.to(DEV), b.to(DEV), t, bad)
        ref = np.zeros((na, nb), dtype=np.int64)
        np.add.at(ref, (a.numpy()[ok], b.numpy()[ok]), 1)
        assert np.array_equal(t.cpu().numpy(), ref) and int(bad) == 2 and int(ref.sum()) == n - 2
    else:
        cells = torch.zeros(na, dtype=torch.int64, device=DEV)
        ops.last_label(a.to(DEV), b.to(DEV), 0, cells, bad)
        ref = np.zeros(na, dtype=np.int64)
        i = np.nonzero(ok)[0]
        np.maximum.at(ref, a.numpy()[i], ((i + 1) << 32) | b.numpy()[i])            # the last sample of a cell stays
        assert np.array_equal(cells.cpu().numpy(), ref) and int(bad) == 2
        assert (ref >> 32).max() > 524288 or r.side == "below"


# ------------------------------------------------------------------ silhouette: the clear of its workspace
@pytest.mark.parametrize("r", LR.rows_of("vsom_silhouette"), ids=LR.row_id)
def test_silhouette_clears_a_poisoned_workspace(r, ops):
    """test_silhouette_gpu.test_many_column_chunks_equal_the_restatement with so many clusters that the cleared words pass
    4096 x 256, on a workspace of all-ones bytes: a word the clear leaves out shows in the exact integer sums."""
    import silhouette_ref as SR
    import test_silhouette_gpu as TS
    N, C, D = r.shape
    X, y = np.random.default_rng(N).integers(0, 32, (N, D)), TS._labels(N, C, N)
    D32, M = SR.exact_euclidean32(X)
    ws = ops.silhouette_workspace(N, C, DEV)
    ws.fill_(255)
    got = ops.silhouette(TS._dev(X), TS._lab(y), SR.EUCLIDEAN, C, ws=ws)
    assert np.array_equal(got.sums.cpu().numpy(), SR.fixed_sums(D32, y, C, SR.bound_exponent(M, SR.EUCLIDEAN)))
    counts = np.bincount(y, minlength=C)
    assert np.array_equal(got.counts.cpu().numpy(), counts)
    assert got.status == [0, 0, C, int((counts == 1).sum())]


# ------------------------------------------------------------------ kNN query: more than one column tile to a chunk
@pytest.mark.parametrize("metric", ["cosine", "euclidean"])
@pytest.mark.parametrize("r", LR.rows_of("vsom_knn_query"), ids=LR.row_id)
def test_knn_query(r, metric):
    """test_knn_gpu.test_query_against_fp64's checks (knn_checks.lists_against_fp64) at the row's shape; then the same queries
    in calls of at most 44 row blocks (one tile to a chunk), with and without `exclude`, bit for bit."""
    import test_knn_gpu as TK
    from knn_checks import lists_against_fp64
    Nq, Nb, D, k = r.shape
    Q, X = (t.to(TK.DEV) for t in TK._randn(Nq, Nb, D))
    idx, dist = TK._query(Q, X, k, metric)
    share, err = lists_against_fp64(idx, dist, Q, X, k, metric)
    print(f"knn {r.regime} {r.shape} {metric}: distance error {err:.3e} (bound 1.000e-05), rows compared index by index {share:.4f}")
    assert share >= LR.MIN_SHARE
    excl = idx[:, 0].contiguous()                                   # every query refuses its nearest bank row
    idx_x, dist_x = TK._query(Q, X, k, metric, exclude=excl)
    assert not bool((idx_x == excl[:, None]).any())
    assert torch.equal(idx_x[:, :k - 1], idx[:, 1:]) and _same_bits(dist_x[:, :k - 1], dist[:, 1:])
    for a, b in _even_slices(Nq, 44 * 128, granule=128):
        assert LR.knn_query_plan(b - a, Nb)["most_tiles"] == 1
        _same_path(Q, Q[a:b])
        pi, pd = TK._query(Q[a:b], X, k, metric)
        assert torch.equal(pi, idx[a:b]) and _same_bits(pd, dist[a:b]), (a, b)
        pi, pd = TK._query(Q[a:b], X, k, metric, exclude=excl[a:b].contiguous())
        assert torch.equal(pi, idx_x[a:b]) and _same_bits(pd, dist_x[a:b]), (a, b)


# ------------------------------------------------------------------ the probe's step: theta, s_new and Z
@pytest.mark.parametrize("r", LR.rows_of("vsom_probe_step"), ids=LR.row_id)
def test_probe_step(r, ops):
    """As test_linear_probe_gpu.test_linesearch_identity_and_the_step_chosen_on_the_device: Z and Zp are multiples of 2^-6 and
    alpha a power of two, so Z + alpha Zp, theta + alpha p and alpha p are exact and the device must give the fp64 values bit
    for bit; the ladder is made so that the third step (alpha = 1/4) is the first accepted."""
    import linear_probe_ref as PR
    import test_linear_probe_gpu as TP
    N, C, D = r.shape
    n = C * D + C
    rng = np.random.RandomState(N + C)
    Z = (rng.randint(-512, 513, (N, C)) / 64.0).astype(np.float32)
    Zp = (rng.randint(-256, 257, (N, C)) / 64.0).astype(np.float32)
    theta, p = rng.standard_normal(n), rng.standard_normal(n)
    phi = np.array([1e12, 1e12] + [float(N)] * 6)
    lam, pen, gtp, f0 = 0.01, np.array([3.0, -0.5, 2.0]), -1e-3, 2.0 * N
    alpha, status, F, j = PR.armijo(phi, 1.0, f0, pen, gtp, N, lam)
    assert (alpha, status, j) == (0.25, 0, 2)

    def run(rows, vec):
        Zd, Zpd = TP._padded(Z[rows], 3), TP._padded(Zp[rows], 3)
        th, s = TP._dev(theta[vec]), torch.full((len(theta[vec]),), float("nan"), dtype=torch.float64, device=DEV)
        rec = torch.zeros(16, dtype=torch.float64, device=DEV)
        ops.probe_step(TP._dev(phi), TP._dev([1.0]), TP._dev([f0]), TP._dev(pen), TP._dev([gtp]), lam, 1e-4, Zd, Zpd, th, TP._dev(p[vec]),
                       s, rec)
        assert bool(torch.isnan(Zd.as_strided((Zd.shape[0], 3), (C + 3, 1), C)).all())       # the padding columns are not touched
        return TP._host(Zd), TP._host(th), TP._host(s), TP._host(rec)

    Zo, th, s, rec = run(slice(0, N), slice(0, n))
    assert (rec[12], int(rec[13]), rec[14], int(rec[15])) == (alpha, status, F, j)
    assert _same_bits(Zo, (Z.astype(np.float64) + alpha * Zp.astype(np.float64)).astype(np.float32))
    assert _same_bits(th, theta + alpha * p) and _same_bits(s, alpha * p)
    # the same elements in two calls below 2048 x 256 each
    hn, hv = N // 2, n // 2
    for rows, vec in ((slice(0, hn), slice(0, hv)), (slice(hn, N), slice(hv, n))):
        assert max((rows.stop - rows.start) * C, vec.stop - vec.start) <= 2048 * 256
        Zs, ths, ss, _ = run(rows, vec)
        assert _same_bits(Zs, Zo[rows]) and _same_bits(ths, th[vec]) and _same_bits(ss, s[vec])


# ------------------------------------------------------------------ rows_add
@pytest.mark.parametrize("r", LR.rows_of("vsom_rows_add"), ids=LR.row_id)
def test_rows_add(r, ops):
    rows, cols = r.shape
    g0 = torch.Generator().manual_seed(rows)
    src, dst = torch.randn(rows, cols + 5, generator=g0), torch.randn(rows, cols + 3, generator=g0)
    sd, dd = src.to(DEV), dst.to(DEV)
    ops.rows_add(sd[:, :cols], dd[:, 1:cols + 1])                    # two row strides, dst off 16-byte alignment
    want = dst.clone()
    want[:, 1:cols + 1] += src[:, :cols]                            # one f32 addition per element; the padding stays
    assert _same_bits(dd, want)


# ------------------------------------------------------------------ Manhattan distance pass: a short last split
@pytest.mark.parametrize("r", LR.rows_of("vsom_bmu_manhattan_fwd"), ids=LR.row_id)
def test_bmu_manhattan_splits(r, ops):
    """The body of test_ops_gpu.test_som_manhattan_fwd_and_bwd at the row's shape (its bounds: distances 2e-6 relative)."""
    import test_ops_gpu as TO
    from oracle import vitsom_oracle
    B, K, L = r.shape
    assert ops.lib.vsom_bmu_manhattan_workspace_bytes(B, K, L) == r.plan["splits"] * B * K * 4
    TO.test_som_manhattan_fwd_and_bwd(ops, vitsom_oracle, B, K, L, (4, 3), "hexa")
    x, W = TO.rnd(B, L, seed=1), torch.rand(K, L, generator=torch.Generator().manual_seed(2))
    dist, bmu = torch.empty(B, K, device=DEV), torch.empty(B, dtype=torch.int64, device=DEV)
    ops.bmu_manhattan_fwd(x.to(DEV), W.to(DEV), dist, bmu)
    ref = torch.cdist(x.double(), W.double(), p=1)
    print(f"manhattan {r.regime} {B}x{K}x{L}: distance error {TO.rel_err(dist.cpu(), ref):.3e}, plain fp32 "
          f"{TO.rel_err(torch.cdist(x, W, p=1), ref):.3e}, bound 2.000e-06")


# ------------------------------------------------------------------ attention maps
@pytest.mark.parametrize("r", LR.rows_of("vsom_attention_probs"), ids=LR.row_id)
def test_attention_probs(r, ops):
    """numeric_edges.attention_eval in fp64 and plain fp32, and test_attention_edges' rule for probs: max(3e-6, 4 e32) absolute."""
    import numeric_edges as NE
    B, N, H, hd = r.shape
    qkv, dout = NE.rnd(B, N, 3 * H * hd, seed=N), torch.zeros(B, N, H * hd)
    ref = NE.attention_eval(qkv, dout, B, N, H, hd, torch.float64)["probs"]
    y32 = NE.attention_eval(qkv, dout, B, N, H, hd, torch.float32)["probs"]
    probs = torch.full((B, H, N, N), float("nan"), device=DEV)
    ops.attention_probs(qkv.to(DEV), torch.zeros(B, H, N, device=DEV), probs, B, N, H, hd)
    e_k, e32 = NE.max_abs(probs.cpu(), ref), NE.max_abs(y32, ref)
    print(f"attention_probs {r.regime} {r.shape}: error {e_k:.3e}, plain fp32 {e32:.3e}, bound {NE.bound(3e-6, e32):.3e}")
    assert NE.accepts(e_k, 3e-6, e32)
