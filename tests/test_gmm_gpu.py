"""Gaussian mixtures on the MI355X: the E-step, M-step and parameter kernels against the fp64 restatements of gmm_ref.py
(plain, strided, misaligned, at numerical edges, with bad rows, inside guard bands), whole fits against sklearn on the
float64 copy of the data, the estimator's behaviour, and evaluate_gmm on the golden ViTSOM / DESOM.

The rule everywhere (gmm_ref.py): a device value may differ from fp64 by max(FLOOR, 4 x the error of the plain-fp32
restatement on the same input), errors relative to the largest reference value.  Every figure is printed before it is
asserted."""
import copy
import functools
import warnings

import numpy as np
import pytest
import torch

import gmm_ref as R
import memcheck as MC

pytestmark = pytest.mark.gpu

EPS10 = R.EPS10


def _dev(a, dtype):
    return torch.tensor(np.asarray(a)).to(device="cuda", dtype=dtype).contiguous()


def _f64(*shape):
    return torch.empty(*shape, dtype=torch.float64, device="cuda")


@functools.lru_cache(maxsize=None)
def _case(N, D, K, ctype, seed=0, offset=0.0, spread=1.0):
    """Inputs (the precisions as the kernel sees them: rounded to f32), the fp64 reference and the fp32 yardstick; shared."""
    X, means, prec, w = R.mixture_case(N, D, K, ctype, seed, offset, spread)
    prec = prec.astype(np.float32).astype(np.float64)
    logc = R.logc64(w, prec, D)
    ref = R.estep64(X, means, prec, w)
    lpn32, resp32 = R.estep32(X, means, prec, logc)
    e32 = dict(lpn=R.err(lpn32, ref["lpn"]), resp=R.err(resp32, ref["resp"]))
    for a in (X, means, prec, w, logc, *ref.values()):
        a.setflags(write=False)
    return X, means, prec, w, logc, ref, e32


def _estep(Xd, means, prec, logc, want_resp=True, want_labels=True, guard=False, ldr=None):
    """One vsom_gmm_estep -> dict of host arrays (and the guard handles when guard)."""
    from vit_som_amd import ops
    N, D = Xd.shape
    K = means.shape[0]
    md, pd, cd = _dev(means, torch.float32), _dev(R.full_prec(prec, D), torch.float32), _dev(logc, torch.float64)
    handles = []
    if guard:
        def out(shape, dtype, ld=None):
            v, h = MC.guarded(shape, dtype, "cuda", ld=ld)
            handles.append(h)
            return v
    else:
        def out(shape, dtype, ld=None):
            if ld is None:
                return torch.empty(*shape, dtype=dtype, device="cuda")
            return torch.full((shape[0], ld), float("nan"), dtype=dtype, device="cuda")[:, :shape[1]]
    resp = out((N, K), torch.float32, ldr) if want_resp else None
    lpn = out((N,), torch.float64)
    labels = out((N,), torch.int64) if want_labels else None
    estat = out((2,), torch.float64)
    part = out((ops.gmm_parts(N, D, K, ops.GMM_ESTEP),), torch.float64) if guard else None
    ops.gmm_estep(Xd, md, pd, cd, resp, lpn, labels, estat, part)
    torch.cuda.synchronize()
    got = dict(lpn=lpn.cpu().numpy(), estat=estat.cpu().numpy(), resp=resp.cpu().numpy() if want_resp else None,
               labels=labels.cpu().numpy() if want_labels else None)
    return (got, handles) if guard else got


def _check_estep(name, got, ref, e32, N):
    for key in ("lpn", "resp"):
        if got[key] is None:
            continue
        e_k, lim = R.err(got[key], ref[key]), R.bound(R.FLOOR, e32[key])
        print(f"{name}: {key} error {e_k:.3e}, plain fp32 {e32[key]:.3e}, bound {lim:.3e}")
        assert e_k <= lim
    assert e32["lpn"] <= R.E32_MAX                        # (resp: plain fp32 is off by 1e-3 at D = 12 288, 1e-5 at D = 128)
    if got["labels"] is not None:
        clear = ref["gap"] > R.GAP
        assert (~clear).mean() <= R.MAX_UNCLEAR, (~clear).mean()
        assert np.array_equal(got["labels"][clear], ref["labels"][clear])
    assert got["estat"][1] == 0 and abs(got["estat"][0] - got["lpn"].sum()) <= 1e-12 * max(np.abs(got["lpn"]).sum(), 1.0)


# ------------------------------------------------------------------ the E-step
@pytest.mark.parametrize("ctype", ["diag", "spherical"])
@pytest.mark.parametrize("N,D,K", R.SHAPES)
def test_estep_against_fp64(N, D, K, ctype):
    X, means, prec, w, logc, ref, e32 = _case(N, D, K, ctype)
    _check_estep(f"estep {N}x{D}x{K} {ctype}", _estep(_dev(X, torch.float32), means, prec, logc), ref, e32, N)


@pytest.mark.parametrize("i", range(len(R.SHAPES)))
def test_estep_strided_misaligned_and_without_resp(i):
    N, D, K = R.SHAPES[i]
    ctype = ("diag", "spherical")[i % 2]
    X, means, prec, w, logc, ref, e32 = _case(N, D, K, ctype)
    # a strided view whose padding columns hold NaN: they must never be read
    big = torch.full((N, D + 5), float("nan"))
    big[:, :D] = torch.tensor(X)
    Xs = big.cuda()[:, :D]
    assert Xs.stride(0) == D + 5 or N == 1
    got = _estep(Xs, means, prec, logc, ldr=K + 3)
    _check_estep(f"strided {N}x{D}x{K}", got, ref, e32, N)
    # without responsibilities (score_samples) and without labels: the same log_prob_norm, bit for bit
    plain = _estep(_dev(X, torch.float32), means, prec, logc)
    bare = _estep(_dev(X, torch.float32), means, prec, logc, want_resp=False, want_labels=False)
    assert np.array_equal(bare["lpn"], plain["lpn"]) and np.array_equal(bare["estat"], plain["estat"])
    _check_estep(f"no resp {N}x{D}x{K}", bare, ref, e32, N)
    # an odd-D view that starts one element off 16-byte alignment (the element path)
    Do = D if D % 2 else D - 1
    Xo, mo, po = X[:, :Do], means[:, :Do], (prec if ctype == "spherical" else prec[:, :Do])
    logco = R.logc64(w, po, Do)
    refo = R.estep64(Xo, mo, po, w)
    lpn32, resp32 = R.estep32(Xo, mo, po, logco)
    big = torch.full((N, Do + 2), float("nan"))
    big[:, 1:Do + 1] = torch.tensor(np.ascontiguousarray(Xo))
    Xv = big.cuda()[:, 1:Do + 1]
    assert Xv.data_ptr() % 16 == 4
    _check_estep(f"misaligned {N}x{Do}x{K}", _estep(Xv, mo, po, logco), refo,
                 dict(lpn=R.err(lpn32, refo["lpn"]), resp=R.err(resp32, refo["resp"])), N)


def test_estep_columns_offset_by_1000():
    """Columns at 1000 +- 1.  The rule still holds for the direct form.  sklearn's expanded form, sum mu^2 p - 2 x.mu p +
    x^2.p, would not: at D = 128 its three terms are near 1.3e8 each and cancel to a few hundred, so one fp32 rounding of a
    term (8 at that magnitude) is already an error of order one in log p."""
    for ctype in ("diag", "spherical"):
        X, means, prec, w, logc, ref, e32 = _case(257, 128, 3, ctype, 1, 1000.0, 1.0)
        _check_estep(f"offset 1000 {ctype}", _estep(_dev(X, torch.float32), means, prec, logc), ref, e32, 257)
        Xd, md, pd = (torch.tensor(a).float() for a in (X, means, R.full_prec(prec, 128)))
        expanded = (md * md * pd).sum(1) - 2 * Xd @ (md * pd).T + (Xd * Xd) @ pd.T
        direct = -2 * (ref["logp"] - logc)
        e_exp = R.err(expanded.double().numpy(), direct)
        print(f"offset 1000 {ctype}: the expanded form in fp32 is off by {e_exp:.3e} of the largest Mahalanobis term")
        assert e_exp > R.bound(R.FLOOR, e32["lpn"])


def test_estep_far_component_identical_components_and_extreme_precisions():
    N, D, K = 257, 37, 3
    X, means, prec, w, logc, ref, e32 = _case(N, D, K, "diag")
    # one component 1e4 standard deviations away: its responsibilities are exactly 0, nothing is NaN
    far = means.copy()
    far[2] = means[2] + 1e4
    logcf = R.logc64(w, prec, D)
    got = _estep(_dev(X, torch.float32), far, prec, logcf)
    reff = R.estep64(X, far, prec, w)
    assert (got["resp"][:, 2] == 0).all() and np.isfinite(got["resp"]).all() and np.isfinite(got["lpn"]).all()
    assert R.err(got["lpn"], reff["lpn"]) <= R.bound(R.FLOOR, e32["lpn"]) and (got["labels"] != 2).all()
    # two identical components: equal responsibilities bit for bit, the label is the lower index
    twin, ptwin, wtwin = means.copy(), prec.copy(), w.copy()
    twin[1], ptwin[1] = twin[0], ptwin[0]
    wtwin[0] = wtwin[1] = 0.5 * (w[0] + w[1])
    got = _estep(_dev(X, torch.float32), twin, ptwin, R.logc64(wtwin, ptwin, D))
    assert np.array_equal(got["resp"][:, 0], got["resp"][:, 1]) and (got["labels"] != 1).all() and (got["labels"] == 0).any()
    # precisions of 1e6 and 1e-6
    for spread in (1e-3, 1e3):
        Xs, ms, ps, ws, lcs, refs, e32s = _case(N, D, K, "diag", 2, 0.0, spread)
        assert 0.4 / spread ** 2 < ps.min() and ps.max() < 2.1 / spread ** 2
        _check_estep(f"precisions {1 / spread ** 2:.0e}", _estep(_dev(Xs, torch.float32), ms, ps, lcs), refs, e32s, N)


def test_estep_bad_rows_are_counted_and_leave_the_others_alone():
    N, D, K = 300, 37, 3
    X, means, prec, w, logc, ref, e32 = _case(N, D, K, "diag", 3)
    clean = X.copy()
    clean[[5, 200]] = 0.0
    bad = clean.copy()
    bad[5, 7], bad[200, 0] = np.nan, np.inf
    a = _estep(_dev(clean, torch.float32), means, prec, logc)
    b = _estep(_dev(bad, torch.float32), means, prec, logc)
    assert b["estat"][1] == 2 and a["estat"][1] == 0
    for r in (5, 200):
        assert np.isnan(b["lpn"][r]) and np.isnan(b["resp"][r]).all() and b["labels"][r] == -1
    keep = np.ones(N, bool)
    keep[[5, 200]] = False
    for key in ("lpn", "resp", "labels"):
        assert np.array_equal(a[key][keep], b[key][keep]), key
    assert np.isfinite(b["estat"][0]) and abs(b["estat"][0] - b["lpn"][keep].sum()) <= 1e-12 * np.abs(b["lpn"][keep]).sum()


# ------------------------------------------------------------------ the M-step and the parameters
def _mstep_params(Xd, resp, means_old, reg, ctype, n_norm=0, estat=None, guard=False, short=0):
    from vit_som_amd import ops
    N, D = Xd.shape
    K = means_old.shape[0]
    sph = ctype == "spherical"
    handles = []

    def out(shape, dtype):
        if not guard:
            return torch.empty(*shape, dtype=dtype, device="cuda")
        v, h = MC.guarded(shape, dtype, "cuda")
        handles.append(h)
        return v
    rd, mo = _dev(resp, torch.float32), _dev(means_old, torch.float32)
    part = out((ops.gmm_parts(N, D, K, ops.GMM_MSTEP) - short,), torch.float64)
    means, cov, prec = out((K, D), torch.float32), out((K,) if sph else (K, D), torch.float64), out((K, D), torch.float32)
    weights, logc, record = out((K,), torch.float64), out((K,), torch.float64), out((ops.GMM_RECORD,), torch.float64)
    ops.gmm_mstep(Xd, rd, mo, part)
    ops.gmm_params(part, N, mo, reg, sph, n_norm, estat, means, cov, prec, weights, logc, record)
    torch.cuda.synchronize()
    got = dict(means=means.cpu().numpy(), cov=cov.cpu().numpy(), prec=prec.cpu().numpy(), weights=weights.cpu().numpy(),
               logc=logc.cpu().numpy(), record=record.cpu().numpy(), part=part.cpu().numpy())
    return (got, handles) if guard else got


@functools.lru_cache(maxsize=None)
def _soft_resp(N, K, seed=5):
    r = np.random.RandomState(seed).dirichlet(np.ones(K), size=N).astype(np.float32)
    r.setflags(write=False)
    return r


@pytest.mark.parametrize("i", range(len(R.SHAPES)))
def test_mstep_and_params_against_fp64(i):
    N, D, K = R.SHAPES[i]
    ctype = ("diag", "spherical")[i % 2]
    X, means, prec, w, logc, _, _ = _case(N, D, K, ctype)
    resp, reg = _soft_resp(N, K), 1e-6
    nk, mu, cov = R.mstep64(X, resp, reg, ctype)
    nk32, mu32, cov32 = R.mstep32(X, resp, reg, ctype)
    got = _mstep_params(_dev(X, torch.float32), resp, means, reg, ctype)
    wref = nk / nk.sum()
    ref = dict(means=mu, cov=cov, weights=wref, prec=R.full_prec(1.0 / cov, D), logc=R.logc64(wref, 1.0 / cov, D))
    y32 = dict(means=mu32, cov=cov32, weights=nk32 / nk32.sum(), prec=R.full_prec(1.0 / cov32, D),
               logc=R.logc64(nk32 / nk32.sum(), 1.0 / cov32, D))
    for key in ref:
        e_k, e32 = R.err(got[key], ref[key]), R.err(y32[key], ref[key])
        print(f"mstep {N}x{D}x{K} {ctype}: {key} error {e_k:.3e}, plain fp32 {e32:.3e}, bound {R.bound(R.FLOOR, e32):.3e}")
        assert e_k <= R.bound(R.FLOOR, e32)
    rec = got["record"]
    assert np.isnan(rec[0]) and abs(rec[1] - nk.min()) <= 1e-6 * nk.min() and abs(rec[2] - cov.min()) <= R.FLOOR * abs(cov).max()
    assert rec[3] == 0 and rec[4] == 0
    # weights over N, as the initialisation takes them
    init = _mstep_params(_dev(X, torch.float32), resp, means, reg, ctype, n_norm=N)
    assert R.err(init["weights"], nk / N) <= R.FLOOR and np.array_equal(init["means"], got["means"])


def test_mstep_one_hot_gives_cluster_mean_and_variance():
    N, D, K = 1001, 128, 7
    X, means, *_ = _case(N, D, K, "diag")
    label = np.random.RandomState(0).randint(0, K, N)
    resp = np.zeros((N, K), np.float32)
    resp[np.arange(N), label] = 1
    got = _mstep_params(_dev(X, torch.float32), resp, means, 1e-6, "diag")
    X64 = X.astype(np.float64)
    for k in range(K):
        rows = X64[label == k]
        assert np.abs(got["means"][k] - rows.mean(axis=0)).max() <= 1e-6 * np.abs(rows).max()
        assert np.abs(got["cov"][k] - (rows.var(axis=0) + 1e-6)).max() <= 1e-9 * rows.var(axis=0).max()
        assert abs(got["weights"][k] - len(rows) / N) <= 1e-12


def test_mstep_empty_component_keeps_its_mean():
    N, D, K = 257, 37, 3
    X, means, *_ = _case(N, D, K, "diag")
    resp = _soft_resp(N, K).copy()
    resp[:, 1] = 0.0
    for ctype in ("diag", "spherical"):
        got = _mstep_params(_dev(X, torch.float32), resp, means, 1e-3, ctype)
        assert np.array_equal(got["means"][1], means[1])                    # sklearn would move it to 0 / tiny
        assert np.abs(got["cov"][1] - 1e-3).max() <= 1e-17 and got["record"][1] == EPS10 and got["record"][3] == 0
        assert abs(got["weights"][1] / (EPS10 / resp.astype(np.float64).sum()) - 1) <= 1e-12


def test_params_count_a_collapsed_component():
    """reg_covar = 0 and a component that holds one row twice, shifted at that row: its spherical covariance is exactly 0."""
    N, D, K = 63, 5, 2
    X, means, *_ = _case(N, D, K, "spherical")
    X = X.copy()
    X[1] = X[0]
    resp = np.zeros((N, K), np.float32)
    resp[:, 0] = 1
    resp[[0, 1], 0], resp[[0, 1], 1] = 0, 1
    old = means.copy()
    old[1] = X[0]
    got = _mstep_params(_dev(X, torch.float32), resp, old, 0.0, "spherical")
    assert got["record"][3] == 1 and got["record"][2] == 0 and got["cov"][1] == 0 and got["cov"][0] > 0
    assert np.array_equal(got["means"][1], X[0])


def test_mstep_slabs_follow_the_rule_and_repeat_bit_for_bit():
    from vit_som_amd import ops
    N, D, K = 1000, 129, 16
    X, means, *_ = _case(N, D, K, "diag")
    resp = _soft_resp(N, K)
    rows = ops.gmm_slab_rows(N, D, K)
    S = -(-N // rows)
    assert S > 1 and rows == ops.gmm_slab_rows(N, D, K)
    runs = [_mstep_params(_dev(X, torch.float32), resp, means, 1e-6, "diag") for _ in range(3)]
    for r in runs[1:]:
        for key in ("means", "cov", "prec", "weights", "logc"):
            assert np.array_equal(r[key], runs[0][key]), key
        assert np.array_equal(r["part"][:S * K * (2 * D + 1)], runs[0]["part"][:S * K * (2 * D + 1)])
    # the slabs are the contiguous row ranges of the rule: [S][K][2][D] sums, then [S][K] counts
    part = runs[0]["part"]
    s12, nks = part[:S * K * 2 * D].reshape(S, K, 2, D), part[S * K * 2 * D:S * K * (2 * D + 1)].reshape(S, K)
    for s in (0, S - 1):
        sl = slice(s * rows, min(N, (s + 1) * rows))
        d = X[sl, None, :].astype(np.float64) - means[None].astype(np.float64)
        r = resp[sl].astype(np.float64)
        assert np.abs(nks[s] - r.sum(axis=0)).max() <= 1e-12 * r.sum(axis=0).max()
        s1, s2 = np.einsum("nk,nkd->kd", r, d), np.einsum("nk,nkd->kd", r, d * d)
        assert np.abs(s12[s, :, 0] - s1).max() <= 1e-12 * np.abs(s1).max() + 1e-12
        assert np.abs(s12[s, :, 1] - s2).max() <= 1e-12 * np.abs(s2).max()


# ------------------------------------------------------------------ the memory contract
@pytest.mark.parametrize("N,D,K,ctype", [(257, 37, 3, "diag"), (1000, 129, 16, "spherical"), (130, 10, 1024, "diag")])
def test_memory_contract(N, D, K, ctype):
    from vit_som_amd import ops
    from vit_som_amd._lib import VsomError
    X, means, prec, w, logc, ref, e32 = _case(N, D, K, ctype)
    Xg, hx = MC.guarded_copy(torch.tensor(X).cuda(), ld=D + 3)
    got, handles = _estep(Xg, means, prec, logc, guard=True, ldr=K + 1)
    for h in handles[:-1]:
        h.check(); h.all_written()
    handles[-1].check()                                   # the scratch: exactly the queried count, guards intact
    hx.check()
    _check_estep(f"guarded {N}x{D}x{K}", got, ref, e32, N)
    got, handles = _mstep_params(Xg, _soft_resp(N, K), means, 1e-6, ctype, guard=True)
    for h in handles[1:]:
        h.check(); h.all_written()
    handles[0].check()
    hx.check()
    assert np.isfinite(got["means"]).all() and np.isfinite(got["cov"]).all() and got["record"][3] == 0
    # one element short: refused on the host
    short = torch.empty(ops.gmm_parts(N, D, K, ops.GMM_ESTEP) - 1, dtype=torch.float64, device="cuda")
    with pytest.raises(VsomError, match="too small"):
        ops.gmm_estep(Xg, _dev(means, torch.float32), _dev(R.full_prec(prec, D), torch.float32), _dev(logc, torch.float64), None,
                      _f64(N), None, _f64(2), short)
    with pytest.raises(VsomError, match="too small"):
        _mstep_params(Xg, _soft_resp(N, K), means, 1e-6, ctype, short=1)
    with pytest.raises(VsomError, match="too small"):
        ops.gmm_set_params(_f64(K), _f64(K) if ctype == "spherical" else _f64(K, D), D, ctype == "spherical",
                           torch.empty(K, D, device="cuda"), _f64(K), _f64(ops.GMM_RECORD), _f64(ops.gmm_parts(1, D, K, ops.GMM_SET) - 1))


# ------------------------------------------------------------------ whole fits against sklearn
def _fit(X, k, **kw):
    from vit_som_amd import GaussianMixture
    from vit_som_amd.gmm import ConvergenceWarning
    with warnings.catch_warnings():
        warnings.simplefilter("error", category=ConvergenceWarning)
        return GaussianMixture(k, **kw).fit(_dev(X, torch.float32))


@pytest.mark.parametrize("i", range(len(R.FIXTURES)))
def test_whole_fit_from_means_init_matches_sklearn(i):
    X, init, k, ctype = R.blobs(i)
    X64 = X.astype(np.float64)
    sk = R.sklearn_fit(i)
    gm = _fit(X, k, covariance_type=ctype, tol=R.TOL, means_init=init, random_state=R.FIXTURES[i][0])
    emu = R.fit32_emulated(X, R.kmeans_resp(i), ctype, means_init=init)
    print(f"fixture {i}: n_iter device {gm.n_iter_} sklearn {sk.n_iter_} emulation {emu['n_iter']}; lower bounds device "
          f"{gm.lower_bounds_} sklearn {sk.lower_bounds_}")
    assert gm.n_iter_ == sk.n_iter_ and gm.converged_ == sk.converged_ and len(gm.lower_bounds_) == gm.n_iter_
    gap = abs(emu["lower_bounds"][-1] - sk.lower_bound_) / abs(sk.lower_bound_)
    e_k = abs(gm.lower_bound_ - sk.lower_bound_) / abs(sk.lower_bound_)
    print(f"fixture {i}: lower bound error {e_k:.3e}, emulation {gap:.3e}")
    assert e_k <= R.bound(R.FLOOR, gap) and gm.lower_bound_ == gm.lower_bounds_[-1]
    for name, ref, y32 in (("weights_", sk.weights_, emu["weights"]), ("means_", sk.means_, emu["means"]),
                           ("covariances_", sk.covariances_, emu["cov"])):
        e_k, e32 = R.err(getattr(gm, name), ref), R.err(y32, ref)
        print(f"fixture {i}: {name} error {e_k:.3e}, emulation {e32:.3e}")
        assert e_k <= R.bound(R.FLOOR, e32)
    assert R.err(gm.precisions_, sk.precisions_) <= 10 * R.FLOOR and R.err(gm.precisions_cholesky_, sk.precisions_cholesky_) <= 10 * R.FLOOR
    # predict where sklearn's own top-two gap is clear
    wlp = np.sort(sk._estimate_weighted_log_prob(X64), axis=1)
    clear = (wlp[:, -1] - wlp[:, -2]) > R.GAP
    assert (~clear).mean() <= R.MAX_UNCLEAR
    Xd = _dev(X, torch.float32)
    assert np.array_equal(gm.predict(Xd).cpu().numpy()[clear], sk.predict(X64)[clear])
    assert np.array_equal(gm.fit_predict(Xd).cpu().numpy()[clear], sk.predict(X64)[clear])
    # score, bic and aic at the fitted parameters; the yardstick: plain fp32 at sklearn's parameters
    lpn32, _ = R.estep32(X, sk.means_, sk.precisions_, R.logc64(sk.weights_, sk.precisions_, X.shape[1]))
    e32 = abs(lpn32.mean() - sk.score(X64)) / abs(sk.score(X64))
    for name in ("score", "bic", "aic"):
        got, ref = getattr(gm, name)(Xd), getattr(sk, name)(X64)
        print(f"fixture {i}: {name} {got:.6f} sklearn {ref:.6f}, plain fp32 {e32:.3e}")
        assert isinstance(got, float) and abs(got - ref) <= R.bound(R.FLOOR, e32) * abs(ref)
    assert gm._n_parameters() == sk._n_parameters() and gm.n_features_in_ == X.shape[1]
    sc = gm.score_samples(Xd)
    assert sc.dtype == torch.float64 and sc.is_cuda and R.err(sc, sk.score_samples(X64)) <= R.bound(R.FLOOR, e32)
    proba = gm.predict_proba(Xd)
    assert proba.shape == (X.shape[0], k) and R.err(proba, sk.predict_proba(X64)) <= 1e-3


# ------------------------------------------------------------------ the estimator's behaviour
@functools.lru_cache(maxsize=None)
def _kmeans_blobs():
    from test_kmeans_gpu import _blobs_f32
    X, _ = _blobs_f32(5, 6000, 48, 8, 2.0)
    X.setflags(write=False)
    return X


def test_kmeans_init_gives_sklearns_fit():
    from sklearn.mixture import GaussianMixture as SK
    X = _kmeans_blobs()
    sk = SK(8, covariance_type="diag", random_state=0).fit(X.astype(np.float64))
    gm = _fit(X, 8, random_state=0)
    print(f"kmeans init: n_iter {gm.n_iter_} / {sk.n_iter_}, weights error {R.err(gm.weights_, sk.weights_):.3e}")
    assert gm.n_iter_ == sk.n_iter_ and gm.converged_ and R.err(gm.weights_, sk.weights_) <= R.FLOOR
    assert R.err(gm.means_, sk.means_) <= R.FLOOR


@pytest.mark.parametrize("init", ["k-means++", "random_from_data", "random"])
def test_other_inits_start_where_sklearn_starts(init):
    from sklearn.mixture import GaussianMixture as SK
    X = _kmeans_blobs()[:1500]
    sk = SK(5, covariance_type="diag", init_params=init, random_state=3, max_iter=0).fit(X.astype(np.float64))
    gm = _fit(X, 5, init_params=init, random_state=3, max_iter=0)
    assert gm.n_iter_ == 0 and not gm.converged_ and gm.lower_bound_ == -np.inf and gm.lower_bounds_ == []
    assert R.err(gm.means_, sk.means_) <= R.FLOOR and R.err(gm.covariances_, sk.covariances_) <= 10 * R.FLOOR
    assert R.err(gm.weights_, sk.weights_) <= R.FLOOR
    if init != "random":                                   # the means are rows of X
        d = np.abs(gm.means_.cpu().numpy()[:, None, :] - X[None]).max(axis=2).min(axis=1)
        assert (d <= 1e-5).all()


def test_fits_are_reproducible_and_n_init_keeps_the_best():
    from vit_som_amd import GaussianMixture
    X = _dev(_kmeans_blobs()[:2000], torch.float32)
    names = ("weights_", "means_", "covariances_", "precisions_", "precisions_cholesky_")
    a = GaussianMixture(6, init_params="random", n_init=3, random_state=7, max_iter=15, tol=1e-2)
    b = GaussianMixture(6, init_params="random", n_init=3, random_state=7, max_iter=15, tol=1e-2)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        la, lb = a.fit_predict(X), b.fit_predict(X)
        rs = np.random.RandomState(7)
        singles = [GaussianMixture(6, init_params="random", random_state=rs, max_iter=15, tol=1e-2).fit(X) for _ in range(3)]
    assert torch.equal(la, lb) and all(torch.equal(getattr(a, n), getattr(b, n)) for n in names)
    assert (a.n_iter_, a.converged_, a.lower_bound_, a.lower_bounds_) == (b.n_iter_, b.converged_, b.lower_bound_, b.lower_bounds_)
    best = max(singles, key=lambda g: g.lower_bound_)
    assert a.lower_bound_ == best.lower_bound_ and a.n_iter_ == best.n_iter_ and torch.equal(a.means_, best.means_)
    assert a.lower_bounds_ == best.lower_bounds_ and len({g.lower_bound_ for g in singles}) > 1


def test_max_iter_zero_warm_start_and_the_warning():
    from vit_som_amd import GaussianMixture
    from vit_som_amd.gmm import NOT_CONVERGED, ConvergenceWarning
    X, init, k, ctype = R.blobs(0)
    Xd = _dev(X, torch.float32)
    g0 = _fit(X, k, means_init=init, random_state=0, max_iter=0)            # no warning: _fit turns warnings into errors
    assert torch.equal(g0.means_.cpu(), torch.tensor(init)) and g0.n_iter_ == 0 and not g0.converged_
    whole = _fit(X, k, means_init=init, random_state=0)
    assert whole.n_iter_ == 5
    warm = GaussianMixture(k, means_init=init, random_state=0, max_iter=2, warm_start=True)
    with pytest.warns(ConvergenceWarning) as rec:
        warm.fit(Xd)
    assert [str(r.message) for r in rec if issubclass(r.category, ConvergenceWarning)] == [NOT_CONVERGED] and warm.n_iter_ == 2 and warm.lower_bounds_ == whole.lower_bounds_[:2]
    with pytest.warns(ConvergenceWarning):
        warm.fit(Xd)                                                        # continues: iterations 3 and 4
    assert warm.lower_bounds_ == whole.lower_bounds_[2:4] and warm.n_iter_ == 2
    warm.max_iter = 10
    warm.fit(Xd)
    assert warm.converged_ and warm.lower_bounds_ == whole.lower_bounds_[4:] and torch.equal(warm.means_, whole.means_)


def test_errors_carry_their_sentences():
    from vit_som_amd import GaussianMixture
    from vit_som_amd.gmm import BAD_COVARIANCE
    X, init, k, ctype = R.blobs(0)
    bad = X.copy()
    bad[3, 2], bad[77, 0], bad[78, 5] = np.nan, np.inf, -np.inf
    with pytest.raises(ValueError, match="3 rows of X hold NaN or infinity"):
        GaussianMixture(k, means_init=init, init_params="random", random_state=0).fit(_dev(bad, torch.float32))
    g = _fit(X, k, means_init=init, random_state=0)
    with pytest.raises(ValueError, match="3 rows of X hold NaN or infinity"):
        g.predict(_dev(bad, torch.float32))
    flat = X.copy()
    flat[:, 4] = 3.0                                                        # a constant column and no regularisation
    with pytest.raises(ValueError) as e:
        GaussianMixture(k, reg_covar=0.0, init_params="random", random_state=0).fit(_dev(flat, torch.float32))
    assert str(e.value) == BAD_COVARIANCE and "ill-defined empirical covariance" in BAD_COVARIANCE
    with pytest.raises(ValueError, match="Expected n_samples >= n_components but got n_components = 9, n_samples = 8"):
        GaussianMixture(9).fit(_dev(X[:8], torch.float32))
    with pytest.raises(ValueError, match=r"The parameter 'means' should have the shape of \(5, 20\), but got \(4, 20\)"):
        GaussianMixture(k, means_init=init[:4]).fit(_dev(X, torch.float32))
    with pytest.raises(ValueError, match=r"The parameter 'weights' should have the shape of \(5,\), but got \(3,\)"):
        GaussianMixture(k, weights_init=np.ones(3) / 3).fit(_dev(X, torch.float32))
    with pytest.raises(ValueError, match=r"The parameter 'diag precision' should have the shape of \(5, 20\), but got \(5,\)"):
        GaussianMixture(k, precisions_init=np.ones(5)).fit(_dev(X, torch.float32))
    # weights_init and precisions_init are taken as given
    w0, p0 = np.array([0.1, 0.2, 0.3, 0.2, 0.2]), np.full((5, 20), 0.25)
    g = _fit(X, k, means_init=init, weights_init=w0, precisions_init=p0, max_iter=0)
    assert np.array_equal(g.weights_.cpu().numpy(), w0) and np.allclose(g.precisions_.cpu().numpy(), p0, rtol=1e-15)


# ------------------------------------------------------------------ evaluate_gmm and the driver
def test_evaluate_gmm_vitsom_and_desom():
    from sklearn.metrics import normalized_mutual_info_score
    from sklearn.mixture import GaussianMixture as SK
    from test_evaluation import purity_reference_loop
    from test_kmeans_gpu import _models, _separable_images
    from vit_som_amd import GaussianMixture, GMMReport, evaluate_gmm
    for m, cfg in _models():
        d = cfg["data"]
        vit = cfg["hyperparameters"]["model_arch"] == "vit_som"
        batches = _separable_images(5, 12, 4, d["num_channels"], d["input_size"], 8)
        test = _separable_images(6, 4, 4, d["num_channels"], d["input_size"], 8)
        feats, ys = [], []
        for x, y in batches:
            f = m.get_latent_representation(x.cuda()) if vit else m(x.cuda().reshape(x.shape[0], -1))[1]
            feats.append(f.reshape(f.shape[0], -1).float().clone()); ys.append(y.numpy())
        feats, ys = torch.cat(feats), np.concatenate(ys)
        m.train(True)
        rep = evaluate_gmm(m, cfg, batches, n_components=4, test_loader=test)
        assert m.training and isinstance(rep, GMMReport) and rep.n_samples == len(ys) == 48 and rep.n_components == 4
        start = GaussianMixture(4, random_state=0, max_iter=0).fit(feats).means_.cpu().numpy().astype(np.float64)
        pred = SK(4, covariance_type="diag", means_init=start, random_state=0).fit_predict(feats.cpu().numpy().astype(np.float64))
        p_ref, n_ref = purity_reference_loop(ys, pred)[0], normalized_mutual_info_score(ys, pred)
        print(f"{cfg['hyperparameters']['model_arch']}: purity {rep.purity} / {p_ref}, nmi {rep.nmi} / {n_ref}, {rep.n_iter} iterations")
        assert abs(rep.purity - p_ref) < 1e-12 and abs(rep.nmi - n_ref) < 1e-10
        assert rep.bic_curve == [(4, rep.bic)] and rep.aic < rep.bic and np.isfinite(rep.log_likelihood)
        assert np.isfinite(rep.test_log_likelihood) and 0.25 <= rep.mean_confidence <= 1.0
        assert rep.weights.shape == (4,) and abs(rep.weights.sum() - 1) < 1e-12 and rep.fit_time > 0 and rep.inference_time > 0
        curve = evaluate_gmm(m, cfg, batches, n_components=[2, 4, 6])
        assert [k for k, _ in curve.bic_curve] == [2, 4, 6] and curve.test_log_likelihood is None
        assert curve.n_components == min(curve.bic_curve, key=lambda kb: kb[1])[0] and curve.bic == min(b for _, b in curve.bic_curve)
        m.world_size = 2
        with pytest.raises(ValueError, match="world_size > 1"):
            evaluate_gmm(m, cfg, batches, n_components=4)
        m.world_size = 1


def test_driver_reports_the_mixture(tmp_path):
    from helpers import load_golden
    from vit_som_amd.train import main, synthetic_loaders
    _, cfg = load_golden("ref_cluster_tiny")
    cfg = copy.deepcopy(cfg)
    cfg["hyperparameters"]["batch_size"] = 16
    logs = []
    loaders = lambda c, r, w: synthetic_loaders(c, r, w, n_train=64, n_val=16, n_test=16)      # noqa: E731
    today = {"accuracy", "precision", "recall", "f1", "purity", "nmi", "run_duration", "inference_time"}
    met = main(cfg, n_runs=1, max_epochs=1, make_loaders=loaders, model_states_dir=str(tmp_path / "a"), log=logs.append, gmm_eval=True)
    assert set(met) == today | {"gmm_purity", "gmm_nmi", "gmm_bic"}
    (p,), (n,), (b,) = met["gmm_purity"], met["gmm_nmi"], met["gmm_bic"]
    assert 0.0 < p <= 1.0 and 0.0 <= n <= 1.0 + 1e-12 and np.isfinite(b)
    assert any("Gaussian mixture: purity" in l for l in logs)
