"""Gaussian mixtures without a GPU: the fp64 restatements of gmm_ref.py against sklearn's private functions, the C-ABI
wiring of the new entries and their host-side refusals, the estimator's surface, and the condition the whole-fit fixtures of
test_gmm_gpu.py rest on (no step of sklearn's lower bound lies near tol)."""
import inspect
import os
import re

import numpy as np
import pytest

import gmm_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("vsom_gmm_parts", "vsom_gmm_slab_rows", "vsom_gmm_estep", "vsom_gmm_mstep", "vsom_gmm_params", "vsom_gmm_set_params")
WRAPPERS = ("gmm_parts", "gmm_slab_rows", "gmm_estep", "gmm_mstep", "gmm_params", "gmm_set_params")
P = 4096                    # stands for a non-null, 16-byte aligned device pointer: nothing is launched, nothing dereferenced
BIG = 1 << 40


# ------------------------------------------------------------------ the restatements against sklearn
@pytest.mark.parametrize("ctype", ["diag", "spherical"])
def test_fp64_restatement_equals_sklearn(ctype):
    from sklearn.mixture import _gaussian_mixture as G
    for N, D, K in [(257, 37, 3), (400, 129, 16)]:
        X32, means32, prec, w = R.mixture_case(N, D, K, ctype, seed=1)
        X, means = X32.astype(np.float64), means32.astype(np.float64)
        ref = G._estimate_log_gaussian_prob(X, means, np.sqrt(prec), ctype)
        got = R.log_gaussian64(X, means, prec)
        assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()
        e = R.estep64(X, means, prec, w)
        assert np.abs(e["lpn"] - R.logsumexp(ref + np.log(w))).max() <= 1e-12 * np.abs(e["lpn"]).max()
        resp = np.random.RandomState(3).dirichlet(np.ones(K), size=N)
        nk, mu, cov = R.mstep64(X, resp, 1e-6, ctype)
        nk_s, mu_s, cov_s = G._estimate_gaussian_parameters(X, resp, 1e-6, ctype)
        assert np.abs(nk - nk_s).max() <= 1e-12 * nk_s.max() and np.abs(mu - mu_s).max() <= 1e-12 * np.abs(mu_s).max()
        assert np.abs(cov - cov_s).max() <= 1e-12 * np.abs(cov_s).max()
        chol = G._compute_precision_cholesky(cov_s, ctype)
        assert np.abs(1.0 / np.sqrt(cov) - chol).max() <= 1e-12 * np.abs(chol).max()
        assert np.abs(R.logc64(w, 1.0 / cov, D) - (np.log(w) + np.log(R.full_prec(chol, D)).sum(axis=1) - 0.5 * D * R.LOG_2PI)).max() \
            <= 1e-12 * D


@pytest.mark.parametrize("i", range(len(R.FIXTURES)))
def test_fixture_condition_and_the_loop_restatement(i):
    """sklearn's fp64 lower bounds have no step with |change| inside [tol / 2, 2 tol]: the device comparison of n_iter_ is
    not marginal.  And the fp64 loop and the f32 emulation of the device solver, from sklearn's own start, stop where
    sklearn stops."""
    sk = R.sklearn_fit(i)
    assert sk.converged_ and len(sk.lower_bounds_) == sk.n_iter_
    assert sk.n_iter_ == (5, 4, 5)[i]
    changes = np.abs(np.diff(np.concatenate([[-np.inf], sk.lower_bounds_])))
    print(f"fixture {i}: n_iter {sk.n_iter_}, |changes| {changes}")
    assert not ((changes >= R.TOL / 2) & (changes <= 2 * R.TOL)).any(), changes
    X, init, k, ctype = R.blobs(i)
    f64 = R.fit64(X, R.kmeans_resp(i), ctype, means_init=init)
    assert f64["n_iter"] == sk.n_iter_ and f64["converged"]
    assert np.abs(np.array(f64["lower_bounds"]) - sk.lower_bounds_).max() <= 1e-9 * abs(sk.lower_bound_)
    f32 = R.fit32_emulated(X, R.kmeans_resp(i), ctype, means_init=init)
    assert f32["n_iter"] == sk.n_iter_ and f32["converged"]
    gap = abs(f32["lower_bounds"][-1] - sk.lower_bound_)
    print(f"fixture {i}: lower bound {sk.lower_bound_:.6f}, f32 emulation off by {gap:.3e}")
    assert gap <= R.FLOOR * abs(sk.lower_bound_)


def test_plain_fp32_yardstick_is_not_vacuous():
    for N, D, K in R.SHAPES:
        X, means, prec, w = R.mixture_case(N, D, K)
        e = R.estep64(X, means, prec, w)
        lpn32, resp32 = R.estep32(X, means, prec, R.logc64(w, prec, D))
        e_lpn, e_resp = R.err(lpn32, e["lpn"]), R.err(resp32, e["resp"])
        print(f"{N}x{D}x{K}: plain fp32 is off by {e_lpn:.2e} (log_prob_norm), {e_resp:.2e} (resp); median largest resp "
              f"{np.median(e['resp'].max(axis=1)):.3f}")
        assert e_lpn <= R.E32_MAX and e_resp <= 2e-3       # resp: 12 288 terms of f32 rounding on log p near -17 000
        assert K == 1 or N < 64 or np.median(e["resp"].max(axis=1)) < 0.99          # the responsibilities are soft
        assert (e["gap"] <= R.GAP).mean() <= R.MAX_UNCLEAR


# ------------------------------------------------------------------ wiring
def _header():
    src = open(os.path.join(ROOT, "include", "vitsom_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_entries_are_declared_bound_exported_and_wrapped():
    import ctypes
    from vit_som_amd import _lib, ops
    src = _header()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        assert re.search(rf"\b{name}\s*\(", src), f"{name} is not declared in include/vitsom_hip.h"
        assert name in _lib.SIGNATURES and hasattr(raw, name)
    for name in WRAPPERS:
        assert callable(getattr(ops, name)) and getattr(ops, name).__doc__
    build = open(os.path.join(ROOT, "vit_som_amd", "csrc", "build.sh")).read()
    compile_list = re.search(r"for f in ([^;]*);", build).group(1).split()
    link_list = re.search(r"obj/\{([^}]*)\}\.o", build).group(1).split(",")
    assert "gmm" in compile_list and "gmm" in link_list
    assert os.path.exists(os.path.join(ROOT, "vit_som_amd", "csrc", "gmm.hip"))


def test_scratch_is_typed_not_byte_sized():
    src = _header()
    for name in ENTRIES:
        params = re.search(rf"\b{name}\s*\(([^)]*)\)", src).group(1)
        for bad in ("ws_bytes", "part_bytes", "planes_bytes", "scratch_bytes", "void"):
            assert not re.search(rf"\b{bad}\b", params), (name, bad)
    for name in ("vsom_gmm_estep", "vsom_gmm_mstep", "vsom_gmm_params", "vsom_gmm_set_params"):
        assert re.search(r"double\*\s*part,\s*long n_part", re.search(rf"\b{name}\s*\(([^)]*)\)", src).group(1)), name


def test_size_queries_are_host_arithmetic():
    from vit_som_amd import ops
    for which in (ops.GMM_ESTEP, ops.GMM_MSTEP, ops.GMM_SET):
        for shape in [(0, 8, 3), (8, 0, 3), (8, 8, 0), (-1, 8, 3), (8, 8, 1025)]:
            assert ops.gmm_parts(*shape, which) == 0
        assert ops.gmm_parts(300, 12288, 10, which) > 0
    assert ops.gmm_parts(3, 8, 2, 7) == 0 and ops.gmm_slab_rows(0, 8, 3) == 0
    # the E-step: two doubles per workgroup and 32 staging rows of K; the M-step: slabs of [K][2][D] + [K], the diag
    # covariances, four numbers per component
    assert ops.gmm_parts(70, 8, 3, ops.GMM_ESTEP) == 3 * (2 + 32 * 3)
    rows = ops.gmm_slab_rows(70, 8, 3)
    slabs = -(-70 // rows)
    assert ops.gmm_parts(70, 8, 3, ops.GMM_MSTEP) == slabs * 3 * (2 * 8 + 1) + 3 * 8 + 3 * 4
    assert ops.gmm_parts(1, 8, 3, ops.GMM_SET) == 12
    # the slab budget bounds the scratch at large K * D
    assert ops.gmm_parts(50000, 12288, 1024, ops.GMM_MSTEP) * 8 <= (256 << 20) + 1024 * 12288 * 8 * 3


def test_host_refusals_without_a_launch():
    from vit_som_amd import ops
    from vit_som_amd._lib import last_error, lib as L
    N, D, K = 70, 8, 3
    ne, nm, ns = (ops.gmm_parts(N, D, K, w) for w in (ops.GMM_ESTEP, ops.GMM_MSTEP, ops.GMM_SET))

    def estep(X=P, ldx=D, N=N, D=D, means=P, prec=P, logc=P, K=K, resp=P, ldr=K, lpn=P, labels=P, estat=P, part=P, n=ne):
        return L.vsom_gmm_estep(X, ldx, N, D, means, prec, logc, K, resp, ldr, lpn, labels, estat, part, n, None)

    def mstep(X=P, ldx=D, N=N, D=D, resp=P, ldr=K, mu=P, K=K, part=P, n=nm):
        return L.vsom_gmm_mstep(X, ldx, N, D, resp, ldr, mu, K, part, n, None)

    def params(part=P, n=nm, N=N, D=D, K=K, mu_old=P, estat=P, means=2 * P, cov=P, prec=P, w=P, logc=P, rec=P):
        return L.vsom_gmm_params(part, n, N, D, K, mu_old, 1e-6, 0, 0, estat, means, cov, prec, w, logc, rec, None)

    def setp(w=P, cov=P, D=D, K=K, prec=P, logc=P, rec=P, part=P, n=ns):
        return L.vsom_gmm_set_params(w, cov, D, K, 0, prec, logc, rec, part, n, None)

    for call in (estep, mstep):
        assert call(X=None) == -1 and "null" in last_error()
        assert call(N=0) == -1 and call(D=0) == -1 and call(K=0) == -1 and call(N=-5) == -1
        assert call(ldx=D - 1) == -1 and "ldx" in last_error()
        assert call(K=1025, ldr=1025, n=BIG) == -3 and "1024" in last_error()
        need = ne if call is estep else nm
        assert call(n=need - 1) == -4 and "part" in last_error() and "too small" in last_error()
        assert call(part=None, n=BIG) == -4 and call(n=0) == -4
    assert estep(ldr=K - 1) == -1 and mstep(ldr=K - 1) == -1
    for name in ("means", "prec", "logc", "lpn", "estat"):
        assert estep(**{name: None}) == -1, name
    assert mstep(resp=None) == -1 and mstep(mu=None) == -1
    for name in ("mu_old", "means", "cov", "prec", "w", "logc", "rec"):
        assert params(**{name: None}) == -1, name
    assert params(means=P) == -1 and "alias" in last_error()
    assert params(N=0) == -1 and params(D=0) == -1 and params(K=0) == -1 and params(K=1025, n=BIG) == -3
    assert params(n=nm - 1) == -4 and params(part=None, n=BIG) == -4
    for name in ("w", "cov", "prec", "logc", "rec"):
        assert setp(**{name: None}) == -1, name
    assert setp(D=0) == -1 and setp(K=0) == -1 and setp(K=1025, n=BIG) == -3
    assert setp(n=ns - 1) == -4 and setp(part=None, n=BIG) == -4


# ------------------------------------------------------------------ the estimator's surface
def test_constructor_signature_and_defaults():
    import vit_som_amd
    from vit_som_amd import gmm
    assert vit_som_amd.GaussianMixture is gmm.GaussianMixture
    sig = inspect.signature(gmm.GaussianMixture.__init__)
    assert str(sig) == ("(self, n_components=1, *, covariance_type='diag', tol=0.001, reg_covar=1e-06, max_iter=100, n_init=1, "
                        "init_params='kmeans', weights_init=None, means_init=None, precisions_init=None, random_state=None, "
                        "warm_start=False)")
    # sklearn's own, but for the default covariance type
    from sklearn.mixture import GaussianMixture as SK
    ref = inspect.signature(SK.__init__).parameters
    for name, p in sig.parameters.items():
        if name == "self":
            continue
        assert p.kind == ref[name].kind and (p.default == ref[name].default or name == "covariance_type"), name
    assert set(sig.parameters) - {"self"} == set(ref) - {"self", "verbose", "verbose_interval"}
    for m in ("fit", "fit_predict", "predict", "predict_proba", "score_samples", "score", "bic", "aic"):
        assert callable(getattr(gmm.GaussianMixture, m))
    assert not hasattr(gmm.GaussianMixture, "sample")
    assert "diag" in gmm.GaussianMixture.__doc__ and "full" in gmm.GaussianMixture.__doc__


@pytest.mark.parametrize("ctype", ["full", "tied"])
def test_full_and_tied_are_refused_with_the_reason(ctype):
    from vit_som_amd import GaussianMixture
    with pytest.raises(NotImplementedError) as e:
        GaussianMixture(3, covariance_type=ctype)
    msg = str(e.value)
    assert "D x D" in msg and "12 288" in msg and "PCA(n).fit_transform" in msg and "'diag'" in msg


def test_unknown_covariance_type_raises_sklearns_error():
    from sklearn.mixture import GaussianMixture as SK
    from vit_som_amd import GaussianMixture
    with pytest.raises(ValueError) as ref:
        SK(2, covariance_type="foo").fit(np.zeros((4, 2)))
    with pytest.raises(ValueError) as got:
        GaussianMixture(2, covariance_type="foo")
    # sklearn prints the options as a set, in an order that changes from process to process
    norm = lambda s: re.sub(r"\{[^}]*\}", lambda m: "{" + ", ".join(sorted(m.group(0)[1:-1].split(", "))) + "}", s)     # noqa: E731
    assert norm(str(got.value)) == norm(str(ref.value))


def test_n_parameters_follow_sklearn():
    from sklearn.mixture import GaussianMixture as SK
    from vit_som_amd import GaussianMixture
    import torch
    for ctype in ("diag", "spherical"):
        sk, gm = SK(4, covariance_type=ctype), GaussianMixture(4, covariance_type=ctype)
        sk.means_ = np.zeros((4, 9))
        gm.means_ = torch.zeros(4, 9)
        assert gm._n_parameters() == sk._n_parameters()


def test_driver_and_entry_live_where_the_surface_test_expects():
    from vit_som_amd import evaluate_gmm, evaluation, gmm, train
    assert inspect.signature(train.main).parameters["gmm_eval"].default is False
    assert list(inspect.signature(train.main).parameters)[-1] == "gmm_eval"
    assert evaluate_gmm.__module__ == "vit_som_amd.gmm" and gmm.GMMReport.__module__ == "vit_som_amd.gmm"
    assert evaluation.evaluate_gmm is evaluate_gmm
    assert str(inspect.signature(evaluate_gmm)) == ("(model, config, dataloader, n_components=None, covariance_type='diag', "
                                                    "num_labels=None, max_rows=None, n_init=1, random_state=0, test_loader=None)")
    assert train._parser().parse_args(["--config", "c", "--gmm-eval"]).gmm_eval is True
