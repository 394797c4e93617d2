"""sklearn.mixture.GaussianMixture (sklearn/mixture/_base.py, _gaussian_mixture.py) on the device, for diagonal and
spherical covariances, and evaluate_gmm, the evaluation entry built on it (no counterpart in the reference).

Every step that touches the data is a HIP kernel (csrc/gmm.hip): the E-step (log densities in the DIRECT form
sum_d (x - mu)^2 p, the fp64 log-sum-exp, responsibilities, labels), the M-step's partial sums shifted at the previous
means, and the parameter pass (means, covariances, precisions, weights, log constants, one status record).  The host
keeps what sklearn decides with small numbers: the draws of one ``np.random.RandomState`` shared by all ``n_init`` runs,
and BaseMixture.fit_predict's loop -- ``lower_bound = -inf``, ``change = lower_bound - prev``, ``abs(change) < tol`` --
on the eight-number record it reads ONCE per iteration.  The features never leave the device; a fit is bitwise reproducible.

Departures from sklearn, all stated here and in INTEGRATION.md:
* ``covariance_type`` defaults to "diag" (sklearn: "full"); "full" and "tied" raise NotImplementedError.
* The log densities use the direct form, not sklearn's expansion sum mu^2 p - 2 x.mu p + x^2.p, which cancels in fp32 at
  D = 12 288 when the column means are large against the spread.
* A component whose responsibilities are all zero keeps its old mean (sklearn moves it to 0 / tiny); its covariance becomes
  ``reg_covar`` as in sklearn.
* ``sample`` is not provided.
"""
import math
import numbers
import time
import warnings
from dataclasses import dataclass

import numpy as np
import torch

from . import ops
from .kmeans import KMeans, _kmeans_plusplus, _random_state
from .pca import NotFittedError

_TYPES = ("spherical", "tied", "diag", "full")
_INITS = ("kmeans", "k-means++", "random", "random_from_data")
BAD_COVARIANCE = ("Fitting the mixture model failed because some components have ill-defined empirical covariance (for instance "
                  "caused by singleton or collapsed samples). Try to decrease the number of components, increase reg_covar, or "
                  "scale the input data.")
NOT_CONVERGED = ("Best performing initialization did not converge. Try different init parameters, or increase max_iter, tol, or "
                 "check for degenerate data.")


class ConvergenceWarning(UserWarning):
    """The best initialisation stopped at max_iter (sklearn.exceptions.ConvergenceWarning is a UserWarning too)."""


def _options(values):
    return "{" + ", ".join(repr(v) for v in values) + "}"


def _check_covariance_type(covariance_type):
    if covariance_type in ("full", "tied"):
        raise NotImplementedError(
            f"GaussianMixture: covariance_type={covariance_type!r} is not implemented: it needs D x D matrices per component, "
            f"1.2 GB each in fp64 at the latent width D = 12 288.  Reduce the rows first, PCA(n).fit_transform(X), and fit "
            f"covariance_type='diag' on the result.")
    if not isinstance(covariance_type, str) or covariance_type not in _TYPES:
        raise ValueError(f"The 'covariance_type' parameter of GaussianMixture must be a str among {_options(_TYPES)}. "
                         f"Got {covariance_type!r} instead.")


def _check_number(name, value, kind, low, closed_low=True):
    ok = not isinstance(value, bool) and isinstance(value, numbers.Integral if kind == "an int" else numbers.Real)
    if ok:
        ok = value >= low if closed_low else value > low
    if not ok:
        raise ValueError(f"The {name!r} parameter of GaussianMixture must be {kind} in the range {'[' if closed_low else '('}"
                         f"{low}, inf). Got {value!r} instead.")


def _check_shape(param, shape, name):
    got = tuple(param.shape)
    if got != tuple(shape):
        raise ValueError("The parameter '%s' should have the shape of %s, but got %s" % (name, tuple(shape), got))


def _check_x(X, who="GaussianMixture"):
    if not (isinstance(X, torch.Tensor) and X.is_cuda and X.dtype == torch.float32):
        raise ValueError(f"{who}: X must be a float32 [N, D] tensor on the GPU")
    if X.dim() != 2:
        raise ValueError(f"Expected 2D array, got {X.dim()}D tensor instead.")
    if X.shape[1] > 0 and X.stride(1) != 1:
        X = X.contiguous()
    return X


def _as_device(a, dtype, device):
    t = a if isinstance(a, torch.Tensor) else torch.tensor(np.asarray(a))
    return t.detach().to(device=device, dtype=dtype).contiguous()


class _Work:
    """Device buffers of one fit (shape-dependent, reused by every run)."""

    def __init__(self, N, D, K, spherical, device):
        f64 = lambda *s: torch.empty(*s, dtype=torch.float64, device=device)        # noqa: E731
        self.resp = torch.empty(N, K, dtype=torch.float32, device=device)
        self.lpn = f64(N)
        self.estat, self.record = f64(2), f64(ops.GMM_RECORD)
        self.part_e = f64(max(ops.gmm_parts(N, D, K, ops.GMM_ESTEP), 1))
        self.part_m = f64(max(ops.gmm_parts(N, D, K, ops.GMM_MSTEP), 1))
        self.means = [torch.empty(K, D, dtype=torch.float32, device=device) for _ in range(2)]
        self.cov = f64(K) if spherical else f64(K, D)
        self.prec = torch.empty(K, D, dtype=torch.float32, device=device)
        self.weights, self.logc = f64(K), f64(K)


class GaussianMixture:
    """sklearn.mixture.GaussianMixture for float32 [N, D] device tensors (a row stride is fine), covariance_type "diag"
    (THE DEFAULT HERE; sklearn's is "full") or "spherical"; "full" and "tied" raise NotImplementedError.  Names, defaults,
    stopping rules and error sentences are sklearn's.  fit / fit_predict / predict / predict_proba / score_samples / score /
    bic / aic; outputs are device tensors or Python floats.  Fitted: weights_ fp64 [K], means_ f32 [K, D], covariances_,
    precisions_, precisions_cholesky_ fp64 ([K, D]; spherical: [K]) on the device; converged_, n_iter_, lower_bound_,
    lower_bounds_, n_features_in_."""

    def __init__(self, n_components=1, *, covariance_type="diag", tol=1e-3, reg_covar=1e-6, max_iter=100, n_init=1,
                 init_params="kmeans", weights_init=None, means_init=None, precisions_init=None, random_state=None,
                 warm_start=False):
        _check_covariance_type(covariance_type)
        self.n_components, self.covariance_type, self.tol, self.reg_covar = n_components, covariance_type, tol, reg_covar
        self.max_iter, self.n_init, self.init_params = max_iter, n_init, init_params
        self.weights_init, self.means_init, self.precisions_init = weights_init, means_init, precisions_init
        self.random_state, self.warm_start = random_state, warm_start

    # ---- parameter checks (sklearn's _parameter_constraints and _check_parameters)
    def _check_params(self):
        _check_covariance_type(self.covariance_type)
        _check_number("n_components", self.n_components, "an int", 1)
        _check_number("tol", self.tol, "a float", 0.0)
        _check_number("reg_covar", self.reg_covar, "a float", 0.0)
        _check_number("max_iter", self.max_iter, "an int", 0)
        _check_number("n_init", self.n_init, "an int", 1)
        if not isinstance(self.init_params, str) or self.init_params not in _INITS:
            raise ValueError(f"The 'init_params' parameter of GaussianMixture must be a str among {_options(_INITS)}. "
                             f"Got {self.init_params!r} instead.")
        if self.n_components > ops.GMM_MAX_K:
            raise ValueError(f"GaussianMixture: n_components={self.n_components} > {ops.GMM_MAX_K}, the most the kernels take")

    def _check_inits(self, D, device):
        K, sph = int(self.n_components), self.covariance_type == "spherical"
        w = m = p = None
        if self.weights_init is not None:
            w = _as_device(self.weights_init, torch.float64, device)
            _check_shape(w, (K,), "weights")
            lo, hi, tot = float(w.min()), float(w.max()), float(w.sum())
            if lo < 0.0 or hi > 1.0:
                raise ValueError("The parameter 'weights' should be in the range [0, 1], but got max value %.5f, min value %.5f"
                                 % (lo, hi))
            if not abs(1.0 - tot) <= 1e-8:
                raise ValueError("The parameter 'weights' should be normalized, but got sum(weights) = %.5f" % tot)
        if self.means_init is not None:
            m = _as_device(self.means_init, torch.float32, device)
            _check_shape(m, (K, D), "means")
        if self.precisions_init is not None:
            p = _as_device(self.precisions_init, torch.float64, device)
            _check_shape(p, (K,) if sph else (K, D), "%s precision" % self.covariance_type)
            if bool((p <= 0.0).any()):
                raise ValueError("'%s precision' should be positive" % self.covariance_type)
        return w, m, p

    # ---- the steps
    def _e_step(self, X, w, means, labels=None, resp=True):
        ops.gmm_estep(X, means, w.prec, w.logc, w.resp if resp else None, w.lpn, labels, w.estat, w.part_e)

    def _m_step(self, X, w, means_old, means_new, n_norm, estat):
        ops.gmm_mstep(X, w.resp, means_old, w.part_m)
        ops.gmm_params(w.part_m, X.shape[0], means_old, self.reg_covar, self.covariance_type == "spherical", n_norm, estat,
                       means_new, w.cov, w.prec, w.weights, w.logc, w.record)

    @staticmethod
    def _refuse_rows(n):
        raise ValueError(f"GaussianMixture: {n} rows of X hold NaN or infinity")

    def _read(self, X, w, estep):
        """The iteration's one host read; raises what the record asks for."""
        rec = w.record.tolist()
        if estep and rec[ops.GMM_REFUSED] > 0:
            self._refuse_rows(int(rec[ops.GMM_REFUSED]))
        if rec[ops.GMM_BAD_COV] > 0:
            if not estep:                                    # an initial M-step: bad rows show as bad covariances first
                sq = torch.empty(X.shape[0], dtype=torch.float32, device=X.device)
                ops.row_sqnorm(X, sq)
                n = int((~torch.isfinite(sq)).sum())
                if n:
                    self._refuse_rows(n)
            raise ValueError(BAD_COVARIANCE)
        return rec

    def _initial_resp(self, X, w, rs):
        """BaseMixture._initialize_parameters: the initial responsibilities, on the device."""
        N, K = w.resp.shape
        dev = X.device
        if self.init_params == "random":
            resp = np.asarray(rs.uniform(size=(N, K)), dtype=np.float32)          # sklearn's own draw, in X's dtype
            resp /= resp.sum(axis=1)[:, np.newaxis]
            w.resp.copy_(torch.from_numpy(resp))
            return
        if self.init_params == "kmeans":
            label = KMeans(n_clusters=K, n_init=1, random_state=rs).fit(X).labels_
            rows = torch.arange(N, device=dev)
        else:
            if self.init_params == "random_from_data":
                indices = rs.choice(N, size=K, replace=False)
            else:
                _, indices = _kmeans_plusplus(X, K, rs)
            rows = torch.from_numpy(np.asarray(indices, dtype=np.int64)).to(dev)
            label = torch.arange(K, device=dev)
        w.resp.zero_()
        w.resp[rows, label] = 1.0

    def _initialize(self, X, w, inits, colmean):
        """GaussianMixture._initialize from w.resp: parameters into w (means in w.means[0]).  The first M-step has no old
        means: every component is shifted at the column means."""
        N, D = X.shape
        K = w.resp.shape[1]
        w_init, m_init, p_init = inits
        self._m_step(X, w, colmean.expand(K, D).contiguous(), w.means[0], N, None)
        self._read(X, w, False)
        if m_init is not None:
            w.means[0].copy_(m_init)
        if w_init is not None or p_init is not None:
            if w_init is not None:
                w.weights.copy_(w_init)
            if p_init is not None:
                w.cov.copy_(1.0 / p_init)
            ops.gmm_set_params(w.weights, w.cov, D, self.covariance_type == "spherical", w.prec, w.logc, w.record)

    def _get(self, w, means):
        return (w.weights.clone(), means.clone(), w.cov.clone(), w.prec.clone(), w.logc.clone())

    # ---- sklearn's interface
    def fit(self, X):
        self.fit_predict(X)
        return self

    def fit_predict(self, X):
        """BaseMixture.fit_predict, rule for rule -> int64 [N] labels on the device."""
        self._check_params()
        X = _check_x(X)
        N, D = X.shape
        K, sph = int(self.n_components), self.covariance_type == "spherical"
        if N < 2:
            raise ValueError(f"Found array with {N} sample(s) (shape=({N}, {D})) while a minimum of 2 is required.")
        if D < 1:
            raise ValueError(f"Found array with {D} feature(s) (shape=({N}, {D})) while a minimum of 1 is required.")
        if N < K:
            raise ValueError(f"Expected n_samples >= n_components but got n_components = {K}, n_samples = {N}")
        inits = self._check_inits(D, X.device)
        do_init = not (self.warm_start and hasattr(self, "converged_"))
        n_init = int(self.n_init) if do_init else 1
        w = _Work(N, D, K, sph, X.device)
        colmean = ops.pca_colstats(X)[0] if do_init else None
        if not do_init:
            if self.means_.shape != (K, D):
                raise ValueError(f"X has {D} features, but GaussianMixture is expecting {self.n_features_in_} features as input.")
            w.weights.copy_(self.weights_); w.means[0].copy_(self.means_); w.cov.copy_(self.covariances_)
            w.prec.copy_(self._prec); w.logc.copy_(self._logc)

        max_lower_bound, best_lower_bounds, best_params, best_n_iter = -np.inf, [], None, 0
        self.converged_ = False
        rs = _random_state(self.random_state)
        for _ in range(n_init):
            if do_init:
                self._initial_resp(X, w, rs)
                self._initialize(X, w, inits, colmean)
            cur, new = w.means
            lower_bound = -np.inf if do_init else self.lower_bound_
            current_lower_bounds = []
            if self.max_iter == 0:
                best_params, best_n_iter = self._get(w, cur), 0
            else:
                converged, n_iter = False, 0
                for n_iter in range(1, int(self.max_iter) + 1):
                    prev_lower_bound = lower_bound
                    self._e_step(X, w, cur)
                    self._m_step(X, w, cur, new, 0, w.estat)
                    cur, new = new, cur
                    lower_bound = self._read(X, w, True)[ops.GMM_LOWER_BOUND]
                    current_lower_bounds.append(lower_bound)
                    change = lower_bound - prev_lower_bound
                    if abs(change) < self.tol:
                        converged = True
                        break
                if lower_bound > max_lower_bound or max_lower_bound == -np.inf:
                    max_lower_bound = lower_bound
                    best_params, best_n_iter = self._get(w, cur), n_iter
                    best_lower_bounds = current_lower_bounds
                    self.converged_ = converged
        if not self.converged_ and self.max_iter > 0:
            warnings.warn(NOT_CONVERGED, ConvergenceWarning)
        self._set(best_params, D)
        self.n_iter_ = best_n_iter
        self.lower_bound_ = float(max_lower_bound)
        self.lower_bounds_ = best_lower_bounds
        # a final E-step: fit_predict(X) equals fit(X).predict(X) whatever max_iter and tol
        return self.predict(X)

    def _set(self, params, D):
        self.weights_, self.means_, self.covariances_, self._prec, self._logc = params
        self.precisions_ = 1.0 / self.covariances_
        self.precisions_cholesky_ = 1.0 / torch.sqrt(self.covariances_)
        self.n_features_in_ = D

    def _estimate(self, X, want_resp, want_labels):
        if not hasattr(self, "means_"):
            raise NotFittedError("This GaussianMixture instance is not fitted yet. Call 'fit' with appropriate arguments before "
                                 "using this estimator.")
        X = _check_x(X)
        N, D = X.shape
        if D != self.n_features_in_:
            raise ValueError(f"X has {D} features, but GaussianMixture is expecting {self.n_features_in_} features as input.")
        K, dev = self.means_.shape[0], X.device
        lpn = torch.empty(N, dtype=torch.float64, device=dev)
        resp = torch.empty(N, K, dtype=torch.float32, device=dev) if want_resp else None
        labels = torch.empty(N, dtype=torch.int64, device=dev) if want_labels else None
        estat = torch.zeros(2, dtype=torch.float64, device=dev)
        if N:
            ops.gmm_estep(X, self.means_, self._prec, self._logc, resp, lpn, labels, estat)
        total, refused = estat.tolist()
        if refused > 0:
            self._refuse_rows(int(refused))
        return lpn, resp, labels, total

    def predict(self, X):
        """The first component of largest weighted log density: int64 [N]."""
        return self._estimate(X, False, True)[2]

    def predict_proba(self, X):
        """The responsibilities, f32 [N, K]."""
        return self._estimate(X, True, False)[1]

    def score_samples(self, X):
        """log p(x_i) under the mixture: fp64 [N]."""
        return self._estimate(X, False, False)[0]

    def score(self, X, y=None):
        """The mean of score_samples (summed on the device in a fixed order)."""
        lpn, _, _, total = self._estimate(X, False, False)
        return total / lpn.shape[0]

    def _n_parameters(self):
        K, D = self.means_.shape
        cov_params = K * D if self.covariance_type == "diag" else K
        return int(cov_params + D * K + K - 1)

    def bic(self, X):
        return -2 * self.score(X) * X.shape[0] + self._n_parameters() * math.log(X.shape[0])

    def aic(self, X):
        return -2 * self.score(X) * X.shape[0] + 2 * self._n_parameters()


# ------------------------------------------------------------------------------------ the evaluation entry
@dataclass
class GMMReport:
    """Host values of one evaluate_gmm pass.  bic_curve: (n_components, bic) of every candidate fitted, in the given order."""
    purity: float
    nmi: float
    log_likelihood: float                # the mean per sample, on the fitted rows
    bic: float
    aic: float
    test_log_likelihood: float           # the mean per sample on test_loader's rows; None without one
    mean_confidence: float               # the mean over rows of the largest responsibility
    weights: np.ndarray                  # float64 [n_components]
    n_components: int
    n_iter: int
    converged: bool
    bic_curve: list
    n_samples: int
    fit_time: float
    inference_time: float


@torch.no_grad()
def evaluate_gmm(model, config, dataloader, n_components=None, covariance_type="diag", num_labels=None, max_rows=None, n_init=1,
                 random_state=0, test_loader=None):
    """A Gaussian mixture of the latents -> GMMReport: GaussianMixture(n_components, covariance_type, n_init, random_state) is
    fitted on the features of `dataloader` through the CURRENT, frozen encoder (evaluate_knn's features:
    get_latent_representation for vit_som, x_encoded for desom; any other model raises ValueError), at most max_rows rows (the
    first ones).  n_components: None = data.num_classes (the number of distinct labels when the config has none), an int as given, a sequence = every candidate is fitted, the one of
    lowest BIC is kept and all are recorded in bic_curve.  purity and nmi come from one contingency fold of the hard labels
    against the loader's (they must lie in [0, num_labels), default max(data.num_classes, 256)); test_log_likelihood is
    the mean log-likelihood of test_loader's rows under the fitted density.  The model's training mode is restored.
    model.world_size > 1 is refused with ValueError: every rank would have to gather all rows and fit the same mixture."""
    from . import evaluation as E                         # its loader pass and model adapter; evaluation imports this module
    arch = E._Arch(model, config, "evaluate_gmm").require("latent")
    if E._world(model) > 1:
        raise ValueError("evaluate_gmm: model.world_size > 1 is not supported; run it on one rank")
    dev = arch.device
    training = model.training
    try:
        X, y = E._rows(arch, dataloader, arch.latent, labels=True, what="loader")
        if max_rows is not None:
            X, y = X[:int(max_rows)], y[:int(max_rows)].contiguous()
        Q = E._rows(arch, test_loader, arch.latent, labels=True, what="test loader")[0] if test_loader is not None else None
    finally:
        model.train(training)
    if n_components is None:
        n_components = int(config["data"].get("num_classes", 0))
        if n_components < 1:                              # a clustering config: the distinct labels, as evaluate_kmeans counts them
            hist = E._Table(1, E._label_count(config, num_labels, True), dev)
            hist.add(torch.zeros_like(y), y)
            n_components = int((hist.numpy() > 0).sum())
    single = isinstance(n_components, numbers.Integral)
    candidates = [int(n_components)] if single else [int(k) for k in n_components]
    if not candidates:
        raise ValueError("evaluate_gmm: n_components is an empty sequence")
    torch.cuda.synchronize(dev)
    start = time.time()
    best, curve = None, []
    for k in candidates:
        gm = GaussianMixture(k, covariance_type=covariance_type, n_init=n_init, random_state=random_state).fit(X)
        bic = gm.bic(X)
        curve.append((k, bic))
        if best is None or bic < best[1]:
            best = (gm, bic)
    gm, bic = best
    fit_time = time.time() - start                        # bic's read of the score drains the device
    start = time.time()
    _, resp, pred, total = gm._estimate(X, True, True)
    table = E._Table(gm.n_components, E._label_count(config, num_labels, True), dev)
    table.add(pred, y)
    t = table.numpy()
    confidence = float(resp.max(dim=1).values.double().mean())
    test_ll = gm.score(Q) if Q is not None else None
    inference_time = time.time() - start
    report = GMMReport(purity=E.purity_from_table(t), nmi=E.nmi_from_table(t), log_likelihood=total / X.shape[0], bic=float(bic),
                       aic=float(gm.aic(X)), test_log_likelihood=test_ll, mean_confidence=confidence,
                       weights=gm.weights_.cpu().numpy(), n_components=int(gm.n_components), n_iter=int(gm.n_iter_),
                       converged=bool(gm.converged_), bic_curve=curve, n_samples=int(X.shape[0]), fit_time=float(fit_time),
                       inference_time=float(inference_time))
    print(f"Purity (GMM, {report.n_components} components): {report.purity:.3f}, NMI (GMM): {report.nmi:.3f}, BIC: {report.bic:.1f}, "
          f"Fit Time: {fit_time:.3f}, Inference Time: {inference_time:.3f}")
    return report
