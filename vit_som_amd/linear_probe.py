"""The linear probe: multinomial logistic regression fitted on the device (sklearn.linear_model.LogisticRegression's
interface; no counterpart in the reference).  The features never leave the device and are never copied: an iteration reads
X [N, D] exactly twice, through the PCA contractions (csrc/pca.hip), and everything else is row-local or vector work in
csrc/linear_probe.hip.  A fit is bitwise reproducible and depends on nothing but (X, y, parameters).

OBJECTIVE.  Parameters W [C, D] and b [C]; the model is always multinomial (softmax over C >= 2 rows):

    F(W, b) = (1 / N) sum_i CE(softmax(x~_i W^T + b), y_i) + (1 / (2 C_reg N)) |W|^2

The intercept is not penalised.  x~ = (x - mean) / std is the standardised row: the column statistics of vsom_pca_colstats,
the population std, scale 0 for a constant column (its x~ is 0).  For C >= 3 this is the objective of
Pipeline(StandardScaler(), sklearn.linear_model.LogisticRegression(C=C_reg)), and ``coef_`` is in standardised units like
the pipeline's.  For TWO classes the softmax parametrisation is kept (``coef_`` is [2, D]): sklearn fits a single row there,
whose penalty is that of w = w_1 - w_0 and not of both rows, so the two optima differ (the predictions rarely do).

FOLDING.  x~ is never materialised: logits = vsom_pca_project(X, mean, W o invstd), and dF/dW =
(vsom_pca_backproject(R, X, mean) o invstd) / N + W / (C_reg N) with R = softmax - onehot.

ALGORITHM.  L-BFGS with memory m = 10 and a backtracking (Armijo) line search, all decisions on the device.
1. The logits Z [N, C] of the current point stay on the device.  For a direction (P, p_b) one project gives
   Zp = (X - mean) (P o invstd)^T, and Z(a) = Z + a Zp: a trial step costs N C work and no pass over X.  The penalty along the
   direction is a quadratic in a from three dot products (vsom_probe_fold).
2. vsom_probe_linesearch evaluates the whole ladder a_j = a0 2^-j, j = 0 .. 15, in one launch; vsom_probe_step takes the
   largest step with F(a_j) <= F(0) + 1e-4 a_j g.p and applies it: Z += a Zp, theta += a p, s = a p.  F is strongly convex in
   W, so s.y > 0 holds at every accepted step without a curvature (Wolfe) condition; should rounding give s.y <= 0 the pair
   is skipped and counted (``n_skipped_pairs_``).
3. vsom_probe_residual forms R (rounded once to f32), the loss and the intercept gradient; one backproject and
   vsom_probe_gradient give g and y = g - g_prev.
4. The direction: vsom_lbfgs_dots (every new dot product in one pass over the 2 m + 3 vectors), vsom_lbfgs_coeff (the
   two-loop recursion on coefficients, one small workgroup), vsom_lbfgs_combine.  The host reads ONE 16-double record per
   iteration (step, line-search status, max |g|) to decide whether to stop.
5. Z accumulates one f32 rounding per step, so every REFRESH = 10 iterations it is recomputed by a true project.  When
   max |g| <= tol is met on an accumulated Z, the point is evaluated afresh before it is believed, and ``loss_`` and
   ``grad_norm_`` always come from a fresh project of the final weights.
6. A line search that finds no step (or a direction that is not a descent direction) empties the history and restarts from
   -g on a fresh Z; two in a row end the fit.
Stop: max |dF| <= tol, or max_iter.  Not reaching tol draws a ConvergenceWarning-style UserWarning, never an exception.
"""
import time
import warnings
from dataclasses import dataclass

import numpy as np
import torch

from . import ops
from .pca import NotFittedError

MAX_CLASSES = ops.PROBE_MAX_CLASSES
REFRESH = 10
LADDER = ops.PROBE_MAX_STEPS
ARMIJO_C1 = 1e-4


class ConvergenceWarning(UserWarning):
    """The solver stopped before max |gradient| <= tol (sklearn.exceptions.ConvergenceWarning is a UserWarning too)."""


def _check_params(C, tol, max_iter, memory):
    if isinstance(C, bool) or not isinstance(C, (int, float, np.integer, np.floating)) or not C > 0:
        raise ValueError(f"The 'C' parameter of LogisticRegression must be a float in the range (0.0, inf]. Got {C!r} instead.")
    if isinstance(tol, bool) or not isinstance(tol, (int, float, np.integer, np.floating)) or not tol >= 0:
        raise ValueError(f"The 'tol' parameter of LogisticRegression must be a float in the range [0.0, inf). Got {tol!r} instead.")
    if isinstance(max_iter, bool) or not isinstance(max_iter, (int, np.integer)) or max_iter < 0:
        raise ValueError(f"The 'max_iter' parameter of LogisticRegression must be an int in the range [0, inf). Got {max_iter!r} "
                         f"instead.")
    if isinstance(memory, bool) or not isinstance(memory, (int, np.integer)) or not 1 <= memory <= ops.LBFGS_MAX_MEMORY:
        raise ValueError(f"The 'memory' parameter of LogisticRegression must be an int in the range [1, {ops.LBFGS_MAX_MEMORY}]. "
                         f"Got {memory!r} instead.")


class LogisticRegression:
    """Multinomial logistic regression on float32 device rows and int64 device labels: fit / decision_function / predict /
    predict_proba / score.  Fitted: coef_ f64 [C, D] (standardised units), intercept_ f64 [C], mean_ f32 [D], scale_ f64 [D]
    (device tensors), classes_, n_iter_, converged_, loss_, grad_norm_, n_skipped_pairs_, n_restarts_, n_features_in_."""

    def __init__(self, C=1.0, tol=1e-4, max_iter=100, fit_intercept=True, standardize=True, n_classes=None, memory=10):
        self.C, self.tol, self.max_iter = C, tol, max_iter
        self.fit_intercept, self.standardize = bool(fit_intercept), bool(standardize)
        self.n_classes, self.memory = n_classes, memory

    # ---- helpers
    @staticmethod
    def _rows(X):
        if not isinstance(X, torch.Tensor) or X.dim() != 2:
            got = f"{X.dim()}D tensor" if isinstance(X, torch.Tensor) else type(X).__name__
            raise ValueError(f"Expected 2D array, got {got} instead.")
        ops._f32(X, "X")
        return X

    def _fitted(self):
        if not hasattr(self, "coef_"):
            raise NotFittedError("This LogisticRegression instance is not fitted yet. Call 'fit' with appropriate arguments before "
                                 "using this estimator.")

    @staticmethod
    def _padded(N, C, dev):
        """[N, C] f32 in rows of a multiple of four floats: the backproject then takes 16-byte loads of it."""
        return torch.zeros(N, (C + 3) // 4 * 4, dtype=torch.float32, device=dev)[:, :C]

    # ---- sklearn's interface
    def fit(self, X, y):
        _check_params(self.C, self.tol, self.max_iter, self.memory)
        X = self._rows(X)
        if not isinstance(y, torch.Tensor) or y.dim() != 1:
            raise ValueError("y should be a 1d tensor of class indices")
        N, D = X.shape
        if y.shape[0] != N:
            raise ValueError(f"Found input variables with inconsistent numbers of samples: [{N}, {y.shape[0]}]")
        if y.dtype != torch.int64 or y.device != X.device:
            raise ValueError("y: expected int64 labels on the device of X")
        if N < 2:
            raise ValueError(f"Found array with {N} sample(s) (shape=({N}, {D})) while a minimum of 2 is required.")
        y = y.contiguous()
        C = self.n_classes
        if C is None:
            C = int(y.max()) + 1
        if isinstance(C, bool) or not isinstance(C, (int, np.integer)) or C < 1:
            raise ValueError(f"n_classes must be a positive int or None, got {C!r}")
        C = int(C)
        if C < 2:
            raise ValueError("This solver needs samples of at least 2 classes in the data, but the data contains only one class: 0")
        if C > MAX_CLASSES or C > D:
            raise ValueError(f"LogisticRegression: n_classes={C} > min({MAX_CLASSES}, n_features={D}), the widest problem the kernels "
                             f"take")
        dev, m = X.device, int(self.memory)
        f64 = lambda *s: torch.zeros(*s, dtype=torch.float64, device=dev)       # noqa: E731

        # ---- statistics, folded into the weights
        if self.standardize:
            mean, var = ops.pca_colstats(X)
            std = torch.sqrt(var * ((N - 1) / N))
            const = std == 0
            invstd = torch.where(const, torch.zeros_like(std), 1.0 / torch.where(const, torch.ones_like(std), std)).contiguous()
            scale = torch.where(const, torch.ones_like(std), std)
        else:
            mean, invstd, scale = None, f64(D) + 1.0, f64(D) + 1.0
        lam = 1.0 / (float(self.C) * N)

        # ---- state
        nw = C * D
        n = nw + (C if self.fit_intercept else 0)
        theta, p, s_new, y_new = f64(n), f64(n), f64(n), f64(n)
        g_cur, g_nxt = f64(n), f64(n)
        W, P = theta[:nw].view(C, D), p[:nw].view(C, D)
        b, pb = (theta[nw:], p[nw:]) if self.fit_intercept else (None, None)
        S, Y = f64(m, n), f64(m, n)
        state = ops.lbfgs_state(m, dev)
        dots, phi, pen, loss, gb = f64(3 * (2 * m + 3) + 1), f64(LADDER), f64(3), f64(1), f64(C)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        Z, Zp, R = self._padded(N, C, dev), self._padded(N, C, dev), self._padded(N, C, dev)
        Bf = torch.empty(C, D, dtype=torch.float32, device=dev)
        Zt = torch.empty(C, D, dtype=torch.float32, device=dev)

        def gradient(fresh, g_prev, g, y_out):
            if fresh:
                ops.probe_fold(W, invstd, Bf)
                ops.pca_project(X, mean, Bf, None, Z)
            ops.probe_residual(Z, b, y, R, loss, gb, status)
            ops.pca_backproject(R, X, mean, Zt)
            ops.probe_gradient(Zt, invstd, theta, gb, N, lam, g, g_prev, y_out)

        def restart(g):
            ops.lbfgs_dots(S, Y, g, None, None, state, dots)
            ops.lbfgs_coeff(dots, m, False, state)

        gradient(True, None, g_cur, None)
        n_bad = int(status.item())
        if n_bad:
            raise ValueError(f"y contains {n_bad} labels outside [0, {C}): labels must be class indices below n_classes")
        restart(g_cur)
        rec = state[:ops.LBFGS_RECORD].cpu().numpy()
        tol = float(self.tol)
        converged, fresh = bool(rec[ops.LBFGS_GMAX] <= tol), True
        n_iter = failures = restarts = 0
        failed_last = False
        while not converged and n_iter < int(self.max_iter):
            n_iter += 1
            ops.lbfgs_combine(S, Y, g_cur, s_new, y_new, state, p)
            ops.probe_fold(P, invstd, Bf, W, pen)
            ops.pca_project(X, mean, Bf, None, Zp)
            ops.probe_linesearch(Z, Zp, b, pb, y, state[ops.LBFGS_ALPHA0:ops.LBFGS_ALPHA0 + 1], LADDER, phi)
            ops.probe_step(phi, state[ops.LBFGS_ALPHA0:ops.LBFGS_ALPHA0 + 1], loss, pen, state[ops.LBFGS_GTP:ops.LBFGS_GTP + 1], lam,
                           ARMIJO_C1, Z, Zp, theta, p, s_new, state)
            fresh = n_iter % REFRESH == 0
            gradient(fresh, g_cur, g_nxt, y_new)
            ops.lbfgs_dots(S, Y, g_nxt, s_new, y_new, state, dots)
            ops.lbfgs_coeff(dots, m, True, state)
            rec = state[:ops.LBFGS_RECORD].cpu().numpy()                 # the iteration's one host read
            g_cur, g_nxt = g_nxt, g_cur
            if rec[ops.PROBE_LS_STATUS] != 0:                            # nothing moved: restart from -g on a fresh Z
                failures += 1
                if failed_last:
                    break
                failed_last, fresh = True, True
                restarts += 1
                gradient(True, None, g_cur, None)
                restart(g_cur)
                continue
            failed_last = False
            if rec[ops.LBFGS_GMAX] <= tol:
                if not fresh:                                            # believed only on a true project
                    gradient(True, None, g_nxt, None)
                    fresh = True
                    converged = float(g_nxt.abs().max()) <= tol
                    # otherwise the fit goes on: Z is fresh now, the direction keeps the gradient its coefficients belong to
                else:
                    converged = True

        # ---- the reported loss and gradient: a fresh project of the final weights
        gradient(True, None, g_nxt, None)
        grad_norm = float(g_nxt.abs().max())
        self.loss_ = float(loss.item()) / N + 0.5 * lam * float((W * W).sum())
        self.grad_norm_ = grad_norm
        self.converged_ = bool(grad_norm <= tol)
        self.n_iter_ = n_iter
        self.n_skipped_pairs_ = int(state[ops.LBFGS_SKIPPED].item()) - failures
        self.n_restarts_ = restarts
        self.coef_ = W.clone()
        self.intercept_ = b.clone() if b is not None else f64(C)
        self.mean_ = mean if mean is not None else torch.zeros(D, dtype=torch.float32, device=dev)
        self.scale_ = scale
        self._mean, self._invstd = mean, invstd
        self.classes_ = torch.arange(C, device=dev)
        self.n_features_in_, self.n_classes_ = D, C
        if not self.converged_:
            warnings.warn(f"LogisticRegression: max |gradient| is {grad_norm:.2e} > tol = {tol:.1e} after {n_iter} iterations. "
                          f"Increase the number of iterations (max_iter) or loosen tol.", ConvergenceWarning)
        return self

    def _forward(self, X, want_prob):
        self._fitted()
        X = self._rows(X)
        if X.shape[1] != self.n_features_in_:
            raise ValueError(f"X has {X.shape[1]} features, but LogisticRegression is expecting {self.n_features_in_} features as "
                             f"input.")
        N, C, dev = X.shape[0], self.n_classes_, X.device
        rows = torch.cat([X, X]) if N == 1 else X            # the kernels take two rows at least
        M = rows.shape[0]
        Z = self._padded(M, C, dev)
        pred = torch.empty(M, dtype=torch.int64, device=dev)
        prob = torch.empty(M, C, dtype=torch.float64, device=dev) if want_prob else None
        if M == 0:
            return Z, pred, prob
        Bf = torch.empty(C, self.n_features_in_, dtype=torch.float32, device=dev)
        ops.probe_fold(self.coef_, self._invstd, Bf)
        ops.pca_project(rows, self._mean, Bf, None, Z)
        f64 = lambda *s: torch.zeros(*s, dtype=torch.float64, device=dev)       # noqa: E731
        ops.probe_residual(Z, self.intercept_, torch.zeros(M, dtype=torch.int64, device=dev), self._padded(M, C, dev), f64(1), f64(C),
                           torch.zeros(1, dtype=torch.int32, device=dev), pred, prob)
        return Z[:N], pred[:N], (prob[:N] if want_prob else None)

    def decision_function(self, X):
        """(x~ coef_^T + intercept_): f64 [N, C]; the contraction runs in f32."""
        Z, _, _ = self._forward(X, False)
        return Z.double() + self.intercept_

    def predict(self, X):
        """The first class of largest decision value: int64 [N]."""
        return self._forward(X, False)[1]

    def predict_proba(self, X):
        """softmax of the decision values in fp64: [N, C]."""
        return self._forward(X, True)[2]

    def score(self, X, y):
        """Mean accuracy."""
        pred = self.predict(X)
        if not isinstance(y, torch.Tensor) or y.shape != pred.shape:
            raise ValueError(f"Found input variables with inconsistent numbers of samples: [{pred.shape[0]}, "
                             f"{y.shape[0] if hasattr(y, 'shape') and len(y.shape) else 1}]")
        return float((pred == y.to(pred.device)).double().mean()) if pred.numel() else 0.0


# ------------------------------------------------------------------------------------ the evaluation entry
@dataclass
class LinearProbeReport:
    """Host values of one evaluate_linear_probe pass.  confusion[t, p] counts the test samples of class t predicted as p."""
    accuracy: float
    per_class_accuracy: np.ndarray       # float64 [C]: NaN for a class without a test sample
    confusion: np.ndarray                # int64 [C, C]
    train_accuracy: float
    n_train: int
    n_test: int
    n_iter: int
    converged: bool
    loss: float                          # the objective at the fitted weights (linear_probe.py)
    fit_time: float
    inference_time: float


def linear_probe_report(cm, train_accuracy, n_train, n_iter, converged, loss, fit_time, inference_time):
    """The report's arithmetic from the confusion table cm[true, pred] of the test set."""
    cm = np.asarray(cm)
    true_sum = cm.sum(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        per_class = np.where(true_sum > 0, np.diag(cm) / true_sum, np.nan)
    n_test = int(cm.sum())
    return LinearProbeReport(accuracy=float(np.diag(cm).sum() / n_test) if n_test else float("nan"), per_class_accuracy=per_class,
                             confusion=cm.astype(np.int64), train_accuracy=float(train_accuracy), n_train=int(n_train), n_test=n_test,
                             n_iter=int(n_iter), converged=bool(converged), loss=float(loss), fit_time=float(fit_time),
                             inference_time=float(inference_time))


@torch.no_grad()
def evaluate_linear_probe(model, config, train_loader, test_loader, C=1.0, tol=1e-4, max_iter=100, num_labels=None, max_rows=None):
    """Linear probe of the latents -> LinearProbeReport: a multinomial logistic regression (linear_probe.LogisticRegression:
    standardised features, L2 penalty 1 / C) is fitted on the features of train_loader through the CURRENT, frozen encoder
    and scored on test_loader.  Features are evaluate_knn's: model.get_latent_representation(x) for vit_som, x_encoded for
    desom; any other model raises ValueError.  At most max_rows training rows (the first ones) are used.  Labels must lie in
    [0, num_labels) (default data.num_classes, or the largest training label + 1 when the config has none; at most
    min(256, feature width)).  The confusion matrix is one `vsom_contingency` launch; the model's training mode is restored.
    model.world_size > 1 is refused with ValueError: every rank would have to gather all rows and fit the same model, and
    that path has not been exercised."""
    from . import evaluation as E                         # its loader pass and model adapter; imported here, evaluation imports this module
    arch = E._Arch(model, config, "evaluate_linear_probe").require("latent")
    if E._world(model) > 1:
        raise ValueError("evaluate_linear_probe: model.world_size > 1 is not supported; run it on one rank")
    dev = arch.device
    training = model.training
    try:
        X, y = E._rows(arch, train_loader, arch.latent, labels=True, what="train loader")
        if max_rows is not None:
            X, y = X[:int(max_rows)], y[:int(max_rows)].contiguous()
        Q, yq = E._rows(arch, test_loader, arch.latent, labels=True, what="test loader")
    finally:
        model.train(training)
    L = int(num_labels or config["data"].get("num_classes", 0) or max(int(y.max()) + 1, 2))
    clf = LogisticRegression(C=C, tol=tol, max_iter=max_iter, n_classes=L)
    torch.cuda.synchronize(dev)
    start = time.time()
    clf.fit(X, y)                                         # its last step reads the final gradient: the device is drained
    fit_time = time.time() - start
    start = time.time()
    train_accuracy = clf.score(X, y)
    pred = clf.predict(Q)
    table = E._Table(L, L, dev)
    table.add(yq, pred)                                   # cm[true, pred]; a label outside [0, L) is counted and raises below
    cm = table.numpy()
    inference_time = time.time() - start
    report = linear_probe_report(cm, train_accuracy, X.shape[0], clf.n_iter_, clf.converged_, clf.loss_, fit_time, inference_time)
    print(f"Linear probe accuracy (C={C}): {report.accuracy:.3f} (train {report.train_accuracy:.3f}, {report.n_iter} iterations), "
          f"Fit Time: {fit_time:.3f}, Inference Time: {inference_time:.3f}")
    return report
