"""The linear probe without a GPU: the references of linear_probe_ref.py against sklearn and against each other, the
class's argument checks and their wording, the report's arithmetic, the driver's switch, and the C-ABI of the new entries
(declared, bound, wrapped, and refusing bad calls on the host before any launch)."""
import os
import re

import numpy as np
import pytest
import torch

import linear_probe_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 4096                    # stands for a non-null, 16-byte aligned device pointer: nothing is launched, nothing dereferenced
ENTRIES = ["vsom_probe_fold_parts", "vsom_probe_fold", "vsom_probe_parts", "vsom_probe_residual", "vsom_probe_linesearch",
           "vsom_probe_step", "vsom_probe_gradient", "vsom_lbfgs_state_doubles", "vsom_lbfgs_parts", "vsom_lbfgs_dots",
           "vsom_lbfgs_coeff", "vsom_lbfgs_combine"]
WRAPPERS = ["probe_parts", "probe_fold", "probe_residual", "probe_linesearch", "probe_step", "probe_gradient", "lbfgs_state",
            "lbfgs_dots", "lbfgs_coeff", "lbfgs_combine"]


# ------------------------------------------------------------------ the references
@pytest.mark.parametrize("name,C_reg", [("odd", 1.0), ("odd", 100.0), ("shifted", 1.0), ("wide", 1.0), ("elementwise", 1.0)])
def test_reference_optimum_is_the_sklearn_pipelines(name, C_reg):
    X, y, _, _ = R.fixture(name)
    C = R.FIXTURES[name][2]
    assert C >= 3
    W, b, F = R.optimum(name, C_reg)
    lr = R.sklearn_pipeline(name, C_reg)[-1]
    print(f"{name} C={C_reg}: |coef - sklearn| {np.abs(W - lr.coef_).max():.2e}")
    assert np.abs(W - lr.coef_).max() <= 1e-4
    assert np.abs((b - b.mean()) - (lr.intercept_ - lr.intercept_.mean())).max() <= 1e-4
    mean, scale = R.standardise(X)
    assert R.objective_at(W, b, X, y, mean, scale, C_reg)[1] <= 1e-8             # a stationary point in fp64


@pytest.mark.parametrize("name", sorted(R.FIXTURES))
def test_fixtures_leave_the_prediction_test_its_rows(name):
    """The cap of the prediction test on the reference alone: at most 2 % of the rows (training and held out) may have an
    fp64 top-two margin of 1e-3 or less at the optimum.  Every class occurs, the shapes are the ones the issue names."""
    X, y, Xh, yh = R.fixture(name)
    N, D, C = R.FIXTURES[name][:3]
    assert X.shape == (N, D) and Xh.shape == (R.HELD_OUT, D) and set(y.tolist()) == set(range(C))
    mean, scale = R.standardise(X)
    for C_reg in (1.0, 100.0):
        W, b, _ = R.optimum(name, C_reg)
        for rows in (X, Xh):
            m = R.margins(W, b, (rows.astype(np.float64) - mean) / scale)
            assert (m <= 1e-3).mean() <= 0.02
    assert {"odd": (257, 131, 5), "shifted": (300, 64, 3), "wide": (515, 260, 17)}.items() <= {k: v[:3] for k, v in R.FIXTURES.items()}.items()
    _, D_e, _, _, _, pad_e = R.FIXTURES["elementwise"]
    assert D_e % 4 != 0 and pad_e > 0 and (D_e + pad_e) % 4 != 0
    assert abs(float(R.fixture("shifted")[0].mean()) - 50.0) < 1.0


def test_gradient_of_the_reference_objective_by_differences():
    X, y, _, _ = R.fixture("elementwise")
    C = R.FIXTURES["elementwise"][2]
    mean, scale = R.standardise(X)
    Xs = (X.astype(np.float64) - mean) / scale
    rng = np.random.RandomState(0)
    theta = 0.1 * rng.standard_normal(C * Xs.shape[1] + C)
    _, g = R.objective(theta, Xs, y, C, 0.7)
    for i in rng.choice(theta.size, 12, replace=False):
        e = np.zeros_like(theta)
        e[i] = 1e-6
        num = (R.objective(theta + e, Xs, y, C, 0.7)[0] - R.objective(theta - e, Xs, y, C, 0.7)[0]) / 2e-6
        assert abs(num - g[i]) <= 1e-8 + 1e-6 * abs(g[i])


def test_emulation_reaches_the_optimum_and_two_loop_is_exact_on_one_pair():
    X, y, _, _ = R.fixture("elementwise")
    C = R.FIXTURES["elementwise"][2]
    W, b, mean, scale, n_iter, converged = R.emulate(X, y, C, 1.0, 1e-5, 500)
    F, gmax = R.objective_at(W, b, X, y, mean, scale, 1.0)
    assert converged and n_iter < 100 and gmax <= 2e-5
    assert 0 <= F - R.optimum("elementwise", 1.0)[2] <= 1e-6
    # one pair, integers: -H g = -(gamma g - ...) by hand
    s, yv, g = np.array([1.0, 0.0, 2.0]), np.array([2.0, 0.0, 0.0]), np.array([4.0, 8.0, -2.0])
    rho, gamma = 1 / (s @ yv), (s @ yv) / (yv @ yv)
    a = rho * (s @ -g)
    q = (-g - a * yv) * gamma
    want = q + (a - rho * (yv @ q)) * s
    assert np.array_equal(R.two_loop([(s, yv)], g), want)
    assert np.array_equal(R.two_loop([], g), -g)


def test_armijo_reference_picks_the_largest_passing_step():
    phi = np.array([50.0, 20.0, 9.0, 9.9])
    assert R.armijo(phi, 1.0, 10.0, (0.0, 0.0, 0.0), -1.0, 1, 0.0)[:2] == (0.25, 0)
    assert R.armijo(phi, 1.0, 5.0, (0.0, 0.0, 0.0), -1.0, 1, 0.0)[:2] == (0.0, 1)
    assert R.armijo(phi, 1.0, 10.0, (0.0, 0.0, 0.0), 0.0, 1, 0.0)[:2] == (0.0, 2)
    # the penalty's quadratic decides: W.P < 0 pays for a rise of the data term
    assert R.armijo(np.array([10.5]), 1.0, 10.0, (4.0, -2.0, 1.0), -1.0, 1, 1.0)[:2] == (1.0, 0)


# ------------------------------------------------------------------ the class
def test_parameter_checks_and_their_wording():
    from vit_som_amd import LogisticRegression
    from vit_som_amd.linear_probe import ConvergenceWarning
    assert issubclass(ConvergenceWarning, UserWarning)
    X, y = torch.zeros(4, 3), torch.zeros(4, dtype=torch.int64)
    with pytest.raises(ValueError, match=r"The 'C' parameter of LogisticRegression must be a float in the range \(0\.0, inf\]\. Got -1\.0 instead\."):
        LogisticRegression(C=-1.0).fit(X, y)
    with pytest.raises(ValueError, match=r"The 'C' parameter .* Got 0 instead"):
        LogisticRegression(C=0).fit(X, y)
    with pytest.raises(ValueError, match=r"The 'tol' parameter of LogisticRegression must be a float in the range \[0\.0, inf\)\. Got -0\.5 instead\."):
        LogisticRegression(tol=-0.5).fit(X, y)
    with pytest.raises(ValueError, match=r"The 'max_iter' parameter of LogisticRegression must be an int in the range \[0, inf\)\. Got -3 instead\."):
        LogisticRegression(max_iter=-3).fit(X, y)
    with pytest.raises(ValueError, match=r"The 'max_iter' parameter .* Got 2\.5 instead"):
        LogisticRegression(max_iter=2.5).fit(X, y)
    with pytest.raises(ValueError, match=r"The 'memory' parameter of LogisticRegression must be an int in the range \[1, 16\]\. Got 17 instead\."):
        LogisticRegression(memory=17).fit(X, y)
    with pytest.raises(ValueError, match="Expected 2D array, got 1D tensor instead"):
        LogisticRegression().fit(torch.zeros(4), y)
    with pytest.raises(ValueError, match="Expected 2D array, got list instead"):
        LogisticRegression().fit([[0.0]], y)
    with pytest.raises(ValueError, match="expected a HIP device tensor"):
        LogisticRegression().fit(X, y)                                   # there is no CPU path
    d = LogisticRegression()
    assert (d.C, d.tol, d.max_iter, d.fit_intercept, d.standardize, d.n_classes, d.memory) == (1.0, 1e-4, 100, True, True, None, 10)


def test_not_fitted_wording():
    from vit_som_amd import LogisticRegression
    from vit_som_amd.pca import NotFittedError
    for method in ("predict", "predict_proba", "decision_function"):
        with pytest.raises(NotFittedError, match="This LogisticRegression instance is not fitted yet. Call 'fit' with appropriate "
                                                 "arguments before using this estimator."):
            getattr(LogisticRegression(), method)(torch.zeros(2, 3))
    with pytest.raises(NotFittedError):
        LogisticRegression().score(torch.zeros(2, 3), torch.zeros(2, dtype=torch.int64))


def test_docstring_states_the_objective_and_the_two_class_difference():
    import vit_som_amd.linear_probe as LP
    doc = LP.__doc__
    for words in ("OBJECTIVE", "The intercept is not penalised", "TWO classes", "sklearn fits a single row", "Armijo", "REFRESH = 10"):
        assert words in doc, words
    assert LP.REFRESH == 10 and LP.LADDER == 16 and LP.ARMIJO_C1 == 1e-4


# ------------------------------------------------------------------ the report and the driver
def test_report_arithmetic_from_a_confusion_table():
    from vit_som_amd.evaluation import LinearProbeReport, linear_probe_report
    cm = np.array([[5, 1, 0, 0], [2, 2, 0, 0], [0, 0, 0, 0], [0, 3, 0, 7]])
    r = linear_probe_report(cm, 0.9, 123, 17, True, 0.25, 1.5, 0.5)
    assert isinstance(r, LinearProbeReport)
    assert r.accuracy == 14 / 20 and r.n_test == 20 and r.n_train == 123 and r.n_iter == 17 and r.converged is True
    assert np.allclose(r.per_class_accuracy[[0, 1, 3]], [5 / 6, 0.5, 0.7]) and np.isnan(r.per_class_accuracy[2])
    assert r.confusion.dtype == np.int64 and np.array_equal(r.confusion, cm) and int(r.confusion.sum()) == r.n_test
    assert (r.train_accuracy, r.loss, r.fit_time, r.inference_time) == (0.9, 0.25, 1.5, 0.5)
    empty = linear_probe_report(np.zeros((3, 3), np.int64), 1.0, 2, 0, False, 0.0, 0.0, 0.0)
    assert np.isnan(empty.accuracy) and empty.n_test == 0 and np.isnan(empty.per_class_accuracy).all()


def test_evaluate_linear_probe_refuses_other_models_and_several_ranks():
    import inspect
    from vit_som_amd import evaluate_linear_probe
    sig = inspect.signature(evaluate_linear_probe)
    assert list(sig.parameters) == ["model", "config", "train_loader", "test_loader", "C", "tol", "max_iter", "num_labels", "max_rows"]
    assert [sig.parameters[k].default for k in ("C", "tol", "max_iter", "num_labels", "max_rows")] == [1.0, 1e-4, 100, None, None]
    cfg = {"data": {"num_channels": 1, "input_size": 8, "num_classes": 3}, "hyperparameters": {"model_arch": "vit"}}
    with pytest.raises(ValueError, match="evaluate_linear_probe: needs a vit_som or a desom model"):
        evaluate_linear_probe(object(), cfg, [], [])

    class Two:
        world_size = 2

        def get_latent_representation(self, x):
            return x
    cfg["hyperparameters"]["model_arch"] = "vit_som"
    with pytest.raises(ValueError, match="world_size > 1 is not supported"):
        evaluate_linear_probe(Two(), cfg, [], [])


def test_driver_switch():
    import inspect
    from vit_som_amd import train
    a = train._parser().parse_args(["--config", "c.yaml", "--linear-probe"])
    assert a.linear_probe is True and a.knn_eval is False
    assert train._parser().parse_args(["--config", "c.yaml"]).linear_probe is False
    assert inspect.signature(train.main).parameters["linear_probe"].default is False


# ------------------------------------------------------------------ the C-ABI
def test_every_new_entry_is_declared_bound_and_wrapped():
    from vit_som_amd import ops
    from vit_som_amd._lib import SIGNATURES, lib
    src = open(os.path.join(ROOT, "include", "vitsom_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(vsom_[a-z0-9_]+)\s*\(", src))
    for name in ENTRIES:
        assert name in declared and name in SIGNATURES and hasattr(lib, name), name
    assert {n for n in declared if n.startswith(("vsom_probe_", "vsom_lbfgs_"))} == set(ENTRIES)
    for name in WRAPPERS:
        assert callable(getattr(ops, name)), name
    text = open(os.path.join(ROOT, "vit_som_amd", "ops.py")).read()
    for name in ENTRIES:
        assert f"lib.{name}(" in text, f"{name} has no wrapper in ops.py"
    assert "linear_probe" in open(os.path.join(ROOT, "vit_som_amd", "csrc", "build.sh")).read()


def test_size_queries_are_host_arithmetic():
    from vit_som_amd._lib import lib as L
    assert L.vsom_probe_parts(257, 5) >= 16 and L.vsom_probe_parts(257, 5) % 16 == 0          # max(C + 1, 16) per workgroup
    assert L.vsom_probe_parts(50000, 100) % 101 == 0 and L.vsom_probe_parts(50000, 100) <= 1024 * 101
    assert L.vsom_probe_parts(2 ** 31 - 300, 256) <= 1024 * 257
    assert L.vsom_probe_parts(0, 5) == 0 and L.vsom_probe_parts(10, 1) == 0 and L.vsom_probe_parts(10, 257) == 0
    assert L.vsom_probe_fold_parts(5, 131) == 3 and L.vsom_probe_fold_parts(100, 12288) == 3 * 400
    assert L.vsom_probe_fold_parts(0, 4) == 0
    assert L.vsom_lbfgs_state_doubles(10) == 16 + 21 * 21 + 21 and L.vsom_lbfgs_state_doubles(0) == 0
    assert L.vsom_lbfgs_state_doubles(17) == 0
    assert L.vsom_lbfgs_parts(660, 10) == 70 and L.vsom_lbfgs_parts(1228900, 10) == 70 * 401
    assert L.vsom_lbfgs_parts(0, 10) == 0 and L.vsom_lbfgs_parts(5, 17) == 0


def test_bad_calls_are_refused_before_any_launch():
    """Limits give VSOM_EUNSUPPORTED (-3), a scratch array that is NULL or one element short VSOM_EWORKSPACE (-4), with the
    buffer named; the calls that precede pass every other check, so -4 is what the workspace check itself returns."""
    from vit_som_amd._lib import last_error, lib as L
    N, C, D, m = 257, 5, 131, 10
    n = C * D + C
    residual = lambda N_, C_, part, n_part: L.vsom_probe_residual(P, 8, N_, C_, P, P, P, 8, P, P, None, None, P, part, n_part, None)  # noqa: E731
    ladder = lambda N_, C_, part, n_part, k=16: L.vsom_probe_linesearch(P, P, 8, N_, C_, P, P, P, P, k, P, part, n_part, None)       # noqa: E731
    fold = lambda C_, D_, part, n_part: L.vsom_probe_fold(P, P, C_, D_, P, D_, P, P, part, n_part, None)                           # noqa: E731
    dots = lambda m_, part, n_part: L.vsom_lbfgs_dots(P, P, P, P, P, n, m_, 1, P, P, part, n_part, None)                           # noqa: E731
    need = L.vsom_probe_parts(N, C)
    for call, need_here in ((lambda p, k: residual(N, C, p, k), need // 16 * (C + 1)), (lambda p, k: ladder(N, C, p, k), need),
                            (lambda p, k: fold(C, D, p, k), L.vsom_probe_fold_parts(C, D)),
                            (lambda p, k: dots(m, p, k), L.vsom_lbfgs_parts(n, m))):
        assert need_here > 0
        assert call(P, need_here - 1) == -4, last_error()
        assert "partial buffer" in last_error() and "<" in last_error()
        assert call(None, 1 << 40) == -4 and call(P, 0) == -4
    for bad in ((N, 1), (N, 257), (1, C)):
        assert residual(*bad, P, 1 << 40) == -3, last_error()
        assert ladder(*bad, P, 1 << 40) == -3, last_error()
    assert L.vsom_probe_step(P, 16, P, P, P, P, 1e-3, 1e-4, P, P, 8, 1, C, P, P, P, n, P, None) == -3
    assert ladder(N, C, P, 1 << 40, 17) == -3 and "steps" in last_error()
    assert fold(9, 8, P, 1 << 40) == -3 and "D=8" in last_error()                   # C > D
    assert fold(257, 300, P, 1 << 40) == -3 and fold(1, 300, P, 1 << 40) == -3
    assert L.vsom_probe_gradient(P, 8, P, P, P, 9, 8, 1, N, 1e-3, None, P, None, None) == -3
    assert L.vsom_probe_gradient(P, D, P, P, None, C, D, 1, N, 1e-3, None, P, None, None) == -1 and "gb" in last_error()
    assert dots(17, P, 1 << 40) == -3 and L.vsom_lbfgs_coeff(P, 0, 1, P, None) == -3
    assert L.vsom_lbfgs_combine(P, P, P, P, P, n, 17, P, P, None) == -3
    assert residual(N, C, None, 0) == -4 and L.vsom_probe_residual(None, 8, N, C, P, P, P, 8, P, P, None, None, P, P, 1 << 40, None) == -1
    assert L.vsom_probe_residual(P, 4, N, C, P, P, P, 8, P, P, None, None, P, P, 1 << 40, None) == -1 and "row stride" in last_error()
