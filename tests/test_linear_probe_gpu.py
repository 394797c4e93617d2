"""The linear probe on the MI355X: the kernels of csrc/linear_probe.hip against fp64 numpy on the same f32 logits, the line
search's identity, the L-BFGS pieces against the textbook two-loop recursion, the solver (vit_som_amd.LogisticRegression)
against the fp64 optimum and sklearn's pipeline, reproducibility, the memory contract of every new entry, and what is built
on top: evaluate_linear_probe and the driver's switch.

Tolerances.  R: 2^-23 absolute, one rounding of a value in [-1, 1].  fp64 sums of at most a few thousand terms (loss, gb,
phi, pen): 1e-12 relative to the largest reference value.  The solver: see test_solver_reaches_the_optimum."""
import copy
import functools
import signal

import numpy as np
import pytest
import torch

import linear_probe_ref as R
import memcheck as MC
from helpers import golden_params, load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL, MAX_ITER = 1e-5, 500
f32, f64, i64 = torch.float32, torch.float64, torch.int64


@pytest.fixture(autouse=True)
def time_limit(request):
    """A limit of its own for every test here, as in test_pca_gpu.py."""
    limit = 300 if "driver" in request.node.name else 120

    def expired(signum, frame):
        raise TimeoutError(f"{request.node.name}: no result after {limit} s")
    old = signal.signal(signal.SIGALRM, expired)
    signal.alarm(limit)
    yield
    signal.alarm(0)
    signal.signal(signal.SIGALRM, old)


def _dev(a, dtype=None):
    return torch.from_numpy(np.array(a, dtype=dtype)).to(DEV)               # a copy: the fixtures are read-only


def _host(t):
    return t.detach().cpu().numpy()


def _padded(A, pad, fill=float("nan")):
    """A on the device in rows of cols + pad elements, the padding filled."""
    A = np.asarray(A)
    Ad = _dev(A)
    buf = torch.full((A.shape[0], A.shape[1] + pad), fill, dtype=Ad.dtype, device=DEV)
    buf[:, :A.shape[1]] = Ad
    return buf[:, :A.shape[1]]


def _close(got, ref, what, rel=1e-12):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    err, top = float(np.abs(got - ref).max()), float(np.abs(ref).max())
    print(f"{what}: error {err:.3e} against {top:.3e} ({err / top if top else 0.0:.3e} relative)")
    assert err <= rel * top, what


def _logits(N, C, seed):
    """f32 logits with rows at +-80 and one saturated row, labels with one -1 and one C among them."""
    rng = np.random.RandomState(seed)
    Z = (3.0 * rng.standard_normal((N, C))).astype(np.float32)
    Z[3] = 80.0 * rng.choice([-1.0, 1.0], C)
    Z[4] = -80.0
    Z[5] = -80.0
    Z[5, C // 2] = 80.0                                  # saturated: one probability is 1, the others exp(-160)
    Z[6] = 80.0
    y = rng.randint(0, C, N).astype(np.int64)
    y[5] = C // 2
    b = rng.standard_normal(C)
    return Z, y, b


def _residual(Z, b, y, pad=3, pred=True, prob=True):
    from vit_som_amd import ops
    N, C = Z.shape
    out = dict(R=torch.full((N, C + 1), float("nan"), device=DEV)[:, :C], loss=torch.full((1,), float("nan"), dtype=f64, device=DEV),
               gb=torch.full((C,), float("nan"), dtype=f64, device=DEV), status=torch.zeros(1, dtype=torch.int32, device=DEV),
               pred=torch.full((N,), -7, dtype=i64, device=DEV) if pred else None,
               prob=torch.full((N, C), float("nan"), dtype=f64, device=DEV) if prob else None)
    ops.probe_residual(_padded(Z, pad), None if b is None else _dev(b), _dev(y), out["R"], out["loss"], out["gb"], out["status"],
                       out["pred"], out["prob"])
    return out


# ------------------------------------------------------------------ 1. kernels against fp64 numpy on the same f32 logits
# C = 2, 5, 17: rows packed 32, 8, 2 to a wave; 100 and 256: a row per wave with two and four columns per lane
ROW_CASES = [(257, 2), (257, 5), (515, 17), (130, 100), (66, 256), (2, 3), (4300, 10)]


@pytest.mark.parametrize("N,C", ROW_CASES)
def test_residual_against_fp64(N, C):
    Z, y, b = _logits(max(N, 8), C, seed=N + C)
    Z, y = Z[:N], y[:N]
    bad = y.copy()
    if N > 8:
        bad[1], bad[7] = -1, C
    out = _residual(Z, b, bad)
    Rr, loss, gb, pred, P = R.residual(Z, b, bad)
    assert int(out["status"]) == (2 if N > 8 else 0)
    assert np.abs(_host(out["R"]).astype(np.float64) - Rr.astype(np.float64)).max() <= 2.0 ** -23
    _close(_host(out["loss"]), [loss], "loss")
    _close(_host(out["gb"]), gb, "gb")
    assert np.array_equal(_host(out["pred"]), pred)
    assert np.abs(_host(out["prob"]) - P).max() <= 2.0 ** -48          # a few fp64 roundings (exp, the sum of C terms) of a value <= 1
    if N > 8:
        assert not _host(out["R"])[[1, 7]].any()
        # the two labels change no output but their own rows: every other row of R has the bits of a run with valid labels
        good = _residual(Z, b, y)
        keep = np.ones(N, bool)
        keep[[1, 7]] = False
        assert np.array_equal(_host(out["R"])[keep].view(np.int32), _host(good["R"])[keep].view(np.int32))
        assert np.array_equal(_host(out["pred"]), _host(good["pred"])) and torch.equal(out["prob"], good["prob"])
        assert int(good["status"]) == 0
    # without an intercept, and without the optional outputs
    plain = _residual(Z, None, bad, pad=0, pred=False, prob=False)
    Rr0, loss0, gb0, _, _ = R.residual(Z, None, bad)
    assert np.abs(_host(plain["R"]).astype(np.float64) - Rr0.astype(np.float64)).max() <= 2.0 ** -23
    _close(_host(plain["loss"]), [loss0], "loss without b")
    _close(_host(plain["gb"]), gb0, "gb without b")


@pytest.mark.parametrize("N,C", ROW_CASES)
def test_linesearch_ladder_against_fp64(N, C):
    from vit_som_amd import ops
    Z, y, b = _logits(max(N, 8), C, seed=3 * N + C)
    Z, y = Z[:N], y[:N]
    if N > 8:
        y[1], y[7] = -1, C
    rng = np.random.RandomState(C)
    Zp, pb, alpha0 = rng.standard_normal((N, C)).astype(np.float32), rng.standard_normal(C), 0.75
    phi = torch.full((16,), float("nan"), dtype=f64, device=DEV)
    ops.probe_linesearch(_padded(Z, 2), _padded(Zp, 2), _dev(b), _dev(pb), _dev(y), _dev([alpha0]), 16, phi)
    _close(_host(phi), R.ladder(Z, Zp, b, pb, y, alpha0, 16), "phi")
    short = torch.full((3,), float("nan"), dtype=f64, device=DEV)
    ops.probe_linesearch(_dev(Z), _dev(Zp), None, None, _dev(y), _dev([alpha0]), 3, short)
    _close(_host(short), R.ladder(Z, Zp, None, None, y, alpha0, 3), "phi, three steps, no intercept")


# ------------------------------------------------------------------ 2. the line search's identity, and the step
@pytest.mark.parametrize("N,C", [(257, 5), (130, 100)])
def test_linesearch_identity_and_the_step_chosen_on_the_device(N, C):
    """Z and Zp are multiples of 2^-6 below 8 and 4 and alpha_j = 2^-j, j < 8, so Z + alpha_j Zp is exact in f32: phi[j] and
    vsom_probe_residual's loss at that matrix are sums of the same fp64 terms."""
    from vit_som_amd import ops
    rng = np.random.RandomState(N)
    Z = (rng.randint(-512, 513, (N, C)) / 64.0).astype(np.float32)
    Zp = (rng.randint(-256, 257, (N, C)) / 64.0).astype(np.float32)
    y, b, pb = rng.randint(0, C, N).astype(np.int64), rng.standard_normal(C), rng.standard_normal(C)
    D = 7
    n = C * D + C
    theta, p = rng.standard_normal(n), rng.standard_normal(n)
    theta[C * D:], p[C * D:] = b, pb
    Zd, Zpd, yd = _padded(Z, 3), _padded(Zp, 3), _dev(y)
    phi = torch.empty(8, dtype=f64, device=DEV)
    ops.probe_linesearch(Zd, Zpd, _dev(b), _dev(pb), yd, _dev([1.0]), 8, phi)
    phi = _host(phi)
    for j in range(8):
        a = 2.0 ** -j
        Zj = Z + np.float32(a) * Zp
        assert np.array_equal(Zj.astype(np.float64), Z.astype(np.float64) + a * Zp.astype(np.float64))
        _close([phi[j]], _host(_residual(Zj, b + a * pb, y, pred=False, prob=False)["loss"]), f"phi[{j}] against the residual's loss")
    f0 = float(_residual(Z, b, y, pred=False, prob=False)["loss"])
    lam, pen = 0.01, np.array([3.0, -0.5, 2.0])
    cases = ((-1.0, 1e9, 0), (-1e-3, f0, None), (-1e-6, float(phi[3]) + 1.0, 0), (1.0, f0, 2), (-1.0, -1e9, 1))
    for gtp, f0_here, want_status in cases:
        rec = torch.zeros(16, dtype=f64, device=DEV)
        Zrun, th, s = _padded(Z, 3), _dev(theta), torch.full((n,), float("nan"), dtype=f64, device=DEV)
        ops.probe_step(_dev(phi), _dev([1.0]), _dev([f0_here]), _dev(pen), _dev([gtp]), lam, 1e-4, Zrun, Zpd, th, _dev(p), s, rec)
        alpha, status, F, j = R.armijo(phi, 1.0, f0_here, pen, gtp, N, lam)
        got = _host(rec)
        print(f"gtp {gtp}: device alpha {got[12]}, status {got[13]}, F {got[14]}, j {got[15]}; host {alpha, status, F, j}")
        assert (got[12], int(got[13]), got[14], int(got[15])) == (alpha, status, F, j)
        assert want_status is None or status == want_status
        assert not got[:12].any()
        assert np.array_equal(_host(Zrun), (Z.astype(np.float64) + alpha * Zp.astype(np.float64)).astype(np.float32))
        assert np.array_equal(_host(th), theta + alpha * p) and np.array_equal(_host(s), alpha * p)
        assert bool(torch.isnan(Zrun.as_strided((N, 3), (C + 3, 1), C)).all())        # the padding columns are not touched


# ------------------------------------------------------------------ fold and gradient
@pytest.mark.parametrize("C,D", [(5, 131), (17, 260), (100, 2051)])
def test_fold_and_gradient(C, D):
    from vit_som_amd import ops
    rng = np.random.RandomState(D)
    A, W, invstd = rng.standard_normal((C, D)), rng.standard_normal((C, D)), rng.uniform(0.5, 2.0, D)
    invstd[3] = 0.0                                        # a constant column
    B = torch.full((C, D + 3), float("nan"), device=DEV)[:, :D]
    pen = torch.full((3,), float("nan"), dtype=f64, device=DEV)
    ops.probe_fold(_dev(A), _dev(invstd), B, _dev(W), pen)
    assert np.array_equal(_host(B), (A * invstd).astype(np.float32))
    _close(_host(pen), [(W * W).sum(), (W * A).sum(), (A * A).sum()], "pen")
    Ai, Wi = rng.randint(-3, 4, (C, D)).astype(np.float64), rng.randint(-3, 4, (C, D)).astype(np.float64)
    ops.probe_fold(_dev(Ai), _dev(invstd), B, _dev(Wi), pen)
    assert np.array_equal(_host(pen), [(Wi * Wi).sum(), (Wi * Ai).sum(), (Ai * Ai).sum()])      # integers: exact in any order
    B2 = torch.empty(C, D, device=DEV)
    ops.probe_fold(_dev(A), _dev(invstd), B2)                           # without the penalty's products
    assert np.array_equal(_host(B2), (A * invstd).astype(np.float32))
    # the gradient
    N, lam = 300, 1.0 / (0.7 * 300)
    Zt, gb = rng.standard_normal((C, D)).astype(np.float32), rng.standard_normal(C)
    theta, g_prev = np.concatenate([W.ravel(), rng.standard_normal(C)]), rng.standard_normal(C * D + C)
    g, yn = torch.full((C * D + C,), float("nan"), dtype=f64, device=DEV), torch.full((C * D + C,), float("nan"), dtype=f64, device=DEV)
    ops.probe_gradient(_padded(Zt, 5), _dev(invstd), _dev(theta), _dev(gb), N, lam, g, _dev(g_prev), yn)
    want = np.concatenate([(Zt.astype(np.float64) * invstd / N + lam * W).ravel(), gb / N])
    _close(_host(g), want, "gradient", rel=2.0 ** -48)                   # a handful of fp64 roundings per element
    assert np.array_equal(_host(yn), _host(g) - g_prev)
    g0 = torch.empty(C * D, dtype=f64, device=DEV)
    ops.probe_gradient(_dev(Zt), _dev(invstd), _dev(W.ravel()), None, N, lam, g0)               # no intercept, no pair
    assert np.array_equal(_host(g0), _host(g)[:C * D])


# ------------------------------------------------------------------ 3. the L-BFGS pieces
class _Lbfgs:
    """The three launches of one iteration, with the caller's buffers."""

    def __init__(self, n, m):
        from vit_som_amd import ops
        self.ops, self.n, self.m = ops, n, m
        self.S, self.Y = (torch.full((m, n), float("nan"), dtype=f64, device=DEV) for _ in range(2))
        self.state = ops.lbfgs_state(m, DEV)
        self.dots = torch.full((3 * (2 * m + 3) + 1,), float("nan"), dtype=f64, device=DEV)
        self.p = torch.full((n,), float("nan"), dtype=f64, device=DEV)

    def step(self, g, s=None, y=None):
        g, s, y = _dev(g), (None if s is None else _dev(s)), (None if y is None else _dev(y))
        self.ops.lbfgs_dots(self.S, self.Y, g, s, y, self.state, self.dots)
        self.ops.lbfgs_coeff(self.dots, self.m, s is not None, self.state)
        hold = torch.zeros(self.n, dtype=f64, device=DEV)
        self.ops.lbfgs_combine(self.S, self.Y, g, hold if s is None else s, hold if y is None else y, self.state, self.p)
        return _host(self.p), _host(self.state[:16]), _host(self.dots)


@pytest.mark.parametrize("n,m", [(5000, 4), (700, 10), (70001, 3)])
def test_lbfgs_direction_is_the_two_loop_recursion(n, m):
    """Integer-valued vectors: every dot product is exact in any order.  Seven pairs: a history shorter than m, a full one and
    (m = 3, 4) a wrapped-around one; pair 4 has s.y < 0 and must be skipped and counted."""
    rng = np.random.RandomState(n)
    L = _Lbfgs(n, m)
    g = rng.randint(-4, 5, n).astype(np.float64)
    p, rec, dots = L.step(g)
    assert np.array_equal(p, -g) and rec[1] == -(g @ g) and rec[2] == g @ g and rec[3] == np.abs(g).max() and rec[4] == 0
    assert abs(rec[0] - min(1.0, 1.0 / np.sqrt(g @ g))) <= 1e-15
    pairs, skipped = [], 0
    for k in range(7):
        s = rng.randint(-3, 4, n).astype(np.float64)
        y = 2.0 * s + rng.randint(-2, 3, n)
        if k == 4:
            y = -y
        g = rng.randint(-4, 5, n).astype(np.float64)
        p, rec, dots = L.step(g, s, y)
        NV = 2 * m + 3
        assert dots[2 * m + 1] == s @ s and dots[2 * m + 2] == s @ y and dots[NV + 2 * m + 2] == y @ y
        assert dots[2 * NV + 2 * m] == g @ g and dots[2 * NV + 2 * m + 1] == g @ s and dots[3 * NV] == np.abs(g).max()
        if s @ y > 0:
            pairs = (pairs + [(s, y)])[-m:]
        else:
            skipped += 1
        want = R.two_loop(pairs, g)
        err = np.abs(p - want).max() / np.abs(want).max()
        print(f"pair {k}: {len(pairs)} held, direction error {err:.2e}")
        assert err <= 1e-12
        assert (rec[0], rec[4], rec[5], rec[6]) == (1.0, len(pairs), skipped, float(s @ y > 0))
        assert abs(rec[1] - g @ want) <= 1e-12 * abs(g @ want) and rec[3] == np.abs(g).max()
    assert skipped == 1
    # a restart empties the history
    p, rec, _ = L.step(g)
    assert np.array_equal(p, -g) and rec[4] == 0 and rec[5] == skipped


def test_lbfgs_direction_is_bitwise_where_the_arithmetic_is_exact():
    """s has 1024 entries of +-1, y = 4 s: s.y, y.y and every quotient are powers of two, the vectors hold small integers, so
    the textbook recursion and the coefficient form round nowhere and must agree bit for bit; likewise with a second such
    pair on disjoint entries."""
    n, m = 5000, 4
    rng = np.random.RandomState(9)
    L = _Lbfgs(n, m)
    g = rng.randint(-4, 5, n).astype(np.float64)
    L.step(g)
    pairs = []
    for k in range(2):
        s = np.zeros(n)
        s[1024 * k:1024 * (k + 1)] = rng.choice([-1.0, 1.0], 1024)
        pairs.append((s, 4.0 * s))
        g = rng.randint(-4, 5, n).astype(np.float64)
        p, rec, _ = L.step(g, s, 4.0 * s)
        assert np.array_equal(p, R.two_loop(pairs, g)) and rec[1] == g @ p


# ------------------------------------------------------------------ 4. the solver
def _device_rows(name):
    X, y, Xh, yh = R.fixture(name)
    pad = R.FIXTURES[name][5]
    return (_padded(X, pad) if pad else _dev(X)), _dev(y), (_padded(Xh, pad) if pad else _dev(Xh)), _dev(yh)


@functools.lru_cache(maxsize=None)
def _fit(name, C_reg):
    from vit_som_amd import LogisticRegression
    X, y, _, _ = _device_rows(name)
    assert X.stride(0) == R.FIXTURES[name][1] + R.FIXTURES[name][5]
    return LogisticRegression(C=C_reg, tol=TOL, max_iter=MAX_ITER).fit(X, y)


@functools.lru_cache(maxsize=None)
def _emulated_gap(name, C_reg):
    X, y, _, _ = R.fixture(name)
    W, b, mean, scale, n_iter, _ = R.emulate(X, y, R.FIXTURES[name][2], C_reg, TOL, MAX_ITER)
    return R.objective_at(W, b, X, y, mean, scale, C_reg)[0] - R.optimum(name, C_reg)[2], n_iter


@pytest.mark.parametrize("C_reg", [1.0, 100.0])
@pytest.mark.parametrize("name", sorted(R.FIXTURES))
def test_solver_reaches_the_optimum(name, C_reg):
    """tol = 1e-5, max_iter = 500.  converged_; the device's own gradient (a fresh project) at most tol; the fp64 gradient
    numpy computes at the returned parameters at most 2 tol; the fp64 objective there within
    4 x max(gap of the float32 host emulation at the same tol, 1e-9) of scipy's optimum."""
    X, y, _, _ = R.fixture(name)
    N, D, C = R.FIXTURES[name][:3]
    clf = _fit(name, C_reg)
    assert clf.converged_ and clf.grad_norm_ <= TOL and 0 < clf.n_iter_ < MAX_ITER
    assert clf.coef_.shape == (C, D) and clf.intercept_.shape == (C,) and clf.coef_.dtype == torch.float64
    assert clf.n_skipped_pairs_ >= 0 and clf.n_features_in_ == D
    mean, scale = R.standardise(X)
    assert np.abs(_host(clf.mean_).astype(np.float64) - mean).max() <= 2.0 ** -23 * np.abs(mean).max()
    assert np.allclose(_host(clf.scale_), scale, rtol=1e-9)
    F, gmax = R.objective_at(_host(clf.coef_), _host(clf.intercept_), X, y, _host(clf.mean_), _host(clf.scale_), C_reg)
    Fopt = R.optimum(name, C_reg)[2]
    gap_emulated, it_emulated = _emulated_gap(name, C_reg)
    print(f"{name} C={C_reg}: {clf.n_iter_} iterations (emulation {it_emulated}), {clf.n_skipped_pairs_} pairs skipped, "
          f"{clf.n_restarts_} restarts; device gradient {clf.grad_norm_:.3e}, fp64 gradient {gmax:.3e}; "
          f"gap to the optimum {F - Fopt:.3e}, emulation's gap {gap_emulated:.3e}; loss_ {clf.loss_:.12f}, fp64 {F:.12f}")
    assert gmax <= 2 * TOL
    # loss_ comes from f32 logits: the cross-entropy moves by at most twice the largest logit error
    Xs = (X.astype(np.float64) - _host(clf.mean_)) / _host(clf.scale_)
    dz = np.abs(_host(clf.decision_function(_device_rows(name)[0])) - (Xs @ _host(clf.coef_).T + _host(clf.intercept_))).max()
    assert abs(clf.loss_ - F) <= 2 * dz + 1e-12
    assert F - Fopt <= 4 * max(gap_emulated, 1e-9)


# ------------------------------------------------------------------ 5. predictions
@pytest.mark.parametrize("name", sorted(R.FIXTURES))
def test_predictions_are_the_sklearn_pipelines(name):
    """On every row whose fp64 top-two margin at the optimum exceeds 1e-3; at most 2 % of the rows may be left out."""
    X, y, Xh, yh = R.fixture(name)
    Xd, yd, Xhd, yhd = _device_rows(name)
    clf, pipe = _fit(name, 1.0), R.sklearn_pipeline(name, 1.0)
    W, b, _ = R.optimum(name, 1.0)
    mean, scale = R.standardise(X)
    for rows, rows_d, labels_d in ((X, Xd, yd), (Xh, Xhd, yhd)):
        keep = R.margins(W, b, (rows.astype(np.float64) - mean) / scale) > 1e-3
        assert (~keep).mean() <= 0.02
        pred = _host(clf.predict(rows_d))
        assert np.array_equal(pred[keep], pipe.predict(rows.astype(np.float64))[keep])
        proba = _host(clf.predict_proba(rows_d))
        assert np.array_equal(proba.argmax(axis=1), pred) and np.abs(proba.sum(axis=1) - 1).max() <= 1e-12
        dec = _host(clf.decision_function(rows_d))
        assert dec.dtype == np.float64 and np.array_equal(dec.argmax(axis=1), pred)
        assert clf.score(rows_d, labels_d) == float((pred == _host(labels_d)).mean())
    assert torch.equal(clf.predict(Xd[:1]), clf.predict(Xd)[:1])


def test_two_classes_no_intercept_and_warnings():
    from vit_som_amd import LogisticRegression
    from vit_som_amd.linear_probe import ConvergenceWarning
    X, y, _, _ = R.fixture("shifted")
    Xd, y2 = _dev(X), _dev((y > 0).astype(np.int64))
    clf = LogisticRegression(tol=TOL, max_iter=MAX_ITER).fit(Xd, y2)
    assert clf.converged_ and clf.coef_.shape == (2, X.shape[1])                      # the softmax form is kept
    assert float((clf.coef_[0] + clf.coef_[1]).abs().max()) <= 1e-3 * float(clf.coef_.abs().max())
    flat = LogisticRegression(tol=TOL, max_iter=MAX_ITER, fit_intercept=False, standardize=False).fit(Xd - 50.0, _dev(y))
    assert flat.converged_ and not bool(flat.intercept_.any()) and bool((flat.scale_ == 1).all())
    with pytest.warns(ConvergenceWarning, match="Increase the number of iterations"):
        short = LogisticRegression(tol=1e-9, max_iter=2).fit(Xd, _dev(y))
    assert short.n_iter_ == 2 and not short.converged_
    # a tolerance that cannot be met: the fit ends at the floor of the f32 contractions (a line search without a passing
    # step restarts from -g, two in a row end it) or at max_iter, with the warning and finite results
    with pytest.warns(ConvergenceWarning):
        floor = LogisticRegression(tol=0.0, max_iter=150).fit(Xd, _dev(y))
    print(f"tol 0: {floor.n_iter_} iterations, {floor.n_restarts_} restarts, {floor.n_skipped_pairs_} pairs skipped, "
          f"max |gradient| {floor.grad_norm_:.3e}, loss {floor.loss_:.12f}")
    assert not floor.converged_ and 2 < floor.n_iter_ <= 150 and floor.n_skipped_pairs_ >= 0
    assert np.isfinite(floor.loss_) and floor.grad_norm_ <= TOL and bool(torch.isfinite(floor.coef_).all())
    with pytest.raises(ValueError, match=r"labels outside \[0, 2\)"):
        LogisticRegression(n_classes=2).fit(Xd, _dev(y))
    with pytest.raises(ValueError, match="inconsistent numbers of samples"):
        LogisticRegression().fit(Xd, _dev(y[:-1]))
    with pytest.raises(ValueError, match="X has 5 features, but LogisticRegression is expecting 64 features as input."):
        clf.predict(torch.zeros(3, 5, device=DEV))
    with pytest.raises(ValueError, match=r"n_classes=70 > min\(256, n_features=64\)"):
        LogisticRegression(n_classes=70).fit(Xd, _dev(y))


# ------------------------------------------------------------------ 6. reproducibility
@pytest.mark.parametrize("name,pad", [("odd", 3), ("shifted", 4)])
def test_a_fit_is_bitwise_reproducible(name, pad):
    """Twice the same bits; and the same bits with X in a padded buffer of another stride that keeps the load path (D = 131:
    element-wise at a stride of 134 as at 131; D = 64: 16-byte loads at a stride of 68 as well)."""
    from vit_som_amd import LogisticRegression
    X, y, _, _ = R.fixture(name)
    first = _fit(name, 1.0)
    for Xd in (_dev(X), _padded(X, pad)):
        again = LogisticRegression(C=1.0, tol=TOL, max_iter=MAX_ITER).fit(Xd, _dev(y))
        assert again.n_iter_ == first.n_iter_ and again.loss_ == first.loss_ and again.grad_norm_ == first.grad_norm_
        assert torch.equal(again.coef_.view(i64), first.coef_.view(i64))
        assert torch.equal(again.intercept_.view(i64), first.intercept_.view(i64))


# ------------------------------------------------------------------ 7. the memory contract of every new entry
def _bits(t):
    t = t.contiguous()
    return t.view({4: torch.int32, 8: torch.int64}[t.element_size()])


ENTRIES = ["fold", "residual", "linesearch", "step", "gradient", "lbfgs_dots", "lbfgs_coeff", "lbfgs_combine"]


@pytest.mark.parametrize("fill", MC.FILLS)
@pytest.mark.parametrize("entry", ENTRIES)
def test_memory_contract(monkeypatch, entry, fill):
    """(N, D, C) = (257, 131, 5), memory 3: outputs in guard-banded poisoned buffers, scratch of exactly the queried size and
    pre-filled, f32 matrices in padded rows whose padding is poisoned.  Guards intact, every output element written, the
    result bit for bit that of the plain run."""
    from vit_som_amd import ops
    N, D, C, m, PAD = 257, 131, 5, 3, 3
    n = C * D + C
    rng = np.random.RandomState(23)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))                  # noqa: E731
    inp = dict(Z=t(rng.standard_normal((N, C)).astype(np.float32)), Zp=t(rng.standard_normal((N, C)).astype(np.float32)),
               Zt=t(rng.standard_normal((C, D)).astype(np.float32)), A=t(rng.standard_normal((C, D))), W=t(rng.standard_normal((C, D))),
               invstd=t(rng.uniform(0.5, 2.0, D)), b=t(rng.standard_normal(C)), pb=t(rng.standard_normal(C)),
               y=t(rng.randint(0, C, N).astype(np.int64)), theta=t(rng.standard_normal(n)), p=t(rng.standard_normal(n)),
               g=t(rng.standard_normal(n)), g_prev=t(rng.standard_normal(n)), gb=t(rng.standard_normal(C)),
               s_new=t(rng.standard_normal(n)), phi=t(np.linspace(400.0, 380.0, 16)), one=t(np.array([1.0])),
               f0=t(np.array([395.0])), pen=t(np.array([3.0, -0.5, 2.0])), gtp=t(np.array([-50.0])))
    inp["y_new"] = 2.0 * inp["s_new"] + 0.1 * t(rng.standard_normal(n))
    S0, Y0 = t(rng.standard_normal((m, n))), t(rng.standard_normal((m, n)))
    # a state with two pairs held, made by the pieces themselves on the plain path
    state0, dots0 = ops.lbfgs_state(m, DEV), torch.zeros(3 * (2 * m + 3) + 1, dtype=f64, device=DEV)
    Sd, Yd = S0.to(DEV), Y0.to(DEV)
    ops.lbfgs_dots(Sd, Yd, inp["g"].to(DEV), None, None, state0, dots0)
    ops.lbfgs_coeff(dots0, m, False, state0)
    for k in range(2):
        s_k = Sd[2].clone() + k
        ops.lbfgs_dots(Sd, Yd, inp["g"].to(DEV), s_k, 3.0 * s_k, state0, dots0)
        ops.lbfgs_coeff(dots0, m, True, state0)
        ops.lbfgs_combine(Sd, Yd, inp["g"].to(DEV), s_k, 3.0 * s_k, state0, torch.empty(n, dtype=f64, device=DEV))
    ops.lbfgs_dots(Sd, Yd, inp["g"].to(DEV), inp["s_new"].to(DEV), inp["y_new"].to(DEV), state0, dots0)
    S0, Y0 = Sd.cpu(), Yd.cpu()
    n_state, n_dots = state0.numel(), dots0.numel()

    # name -> (shape, dtype, ld, initial value or None): outputs, and the buffers an entry updates in place
    shapes = {
        "fold": {"B": ((C, D), f32, D + PAD, None), "pen": ((3,), f64, None, None)},
        "residual": {"R": ((N, C), f32, C + PAD, None), "loss": ((1,), f64, None, None), "gb": ((C,), f64, None, None),
                     "pred": ((N,), i64, None, None), "prob": ((N, C), f64, None, None)},
        "linesearch": {"phi_out": ((16,), f64, None, None)},
        "step": {"Zio": ((N, C), f32, C + PAD, inp["Z"]), "theta_io": ((n,), f64, None, inp["theta"]), "s_out": ((n,), f64, None, None),
                 "rec": ((16,), f64, None, torch.zeros(16, dtype=f64))},
        "gradient": {"g_out": ((n,), f64, None, None), "y_out": ((n,), f64, None, None)},
        "lbfgs_dots": {"dots": ((n_dots,), f64, None, None)},
        "lbfgs_coeff": {"state": ((n_state,), f64, None, state0.cpu())},
        "lbfgs_combine": {"S": ((m, n), f64, None, S0), "Y": ((m, n), f64, None, Y0), "p_out": ((n,), f64, None, None)},
    }[entry]

    def run(i, o):
        status = torch.zeros(1, dtype=torch.int32, device=DEV)
        if entry == "fold":
            ops.probe_fold(i["A"], i["invstd"], o["B"], i["W"], o["pen"])
        elif entry == "residual":
            ops.probe_residual(i["Z"], i["b"], i["y"], o["R"], o["loss"], o["gb"], status, o["pred"], o["prob"])
        elif entry == "linesearch":
            ops.probe_linesearch(i["Z"], i["Zp"], i["b"], i["pb"], i["y"], i["one"], 16, o["phi_out"])
        elif entry == "step":
            ops.probe_step(i["phi"], i["one"], i["f0"], i["pen"], i["gtp"], 0.01, 1e-4, o["Zio"], i["Zp"], o["theta_io"], i["p"],
                           o["s_out"], o["rec"])
        elif entry == "gradient":
            ops.probe_gradient(i["Zt"], i["invstd"], i["theta"], i["gb"], N, 0.01, o["g_out"], i["g_prev"], o["y_out"])
        elif entry == "lbfgs_dots":
            ops.lbfgs_dots(i["S"], i["Y"], i["g"], i["s_new"], i["y_new"], i["state"], o["dots"])
        elif entry == "lbfgs_coeff":
            ops.lbfgs_coeff(i["dots"], m, True, o["state"])
        else:
            ops.lbfgs_combine(o["S"], o["Y"], i["g"], i["s_new"], i["y_new"], i["state"], o["p_out"])

    state1 = state0.clone()                                # the state after the third pair's coeff: what combine reads
    ops.lbfgs_coeff(dots0, m, True, state1)
    extra = dict(S=S0, Y=Y0, state=state1.cpu() if entry == "lbfgs_combine" else state0.cpu(), dots=dots0.cpu())
    plain_in = {k: v.to(DEV) for k, v in {**inp, **extra}.items()}
    plain = {}
    for k, (shape, dt, _, init) in shapes.items():
        plain[k] = torch.empty(shape, dtype=dt, device=DEV) if init is None else init.to(DEV).clone()
    run(plain_in, plain)
    torch.cuda.synchronize()

    es = MC.ExactScratch(fill)
    handles, gin, outs = {}, {}, {}
    for k, v in {**inp, **extra}.items():
        ld = v.shape[1] + PAD if v.dtype == f32 and v.dim() == 2 else None
        gin[k], handles[k] = MC.guarded_copy(v.to(DEV), ld=ld)
    for k, (shape, dt, ld, init) in shapes.items():
        outs[k], handles["out " + k] = MC.guarded(shape, dt, DEV, ld=ld)
        if init is not None:
            outs[k].copy_(init.to(DEV))
    if entry == "step":
        gin["Zp"], handles["Zp"] = MC.guarded_copy(inp["Zp"].to(DEV), ld=C + PAD)      # the row stride of Z
    with monkeypatch.context() as mp:
        mp.setattr(ops, "scratch", es)
        run(gin, outs)
    torch.cuda.synchronize()
    need = {"fold": 8 * ops.lib.vsom_probe_fold_parts(C, D), "residual": 8 * ops.probe_parts(N, C),
            "linesearch": 8 * ops.probe_parts(N, C), "lbfgs_dots": 8 * ops.lib.vsom_lbfgs_parts(n, m)}
    assert (es.calls > 0) == (entry in need)
    if es.calls:
        assert [key[2] for key in es.arenas] == [need[entry]]
    es.check()
    for name, h in handles.items():
        h.check(f"[{fill}] {name}")
    for k, v in {**inp, **extra}.items():
        assert torch.equal(_bits(gin[k]), _bits(v.to(DEV))), f"[{fill}] input {k} was written"
    for k in shapes:
        handles["out " + k].all_written(f"[{fill}] {k}")
        assert torch.equal(_bits(outs[k]), _bits(plain[k])), f"[{fill}] {k} differs from the plain run"
    if entry == "step":
        assert float(outs["rec"][12]) > 0 and not torch.equal(outs["Zio"], inp["Z"].to(DEV))     # a step was taken
    if entry == "lbfgs_combine":
        assert float(state1[6]) == 1.0 and not torch.equal(outs["S"], S0.to(DEV))                 # the pair went into its slot


def test_scratch_one_element_short_is_refused():
    """VSOM_EWORKSPACE from every entry with scratch, on real device buffers, before anything is written."""
    from vit_som_amd import ops
    L = ops.lib
    N, C, D, m = 257, 5, 131, 3
    n = C * D + C
    Z, R_ = torch.zeros(N, C, device=DEV), torch.full((N, C), 7.0, device=DEV)
    d = lambda k, v=0.0: torch.full((k,), v, dtype=f64, device=DEV)             # noqa: E731
    y, st = torch.zeros(N, dtype=i64, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    loss, gb, phi, pen, dots = d(1, 7.0), d(C, 7.0), d(16, 7.0), d(3, 7.0), d(3 * (2 * m + 3) + 1, 7.0)
    p = lambda t: t.data_ptr()                                                   # noqa: E731
    need = ops.probe_parts(N, C)
    part = d(max(need, L.vsom_lbfgs_parts(n, m), L.vsom_probe_fold_parts(C, D)))
    rows = need // 16
    assert L.vsom_probe_residual(p(Z), C, N, C, None, p(y), p(R_), C, p(loss), p(gb), None, None, p(st), p(part), rows * (C + 1) - 1, None) == -4
    assert L.vsom_probe_linesearch(p(Z), p(Z), C, N, C, None, None, p(y), p(d(1, 1.0)), 16, p(phi), p(part), need - 1, None) == -4
    A, B = d(C * D), torch.full((C, D), 7.0, device=DEV)
    assert L.vsom_probe_fold(p(A), p(d(D, 1.0)), C, D, p(B), D, p(A), p(pen), p(part), L.vsom_probe_fold_parts(C, D) - 1, None) == -4
    S, state = d(m * n), ops.lbfgs_state(m, DEV)
    assert L.vsom_lbfgs_dots(p(S), p(S), p(d(n)), p(d(n)), p(d(n)), n, m, 1, p(state), p(dots), p(part), L.vsom_lbfgs_parts(n, m) - 1, None) == -4
    torch.cuda.synchronize()
    for out in (R_, loss, gb, phi, pen, dots, B):
        assert bool((out == 7.0).all())


# ------------------------------------------------------------------ 8. the top of the stack
def _model(name):
    import vit_som_amd
    z, cfg = load_golden(name)
    m = vit_som_amd.ViTSOM(copy.deepcopy(cfg), device=DEV)
    m.load_state_dict(golden_params(z))
    return m, cfg


def _trained(steps):
    """The tiny classification model after `steps` fused steps (the third records the launch tape) -> (model, cfg, step)."""
    m, cfg = _model("ref_cls_tiny")
    d = cfg["data"]
    m.set_schedule(120, 100)
    (opt,), _ = m.configure_optimizers()
    g = torch.Generator().manual_seed(0)

    def step():
        x = torch.rand(5, d["num_channels"], d["input_size"], d["input_size"], generator=g).to(DEV)
        loss = m.train_step_fused(x, torch.randint(0, 5, (5,), generator=g).to(DEV))
        opt.step()
        return loss
    m.train()
    for _ in range(steps):
        step()
    return m, cfg, step


def test_evaluate_linear_probe_on_the_tiny_fixture():
    from test_knn_gpu import _features, _loaders
    from vit_som_amd import LinearProbeReport, LogisticRegression, evaluate_linear_probe
    m, cfg, step = _trained(3)
    twin, _, twin_step = _trained(3)
    assert torch.equal(m.arena.params, twin.arena.params)
    train, test = _loaders(cfg, 5)
    rep = evaluate_linear_probe(m, cfg, train, test, tol=1e-4, max_iter=200)
    assert m.training                                                   # the mode it was in
    assert isinstance(rep, LinearProbeReport) and (rep.n_train, rep.n_test) == (120, 40)
    assert rep.confusion.shape == (5, 5) and rep.confusion.dtype == np.int64 and rep.confusion.sum() == rep.n_test == 40
    with np.errstate(invalid="ignore"):
        assert np.array_equal(rep.per_class_accuracy, np.diag(rep.confusion) / rep.confusion.sum(axis=1), equal_nan=True)
    assert rep.accuracy == np.diag(rep.confusion).sum() / 40 and rep.fit_time > 0 and rep.inference_time > 0
    assert rep.converged and 0 < rep.n_iter <= 200 and np.isfinite(rep.loss)
    m.eval()
    X, y = _features(m, cfg, train)
    Q, yq = _features(m, cfg, test)
    clf = LogisticRegression(tol=1e-4, max_iter=200, n_classes=5).fit(X, y)
    assert rep.accuracy == clf.score(Q, yq) and rep.train_accuracy == clf.score(X, y) and rep.n_iter == clf.n_iter_
    assert rep.loss == clf.loss_
    cm = np.zeros((5, 5), dtype=np.int64)
    np.add.at(cm, (_host(yq), _host(clf.predict(Q))), 1)
    assert np.array_equal(rep.confusion, cm)
    assert evaluate_linear_probe(m, cfg, train, test, max_rows=60, max_iter=200).n_train == 60
    with pytest.raises(ValueError, match="labels outside"):
        evaluate_linear_probe(m, cfg, train, test, num_labels=3)
    # a training step after the call is bit for bit the step of a model that was never probed
    m.train()
    a, b = step(), twin_step()
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    assert torch.equal(m.arena.params, twin.arena.params) and torch.equal(m.arena.exp_avg, twin.arena.exp_avg)


def test_driver_reports_linear_probe_accuracy(tmp_path):
    from vit_som_amd.train import main, synthetic_loaders
    _, cfg = load_golden("ref_cluster_tiny")
    cfg = copy.deepcopy(cfg)
    cfg["hyperparameters"]["batch_size"] = 16
    logs = []
    loaders = lambda c, r, w: synthetic_loaders(c, r, w, n_train=64, n_val=16, n_test=16)      # noqa: E731
    today = {"accuracy", "precision", "recall", "f1", "purity", "nmi", "run_duration", "inference_time"}
    met = main(cfg, n_runs=1, max_epochs=1, make_loaders=loaders, model_states_dir=str(tmp_path / "a"), log=logs.append,
               linear_probe=True)
    assert set(met) == today | {"linear_probe_accuracy"}
    (acc,) = met["linear_probe_accuracy"]
    assert np.isfinite(acc) and 0.0 <= acc <= 1.0
    assert len(met["purity"]) == 1 and any("Linear probe: accuracy" in l for l in logs)
