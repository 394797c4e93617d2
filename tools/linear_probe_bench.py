"""Timing of the linear probe at the sizes users run (profiles/r17_linear_probe.txt).

    python tools/linear_probe_bench.py [--out profiles/r17_linear_probe.txt] [--repeats 7] [--rows 10000 50000]
                                       [--classes 10 100] [--no-sklearn] [--tests-log LOG]

kernels: every launch of one L-BFGS iteration at N rows, D = 12 288, C classes, on its own: the two passes over X
(ops.pca_project, ops.pca_backproject), the row-local kernels (probe_residual, probe_linesearch with its ladder of 16,
probe_step), the vector kernels (probe_fold with the penalty's products, probe_gradient) and the three L-BFGS launches at a
full memory of 10; alternated in one process, one warm-up round, device events around each call.  The two passes are set
against X read once at 6.3 TB/s.  The share of an iteration spent outside the two passes is reported as it comes out.
end to end: LogisticRegression().fit by wall clock around calls that end in a device synchronise, and the time per iteration
that follows from it (launch overhead and the one host read per iteration included).
sklearn (skipped with --no-sklearn): Pipeline(StandardScaler(), LogisticRegression()) on the host once at N = 3 000, C = 10,
for scale.
--tests-log: the lines of a `pytest -s tests/test_linear_probe_gpu.py` log that state the solver's gaps are copied in.
Everything is printed and written to --out."""
import argparse
import os
import statistics
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_TBS = 6.3
D = 12288
MEMORY = 10


def _row(say, name, t, unit="ms"):
    med = statistics.median(t)
    say(f"{name:30s} " + " ".join(f"{v:9.3f}" for v in t) + f"   median {med:9.3f}  min {min(t):9.3f}  max {max(t):9.3f}  "
        f"spread {(max(t) - min(t)) / med:.4f}  ({unit})")
    return med


def data(N, C, device="cuda"):
    """Rows are class mean plus unit noise plus a column mean; the class means are small, so the classes overlap."""
    import torch
    g = torch.Generator(device=device).manual_seed(0)
    means = 0.05 * torch.randn(C, D, device=device, generator=g)
    y = torch.randint(0, C, (N,), device=device, generator=g)
    X = means[y]
    X.add_(torch.randn(N, D, device=device, generator=g)).add_(0.5)
    return X, y


def kernels(N, C, repeats, say):
    import torch
    from vit_som_amd import LogisticRegression, ops
    X, y = data(N, C)
    dev, m = X.device, MEMORY
    n = C * D + C
    f64 = lambda *s: torch.randn(*s, dtype=torch.float64, device=dev) * 1e-2           # noqa: E731
    mean, var = ops.pca_colstats(X)
    invstd = (1.0 / torch.sqrt(var * ((N - 1) / N))).contiguous()
    theta, p, s_new, g, g_prev, y_new = f64(n), f64(n), f64(n), f64(n), f64(n), f64(n)
    W, P, b, pb = theta[:C * D].view(C, D), p[:C * D].view(C, D), theta[C * D:], p[C * D:]
    pad = lambda: torch.zeros(N, (C + 3) // 4 * 4, device=dev)[:, :C]                 # noqa: E731
    Z, Zp, R = pad(), pad(), pad()
    Bf, Zt = torch.empty(C, D, device=dev), torch.empty(C, D, device=dev)
    loss, gb, pen, phi = (torch.zeros(k, dtype=torch.float64, device=dev) for k in (1, C, 3, 16))
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    S, Y = f64(m, n), f64(m, n)
    Y.copy_(2.0 * S + 0.1 * Y)
    state, dots = ops.lbfgs_state(m, dev), torch.zeros(3 * (2 * m + 3) + 1, dtype=torch.float64, device=dev)
    ops.lbfgs_dots(S, Y, g, None, None, state, dots)
    ops.lbfgs_coeff(dots, m, False, state)
    for k in range(m):                                    # fill the memory through the pieces themselves
        s_k = S[k].clone()
        ops.lbfgs_dots(S, Y, g, s_k, 2.0 * s_k, state, dots)
        ops.lbfgs_coeff(dots, m, True, state)
        ops.lbfgs_combine(S, Y, g, s_k, 2.0 * s_k, state, p)
    y_new.copy_(2.0 * s_new)
    one, gtp = torch.ones(1, dtype=torch.float64, device=dev), -torch.ones(1, dtype=torch.float64, device=dev)
    f_big = torch.full((1,), 1e30, dtype=torch.float64, device=dev)                    # the first step of the ladder always passes
    ops.probe_fold(W, invstd, Bf)
    ops.pca_project(X, mean, Bf, None, Z)
    ops.pca_project(X, mean, Bf, None, Zp)
    state_run = state.clone()

    def coeff():
        state_run.copy_(state)
        ops.lbfgs_coeff(dots, m, True, state_run)
    arms = {"project": lambda: ops.pca_project(X, mean, Bf, None, Zp),
            "backproject": lambda: ops.pca_backproject(R, X, mean, Zt),
            "fold (+ penalty products)": lambda: ops.probe_fold(P, invstd, Bf, W, pen),
            "residual": lambda: ops.probe_residual(Z, b, y, R, loss, gb, status),
            "linesearch (16 steps)": lambda: ops.probe_linesearch(Z, Zp, b, pb, y, one, 16, phi),
            "step": lambda: ops.probe_step(phi, one, f_big, pen, gtp, 1.0 / N, 1e-4, Z, Zp, theta, p, s_new, state_run),
            "gradient": lambda: ops.probe_gradient(Zt, invstd, theta, gb, N, 1.0 / N, g, g_prev, y_new),
            "lbfgs dots": lambda: ops.lbfgs_dots(S, Y, g, s_new, y_new, state, dots),
            "lbfgs coeff (+ state copy)": coeff,
            "lbfgs combine": lambda: ops.lbfgs_combine(S, Y, g, s_new, y_new, state, p)}
    times = {name: [] for name in arms}
    for r in range(repeats + 1):                                                         # the first round warms every arm up
        for name, fn in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if r:
                times[name].append(e0.elapsed_time(e1))
    say(f"## kernels: N {N}, D {D}, C {C}, memory {m}; ms per call (device events), {repeats} repeats after one warm-up round, "
        f"alternated")
    med = {name: _row(say, name, times[name]) for name in arms}
    floor = N * D * 4 / (HBM_TBS * 1e12) * 1e3
    for name in ("project", "backproject"):
        say(f"{name}: bound = X read once at {HBM_TBS} TB/s = {floor:.3f} ms -> {100 * floor / med[name]:.1f} % of that rate")
    passes = med["project"] + med["backproject"]
    rows = med["residual"] + med["linesearch (16 steps)"] + med["step"]
    lbfgs = med["lbfgs dots"] + med["lbfgs coeff (+ state copy)"] + med["lbfgs combine"]
    vec = med["fold (+ penalty products)"] + med["gradient"]
    total = passes + rows + lbfgs + vec
    say(f"one iteration, sum of the medians: {total:.3f} ms = the two X passes {passes:.3f} + residual, line search and step {rows:.3f} "
        f"+ fold and gradient {vec:.3f} + the three L-BFGS launches {lbfgs:.3f}")
    say(f"share of an iteration outside the two X passes: {100 * (total - passes) / total:.1f} %")
    wall, iters = [], []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for r in range(repeats + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            clf = LogisticRegression().fit(X, y)
            torch.cuda.synchronize()
            if r:
                wall.append((time.perf_counter() - t0) * 1e3)
                iters.append(clf.n_iter_)
    say(f"## end to end: LogisticRegression().fit(X [{N}, {D}], y) with C = {C} classes (tol 1e-4, max_iter 100); wall ms, {repeats} "
        f"repeats after one warm-up fit")
    w = _row(say, "fit", wall)
    say(f"that fit: {iters[0]} iterations ({'the same' if len(set(iters)) == 1 else 'NOT the same'} in every repeat), converged "
        f"{clf.converged_}, loss {clf.loss_:.6f}, max |gradient| {clf.grad_norm_:.2e}, training accuracy {clf.score(X, y):.4f}; "
        f"{w / max(iters[0], 1):.3f} ms per iteration, column statistics and the final evaluation included")


def sklearn_once(say):
    import numpy as np
    import torch
    from sklearn.linear_model import LogisticRegression
    from sklearn.pipeline import make_pipeline
    from sklearn.preprocessing import StandardScaler
    from vit_som_amd import LogisticRegression as Ours
    X, y = data(3000, 10)
    Xh, yh = X.cpu().numpy().astype(np.float64), y.cpu().numpy()
    t0 = time.perf_counter()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        pipe = make_pipeline(StandardScaler(), LogisticRegression(tol=1e-4, max_iter=100)).fit(Xh, yh)
    host = time.perf_counter() - t0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        Ours().fit(X, y)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        clf = Ours().fit(X, y)
        torch.cuda.synchronize()
    ours = time.perf_counter() - t0
    agree = float((clf.predict(X).cpu().numpy() == pipe.predict(Xh)).mean())
    say(f"## for scale: N 3000, D {D}, C 10, one call each, wall: sklearn's pipeline on the host ({os.cpu_count()} CPUs visible) "
        f"{host * 1e3:.1f} ms in {int(pipe[-1].n_iter_[0])} iterations; this fit {ours * 1e3:.1f} ms in {clf.n_iter_} iterations; "
        f"the two predict alike on {100 * agree:.2f} % of the training rows")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17_linear_probe.txt"))
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--rows", type=int, nargs="+", default=[10000, 50000])
    ap.add_argument("--classes", type=int, nargs="+", default=[10, 100])
    ap.add_argument("--no-sklearn", action="store_true")
    ap.add_argument("--tests-log", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("linear_probe_bench: no GPU; a timing taken anywhere else says nothing")
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    arch = getattr(torch.cuda.get_device_properties(0), "gcnArchName", "?").split(":")[0]
    say(f"# linear probe on one MI355X ({arch}; torch reports the device name {torch.cuda.get_device_name(0)!r}): "
        f"tools/linear_probe_bench.py --repeats {a.repeats}")
    for N in a.rows:
        for C in a.classes:
            kernels(N, C, a.repeats, say)
    if not a.no_sklearn:
        sklearn_once(say)
    say("## not measured: kernel times from a profiler trace (the figures above are device events around one call, launch "
        "overhead included); more than one GPU; C > 100; the fit under a launch tape; real latents (the rows are synthetic).")
    if a.tests_log:
        say("## the solver tests (tests/test_linear_probe_gpu.py::test_solver_reaches_the_optimum, tol 1e-5): the device's gap to "
            "scipy's fp64 optimum next to the float32 host emulation's")
        for line in open(a.tests_log):
            if "gap to the optimum" in line:
                say(line.strip().lstrip("."))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
