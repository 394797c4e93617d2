"""PCA on the MI355X: the kernels of csrc/pca.hip bit for bit on integer data, within the project's tolerance rule on float
data, the solver (vit_som_amd.PCA) against sklearn in fp64, the memory contract of every new entry, and what is built on
top: SOMLayer.init_prototypes, evaluate_latent_spectrum, visualize_pca_map, init_som_from_data and the driver's switches.

The rule (pca_ref.bound): a value is held to 4 x max(e32, 2^-23) against fp64, e32 being the float32 reference's error
against the same fp64 value, errors measured as the largest absolute error over the largest absolute fp64 value."""
import copy
import signal
import warnings

import numpy as np
import pytest
import torch

import memcheck as MC
import pca_ref as R
from helpers import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(257, 12288), (333, 1003), (130, 3), (5, 40)]
WIDTHS = [10, 32, 64, 65]
# every (shape, width) with l <= min(N, D), and the two small shapes at their own full width
EXACT_CASES = [(N, D, l) for N, D in SHAPES for l in WIDTHS if l <= min(N, D)] + [(130, 3, 3), (5, 40, 5)]
KERNEL_CASES = [(257, 12288, 10), (333, 1003, 65), (130, 3, 3), (5, 40, 5)]


@pytest.fixture(autouse=True)
def time_limit(request):
    """A limit of its own for every test here, as in test_silhouette_gpu.py."""
    limit = 300 if "driver" in request.node.name else 120

    def expired(signum, frame):
        raise TimeoutError(f"{request.node.name}: no result after {limit} s")
    old = signal.signal(signal.SIGALRM, expired)
    signal.alarm(limit)
    yield
    signal.alarm(0)
    signal.signal(signal.SIGALRM, old)


def _dev(a, dtype=np.float32):
    return torch.from_numpy(np.array(a, dtype=dtype)).to(DEV)           # a copy: the fixtures are read-only


def _host(t):
    return t.detach().cpu().numpy()


def _ints(shape, lo, hi, seed):
    return np.random.RandomState(seed).randint(lo, hi + 1, size=shape).astype(np.float64)


def _padded(X, pad, fill=float("nan")):
    """X on the device in rows of D + pad elements, the padding filled."""
    N, D = X.shape
    buf = torch.full((N, D + pad), fill, dtype=torch.float32, device=DEV)
    buf[:, :D] = _dev(X)
    return buf[:, :D]


def _rule(got, ref32, ref64, what):
    err, bound = R.rel_err(got, ref64), R.bound(ref32, ref64)
    print(f"{what}: error {err:.3e}, bound {bound:.3e} (e32 {R.rel_err(ref32, ref64):.3e})")
    assert err <= bound, what


def _float_case(N, D, seed=5):
    """A float fixture of that shape: rank min(12, N - 1, D) signal, noise, a large column mean."""
    return R.fixture(N, D, min(12, N - 1, D), 0.7, 1e-3 if min(N, D) > 5 else 0.0, seed)


# ------------------------------------------------------------------ exact: integers below 2^24
@pytest.mark.parametrize("N,D,l", EXACT_CASES)
def test_project_and_backproject_are_exact_on_integers(N, D, l):
    """Centring of tile elements outside the matrix would add -mean into the sums: caught here bit for bit."""
    from vit_som_amd import ops
    X, mean = _ints((N, D), -3, 3, 1), _ints((D,), -2, 2, 2)
    B, Yin = _ints((l, D), -2, 2, 3), _ints((N, l), -2, 2, 4)
    Xc = X - mean
    want_y, want_z = (Xc @ B.T).astype(np.int64), (Yin.T @ Xc).astype(np.int64)
    assert max(np.abs(want_y).max(), np.abs(want_z).max()) < 2 ** 24 and 5 * 2 * max(N, D) < 2 ** 24
    Xd, md, Bd, Yd = _dev(X), _dev(mean), _dev(B), _dev(Yin)
    Y = ops.pca_project(Xd, md, Bd, None, torch.empty(N, l, device=DEV))
    assert np.array_equal(_host(Y).astype(np.int64), want_y) and np.array_equal(_host(Y), want_y.astype(np.float32))
    Z = ops.pca_backproject(Yd, Xd, md, torch.empty(l, D, device=DEV))
    assert np.array_equal(_host(Z), want_z.astype(np.float32))
    # a row pitch of Y that is a multiple of four floats (what PCA.fit uses): the 16-byte path of the k-strided operand
    Yp = _padded(Yin, (-l) % 4 + 4)
    Z = ops.pca_backproject(Yp, Xd, md, torch.empty(l, D, device=DEV))
    assert np.array_equal(_host(Z), want_z.astype(np.float32))


@pytest.mark.parametrize("N,D,l", [(257, 12288, 10), (333, 1003, 65)])
def test_exact_with_a_padded_stride_and_without_a_mean(N, D, l):
    from vit_som_amd import ops
    X, mean = _ints((N, D), -3, 3, 6), _ints((D,), -2, 2, 7)
    B, Yin = _ints((l, D), -2, 2, 8), _ints((N, l), -2, 2, 9)
    Xp, md, Bd, Yd = _padded(X, 4), _dev(mean), _dev(B), _dev(Yin)             # ldx = D + 4, the padding columns NaN
    assert Xp.stride(0) == D + 4
    Y = ops.pca_project(Xp, md, Bd, None, torch.empty(N, l, device=DEV))
    assert np.array_equal(_host(Y), ((X - mean) @ B.T).astype(np.float32))
    Z = ops.pca_backproject(Yd, Xp, md, torch.empty(l, D, device=DEV))
    assert np.array_equal(_host(Z), (Yin.T @ (X - mean)).astype(np.float32))
    Y = ops.pca_project(_dev(X), None, Bd, None, torch.empty(N, l, device=DEV))
    assert np.array_equal(_host(Y), (X @ B.T).astype(np.float32))
    Z = ops.pca_backproject(Yd, _dev(X), None, torch.empty(l, D, device=DEV))
    assert np.array_equal(_host(Z), (Yin.T @ X).astype(np.float32))
    # an integer scale is exact too
    scale = _ints((l,), 1, 3, 10)
    Y = ops.pca_project(Xp, md, Bd, _dev(scale), torch.empty(N, l, device=DEV))
    assert np.array_equal(_host(Y), (((X - mean) @ B.T) * scale).astype(np.float32))


# ------------------------------------------------------------------ rule-bound, kernel by kernel
@pytest.mark.parametrize("N,D,l", KERNEL_CASES)
def test_kernels_within_the_rule(N, D, l):
    from vit_som_amd import ops
    rng = np.random.RandomState(11)
    X = _float_case(N, D)
    Xt, X64 = torch.from_numpy(X.copy()), X.astype(np.float64)
    Xd = _dev(X)

    mean, var = ops.pca_colstats(Xd)
    _rule(_host(mean), Xt.mean(dim=0).numpy(), X64.mean(axis=0), "colstats mean")
    mean64 = _host(mean).astype(np.float64)
    var64 = ((X64 - mean64) ** 2).sum(axis=0) / (N - 1)
    _rule(_host(var), ((Xt - mean.cpu()) ** 2).sum(dim=0).numpy() / np.float32(N - 1), var64, "colstats var")

    B = rng.standard_normal((l, D)).astype(np.float32) / np.float32(np.sqrt(D))
    scale = rng.uniform(0.5, 2.0, l).astype(np.float32)
    Bt, Bd, sd = torch.from_numpy(B), _dev(B), _dev(scale)
    Xc32, Xc64 = Xt - mean.cpu(), X64 - mean64
    ref64 = Xc64 @ B.astype(np.float64).T
    Y = ops.pca_project(Xd, mean, Bd, None, torch.empty(N, l, device=DEV))
    _rule(_host(Y), (Xc32 @ Bt.T).numpy(), ref64, "project")
    Ys = ops.pca_project(Xd, mean, Bd, sd, torch.empty(N, l, device=DEV))
    _rule(_host(Ys), ((Xc32 @ Bt.T) * torch.from_numpy(scale)).numpy(), ref64 * scale.astype(np.float64), "project with scale")

    Yin = rng.standard_normal((N, l)).astype(np.float32)
    Z = ops.pca_backproject(_dev(Yin), Xd, mean, torch.empty(l, D, device=DEV))
    _rule(_host(Z), (torch.from_numpy(Yin).T @ Xc32).numpy(), Yin.astype(np.float64).T @ Xc64, "backproject")

    G = torch.empty(l, l, dtype=torch.float64, device=DEV)
    H = torch.empty(l, l, dtype=torch.float64, device=DEV)
    ops.pca_gram(Z, G, Bd, H)
    Z64, B64 = _host(Z).astype(np.float64), B.astype(np.float64)
    assert R.rel_err(_host(G), Z64 @ Z64.T) <= 1e-12 and R.rel_err(_host(H), B64 @ Z64.T) <= 1e-12
    assert torch.equal(G, G.T.contiguous())
    G1 = torch.empty(l, l, dtype=torch.float64, device=DEV)
    ops.pca_gram(Z, G1)
    assert torch.equal(G1, G)

    T = rng.standard_normal((max(l - 1, 1), l))
    out = ops.pca_rotate(_dev(T, np.float64), Z, torch.empty(T.shape[0], D, device=DEV))
    _rule(_host(out), (torch.from_numpy(T.astype(np.float32)) @ Z.cpu()).numpy(), T @ Z64, "rotate")
    with pytest.raises(Exception, match="overlaps"):
        ops.pca_rotate(_dev(T, np.float64), Z, Z[:T.shape[0]])

    M = 7
    Ym = rng.standard_normal((M, l)).astype(np.float32)
    rec = ops.pca_reconstruct(_dev(Ym), sd, Bd, mean, torch.empty(M, D, device=DEV))
    ref64 = (Ym.astype(np.float64) * scale.astype(np.float64)) @ B64 + mean64
    ref32 = ((torch.from_numpy(Ym) * torch.from_numpy(scale)) @ Bt + mean.cpu()).numpy()
    _rule(_host(rec), ref32, ref64, "reconstruct")
    rec0 = ops.pca_reconstruct(_dev(Ym), None, Bd, None, torch.empty(M, D, device=DEV))
    _rule(_host(rec0), (torch.from_numpy(Ym) @ Bt).numpy(), Ym.astype(np.float64) @ B64, "reconstruct, no scale, no mean")


# ------------------------------------------------------------------ the solver against sklearn in fp64
def _fit(fx, **kw):
    from vit_som_amd import PCA
    N, D, r, ratio, noise, k = fx
    X = _dev(R.fixture(N, D, r, ratio, noise))
    with warnings.catch_warnings():
        warnings.simplefilter("error")                  # no residual above tol, no dropped direction
        return PCA(n_components=k, **kw).fit(X), X


def _signs(C, C64):
    s = np.sign(np.sum(np.asarray(C, np.float64) * C64, axis=1))
    s[s == 0] = 1
    return s


@pytest.mark.parametrize("fx", R.SOLVER_FIXTURES, ids=lambda f: f"{f[0]}x{f[1]}k{f[5]}")
def test_solver_against_sklearn_fp64(fx):
    N, D, r, ratio, noise, k = fx
    p, X = _fit(fx)
    sk32, sk64 = R.sklearn_pair(*fx)
    Xh = R.fixture(N, D, r, ratio, noise)
    C, C64 = _host(p.components_), sk64.components_
    assert C.shape == (k, D) and p.basis_width_ == min(k + 8, N, D) and p.n_iter_ == 10
    assert (p.n_samples_, p.n_features_in_) == (N, D)
    _rule(_host(p.explained_variance_), sk32.explained_variance_, sk64.explained_variance_, "explained_variance_ (relative to lambda_1)")
    _rule(_host(p.explained_variance_ratio_), sk32.explained_variance_ratio_, sk64.explained_variance_ratio_, "explained_variance_ratio_")
    _rule(_host(p.mean_), sk32.mean_, sk64.mean_, "mean_")
    cos, cos32 = R.one_minus_cos(C, C64), R.one_minus_cos(sk32.components_, C64)
    print(f"1 - |cos|: {cos:.3e}, bound {4 * max(cos32, R.EPS32):.3e} (sklearn float32 {cos32:.3e})")
    assert cos <= 4 * max(cos32, R.EPS32)
    orth, orth32 = R.ortho_err(C), R.ortho_err(sk32.components_)
    print(f"max |W W^T - I|: {orth:.3e}, bound {4 * max(orth32, R.EPS32):.3e}")
    assert orth <= 4 * max(orth32, R.EPS32)
    Y64 = sk64.transform(Xh.astype(np.float64))
    Y32 = sk32.transform(Xh) * _signs(sk32.components_, C64)
    _rule(_host(p.transform(X)) * _signs(C, C64), Y32, Y64, "transform (up to each component's sign)")
    res = _host(p.residuals_)
    print(f"residuals: max {res.max():.3e}")
    assert res.shape == (k,) and float(res.max()) <= 1e-3
    assert abs(p.noise_variance_ - sk64.noise_variance_) <= 4 * max(abs(float(sk32.noise_variance_) - sk64.noise_variance_), R.EPS32 * sk64.explained_variance_[0])
    big = np.argmax(np.abs(C), axis=1)
    assert (C[np.arange(k), big] > 0).all(), "sign rule: the entry of largest magnitude is positive"


def test_wide_basis_one_past_a_tile():
    fx = R.WIDE_FIXTURE
    N, D, r, ratio, noise, k = fx
    p, X = _fit(fx)
    sk32, sk64 = R.sklearn_pair(*fx)
    assert p.basis_width_ == 65 and p.components_.shape == (57, D)
    _rule(_host(p.explained_variance_), sk32.explained_variance_, sk64.explained_variance_, "explained_variance_ (relative to lambda_1)")
    C = _host(p.components_)
    assert R.ortho_err(C) <= 4 * max(R.ortho_err(sk32.components_), R.EPS32)
    big = np.argmax(np.abs(C), axis=1)
    assert (C[np.arange(k), big] > 0).all()
    # the kernels, not the conditioning of the 57th direction: against the fp64 products of the fitted components
    Xh, mean = R.fixture(N, D, r, ratio, noise), _host(p.mean_)
    Xc64, C64 = Xh.astype(np.float64) - mean.astype(np.float64), C.astype(np.float64)
    Y = p.transform(X)
    _rule(_host(Y), ((torch.from_numpy(Xh.copy()) - torch.from_numpy(mean)) @ torch.from_numpy(C).T).numpy(), Xc64 @ C64.T, "transform")
    Yh = _host(Y)
    back64 = Yh.astype(np.float64) @ C64 + mean.astype(np.float64)
    back32 = (torch.from_numpy(Yh) @ torch.from_numpy(C) + torch.from_numpy(mean)).numpy()
    _rule(_host(p.inverse_transform(Y)), back32, back64, "inverse_transform")


def test_rank_deficient_set():
    fx = R.RANK_FIXTURE
    N, D, r, ratio, noise, k = fx
    from vit_som_amd import PCA
    X = _dev(R.fixture(N, D, r, ratio, noise))
    p = PCA(n_components=k).fit(X)
    sk32, sk64 = R.sklearn_pair(*fx)
    C, ev = _host(p.components_), _host(p.explained_variance_)
    lam1 = sk64.explained_variance_[0]
    _rule(ev[:4], sk32.explained_variance_[:4], sk64.explained_variance_[:4], "explained_variance_[:4]")
    cos = R.one_minus_cos(C[:4], sk64.components_[:4])
    assert cos <= 4 * max(R.one_minus_cos(sk32.components_[:4], sk64.components_[:4]), R.EPS32)
    assert 0.0 <= ev[4] <= R.EPS32 * lam1
    assert np.isfinite(C).all() and C.shape == (5, D)
    assert R.ortho_err(C) <= 4 * max(R.ortho_err(sk32.components_), R.EPS32)


@pytest.mark.parametrize("whiten", [False, True])
def test_round_trip(whiten):
    fx = R.SOLVER_FIXTURES[1]
    N, D, r, ratio, noise, k = fx
    p, X = _fit(fx, whiten=whiten)
    Xh, mean, C = R.fixture(N, D, r, ratio, noise), _host(p.mean_), _host(p.components_)
    Y = p.transform(X)
    back = _host(p.inverse_transform(Y))
    Xc64, C64, mean64 = Xh.astype(np.float64) - mean.astype(np.float64), C.astype(np.float64), mean.astype(np.float64)
    Xc32, C32 = torch.from_numpy(Xh.copy()) - torch.from_numpy(mean), torch.from_numpy(C)
    _rule(back, ((Xc32 @ C32.T) @ C32 + torch.from_numpy(mean)).numpy(), (Xc64 @ C64.T) @ C64 + mean64, "round trip")
    if whiten:
        sd64 = np.sqrt(_host(p.explained_variance_))
        want64 = (Xc64 @ C64.T) / sd64
        _rule(_host(Y), ((Xc32 @ C32.T) / torch.from_numpy(sd64.astype(np.float32))).numpy(), want64, "whitened transform")
        var = _host(Y).astype(np.float64).var(axis=0, ddof=1)
        ref32 = ((Xc32 @ C32.T) / torch.from_numpy(sd64.astype(np.float32))).numpy().astype(np.float64).var(axis=0, ddof=1)
        _rule(var, ref32, np.ones(k), "unit sample variance per component")


def test_fit_is_reproducible_and_the_seed_only_moves_bits():
    fx = R.SOLVER_FIXTURES[3]
    a, _ = _fit(fx)
    b, _ = _fit(fx)
    for name in ("components_", "mean_", "explained_variance_", "explained_variance_ratio_", "singular_values_", "residuals_"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert a.noise_variance_ == b.noise_variance_ and a.basis_width_ == b.basis_width_
    c, _ = _fit(fx, random_state=1)
    assert not torch.equal(a.components_, c.components_)
    sk32, sk64 = R.sklearn_pair(*fx)
    _rule(_host(c.explained_variance_), sk32.explained_variance_, sk64.explained_variance_, "explained_variance_, another seed")
    cos = R.one_minus_cos(_host(c.components_), sk64.components_)
    assert cos <= 4 * max(R.one_minus_cos(sk32.components_, sk64.components_), R.EPS32)


def test_transform_of_one_row_and_argument_errors():
    p, X = _fit(R.SOLVER_FIXTURES[2])
    assert torch.equal(p.transform(X[:1]), p.transform(X)[:1])      # D = 3: one k-tile, one split, whatever the row count
    with pytest.raises(ValueError, match="features"):
        p.transform(torch.zeros(4, 5, device=DEV))
    with pytest.raises(ValueError, match="float32"):
        p.transform(X.double())


# ------------------------------------------------------------------ the memory contract of every new entry
def _bits(t):
    t = t.contiguous()
    return t.view({4: torch.int32, 8: torch.int64}[t.element_size()])


@pytest.mark.parametrize("fill", MC.FILLS)
@pytest.mark.parametrize("entry", ["colstats", "project", "backproject", "gram", "rotate", "reconstruct"])
def test_memory_contract(monkeypatch, entry, fill):
    """(257, 1003, l = 10): outputs in guard-banded poisoned buffers, slabs / partials of exactly the queried size and
    pre-filled with the poison, X in rows of D + 8 whose padding is poisoned.  Guards intact, every output element written,
    the result bit for bit that of the plain run."""
    from vit_som_amd import ops
    N, D, l, PAD = 257, 1003, 10, 8
    rng = np.random.RandomState(17)
    X = torch.from_numpy(_float_case(N, D).copy())
    mean = X.mean(dim=0)
    B = torch.from_numpy(rng.standard_normal((l, D)).astype(np.float32))
    Yin = torch.from_numpy(rng.standard_normal((N, l)).astype(np.float32))
    scale = torch.from_numpy(rng.uniform(0.5, 2.0, l).astype(np.float32))
    T = torch.from_numpy(rng.standard_normal((7, l)))
    f32, f64 = torch.float32, torch.float64

    def run(x, b, y, outs):
        m, s = mean.to(DEV), scale.to(DEV)
        if entry == "colstats":
            ops.pca_colstats(x, outs["mean"], outs["var"])
        elif entry == "project":
            ops.pca_project(x, m, b, s, outs["Y"])
        elif entry == "backproject":
            ops.pca_backproject(y, x, m, outs["Zt"])
        elif entry == "gram":
            ops.pca_gram(x[:l], outs["G"], b, outs["H"])
        elif entry == "rotate":
            ops.pca_rotate(T.to(DEV), x[:l], outs["Bout"])
        else:
            ops.pca_reconstruct(y[:9], s, b, m, outs["Xout"])

    shapes = {"colstats": {"mean": ((D,), f32, None), "var": ((D,), f64, None)},
              "project": {"Y": ((N, l), f32, l + 2)}, "backproject": {"Zt": ((l, D), f32, D + PAD)},
              "gram": {"G": ((l, l), f64, None), "H": ((l, l), f64, None)}, "rotate": {"Bout": ((7, D), f32, D + PAD)},
              "reconstruct": {"Xout": ((9, D), f32, D + PAD)}}[entry]
    plain = {k: torch.empty(shape, dtype=dt, device=DEV) for k, (shape, dt, _) in shapes.items()}
    run(X.to(DEV), B.to(DEV), Yin.to(DEV), plain)
    torch.cuda.synchronize()

    es = MC.ExactScratch(fill)
    handles, outs = {}, {}
    x, handles["X"] = MC.guarded_copy(X.to(DEV), ld=D + PAD)
    b, handles["B"] = MC.guarded_copy(B.to(DEV), ld=D + PAD)
    y, handles["Yin"] = MC.guarded_copy(Yin.to(DEV), ld=l + 2)
    for k, (shape, dt, ld) in shapes.items():
        outs[k], handles[k] = MC.guarded(shape, dt, DEV, ld=ld)
    with monkeypatch.context() as mp:
        mp.setattr(ops, "scratch", es)
        run(x, b, y, outs)
    torch.cuda.synchronize()
    assert (es.calls > 0) == (entry in ("colstats", "project", "backproject"))
    if es.calls:
        need = {"colstats": 8 * ops.lib.vsom_pca_colstats_parts(N, D), "project": 4 * ops.pca_slabs(N, D, l, 0),
                "backproject": 4 * ops.pca_slabs(N, D, l, 1)}[entry]
        assert [key[2] for key in es.arenas] == [need]
    es.check()
    for name, h in handles.items():
        h.check(f"[{fill}] {name}")
    assert torch.equal(x, X.to(DEV)) and torch.equal(b, B.to(DEV)) and torch.equal(y, Yin.to(DEV))
    for k in shapes:
        handles[k].all_written(f"[{fill}] {k}")
        assert torch.equal(_bits(outs[k]), _bits(plain[k])), f"[{fill}] {k} differs from the plain run"


# ------------------------------------------------------------------ SOM initialisation
def _tiny_model(topology, distance):
    import vit_som_amd
    _, cfg = load_golden("ref_cluster_tiny")
    cfg = copy.deepcopy(cfg)
    cfg["hyperparameters"]["som"].update(topology=topology, distance_fcn=distance, map_size=[4, 3] if topology == "hexa" else [3, 5])
    return vit_som_amd.ViTSOM(cfg, device=DEV), cfg


@pytest.mark.parametrize("topology,distance", [("square", "euclidean"), ("hexa", "euclidean"), ("square", "cosine")])
def test_init_prototypes_pca(topology, distance):
    m, cfg = _tiny_model(topology, distance)
    som = m.som_layer
    K, D = som.prototypes.shape
    Xh = R.fixture(200, D, 6, 0.7, 1e-3, seed=3)
    before, stamp = som.prototypes.data_ptr(), som._w_stamp()
    param = som.prototypes
    p = som.init_prototypes(_dev(Xh), method="pca", span=2.0)
    assert som.prototypes is param and som.prototypes.data_ptr() == before and som._w_stamp() != stamp
    assert som.prototypes.requires_grad and som._wplanes_stamp is None
    uv = som.pca_grid_coordinates().numpy()
    assert uv.min() == -1.0 and uv.max() == 1.0
    sd = np.sqrt(_host(p.explained_variance_))
    C64, mean64 = _host(p.components_).astype(np.float64), _host(p.mean_).astype(np.float64)
    want64 = mean64 + 2.0 * ((uv * sd) @ C64)
    want32 = (torch.from_numpy(_host(p.mean_)) + (torch.from_numpy((2.0 * uv).astype(np.float32)) * torch.from_numpy(sd.astype(np.float32)))
              @ torch.from_numpy(_host(p.components_))).numpy()
    W = _host(som.prototypes)
    if distance == "cosine":
        assert np.abs(np.linalg.norm(W.astype(np.float64), axis=1) - 1.0).max() <= 4 * R.EPS32
        want64 = want64 / np.linalg.norm(want64, axis=1, keepdims=True)
        want32 = torch.nn.functional.normalize(torch.from_numpy(want32), p=2, dim=1).numpy()
    _rule(W, want32, want64, f"prototypes after the linear initialisation ({topology}, {distance})")
    # the map lies in the data now: no prototype is farther from the mean than the spread of the plane allows
    if distance != "cosine":
        assert np.linalg.norm(W - mean64, axis=1).max() <= 2.0 * np.sqrt(2.0) * sd[0] * (1 + 1e-5)


def test_init_prototypes_sample():
    m, cfg = _tiny_model("square", "euclidean")
    som = m.som_layer
    K, D = som.prototypes.shape
    Xh = R.fixture(200, D, 6, 0.7, 1e-3, seed=3)
    assert som.init_prototypes(_dev(Xh), method="sample", seed=4) is None
    idx = np.random.RandomState(4).choice(200, K, replace=False)
    assert np.array_equal(_host(som.prototypes), Xh[idx])
    few = Xh[:7]
    som.init_prototypes(_dev(few), method="sample", seed=4)
    assert np.array_equal(_host(som.prototypes), few[np.random.RandomState(4).choice(7, K, replace=True)])


# ------------------------------------------------------------------ evaluation and the driver
def test_latent_spectrum_pca_map_and_init_from_data(tmp_path):
    from test_knn_gpu import _loaders, _model
    from vit_som_amd import LatentSpectrum, PCA, evaluate_latent_spectrum, init_som_from_data, visualize_pca_map
    from vit_som_amd.evaluation import _som_latents, components_for, effective_rank
    m, cfg = _model("ref_cluster_tiny")
    train, _ = _loaders(cfg, 4)                                    # 96 samples in batches of 10
    X, _ = _som_latents(m, cfg, train, "test")
    rep = evaluate_latent_spectrum(m, cfg, train, n_components=16)
    want = PCA(n_components=16).fit(X)
    assert isinstance(rep, LatentSpectrum) and rep.n_samples == 96 and rep.explained_variance.shape == (16,)
    assert np.array_equal(rep.explained_variance, _host(want.explained_variance_))
    assert np.array_equal(rep.cumulative_ratio, np.cumsum(_host(want.explained_variance_ratio_)))
    assert rep.total_variance == want.total_variance_ and 0 < rep.cumulative_ratio[-1] <= 1 + 1e-6
    assert rep.components_for == components_for(rep.cumulative_ratio) and set(rep.components_for) == {0.5, 0.9, 0.95, 0.99}
    assert rep.effective_rank == effective_rank(rep.explained_variance) and 1.0 <= rep.effective_rank <= 16.0
    assert (np.diff(rep.explained_variance) <= 0).all() and rep.residuals.shape == (16,)

    proj, labels, protos, ratio = visualize_pca_map(m, cfg, train, epoch=3, output_dir=str(tmp_path))
    K = m.som_layer.n_prototypes
    assert proj.shape == (96, 2) and labels.shape == (96,) and protos.shape == (K, 2) and ratio.shape == (2,)
    assert np.isfinite(proj).all() and np.isfinite(protos).all() and ratio[0] >= ratio[1] > 0
    try:
        import matplotlib  # noqa: F401
        assert (tmp_path / "som_pca_map_epoch_3.png").exists()
    except ImportError:
        pass

    was_training, before = m.training, m.som_layer.prototypes.detach().clone()
    fitted = init_som_from_data(m, cfg, train, method="pca")
    assert m.training == was_training and not torch.equal(before, m.som_layer.prototypes)
    W = _host(m.som_layer.prototypes).astype(np.float64)
    if m.som_layer.distance_fcn == "cosine":
        assert np.abs(np.linalg.norm(W, axis=1) - 1).max() <= 4 * R.EPS32
    assert fitted.n_samples_ == 96
    init_som_from_data(m, cfg, train, method="sample", max_rows=50)
    rows = _host(X)[:50]
    if m.som_layer.distance_fcn == "cosine":
        rows = torch.nn.functional.normalize(torch.from_numpy(rows), p=2, dim=1).numpy()
    Wn = _host(m.som_layer.prototypes)
    assert all((np.abs(rows - w).max(axis=1) <= 1e-6).any() for w in Wn)


def test_driver_som_init_and_latent_spectrum(tmp_path):
    from vit_som_amd.train import main, synthetic_loaders
    _, cfg = load_golden("ref_cluster_tiny")
    cfg = copy.deepcopy(cfg)
    cfg["hyperparameters"]["batch_size"] = 16
    loaders = lambda c, r, w: synthetic_loaders(c, r, w, n_train=64, n_val=16, n_test=16)      # noqa: E731
    today = {"accuracy", "precision", "recall", "f1", "purity", "nmi", "run_duration", "inference_time"}
    logs = []
    met = main(cfg, n_runs=1, max_epochs=1, make_loaders=loaders, model_states_dir=str(tmp_path / "a"), log=logs.append,
               som_init="pca", latent_spectrum=True)
    assert set(met) == today | {"effective_rank", "components_90"}
    (er,), (c90,) = met["effective_rank"], met["components_90"]
    assert 1.0 <= er <= 64.0 and (np.isnan(c90) or 1 <= c90 <= 64)
    print([line for line in logs if "spectrum" in line or "initialised" in line])
    assert any("SOM initialised" in line for line in logs) and any("effective_rank" in line for line in logs)
    with pytest.raises(ValueError, match="som_init"):
        main(cfg, n_runs=1, max_epochs=1, make_loaders=loaders, model_states_dir=str(tmp_path / "c"), log=logs.append, som_init="kmeans")
