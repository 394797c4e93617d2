"""On-device spectral embedding (csrc/spectral.hip, vit_som_amd/spectral.py) at the smallest shapes at which the kernels can
still go wrong -- every kernel against the fp64 restatement with a bound derived from the sums themselves, bitwise
reproducibility and independence of the launch geometry -- and whole fits against dense eigh and sklearn.  Every condition
a fit is held to is shown in test_spectral_cpu.py to hold for the reference alone.  Nothing is larger than 3000 rows."""
import signal
import warnings

import numpy as np
import pytest
import scipy.sparse
import scipy.sparse.csgraph
import torch

import spectral_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-8
U52 = 2.0 ** -52


@pytest.fixture(autouse=True)
def time_limit(request):
    """A limit of its own for every test here, as in test_dbscan_gpu.py."""
    def expired(signum, frame):
        raise TimeoutError(f"{request.node.name}: no result after 120 s")
    old = signal.signal(signal.SIGALRM, expired)
    signal.alarm(120)
    yield
    signal.alarm(0)
    signal.signal(signal.SIGALRM, old)


def _dev(a, dtype=np.float64):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def _csr(A):
    return _dev(A.indptr, np.int64), _dev(A.indices, np.int64), _dev(A.data, np.float64)


def _degrees(A):
    """ops.spectral_degrees on a scipy CSR (indices as they stand) -> (triple, d, s, heavy, status list)."""
    from vit_som_amd import ops
    N = A.shape[0]
    tri = _csr(A)
    d, s = torch.empty(N, dtype=torch.float64, device=DEV), torch.empty(N, dtype=torch.float64, device=DEV)
    heavy, status = torch.empty(N, dtype=torch.int32, device=DEV), torch.empty(ops.SPECTRAL_STATUS, dtype=torch.int64, device=DEV)
    ops.spectral_degrees(*tri, d, s, heavy, status)
    return tri, d, s, heavy, status.tolist()


# ------------------------------------------------------------------ (a) the product
def _odd_matrix(N=257, seed=0):
    """Rows of 0..12 entries, rows 0, 100 and 256 empty, row 7 with a diagonal entry, row 5 with 1500 entries (columns
    repeat): not symmetric, which the product does not need."""
    rs = np.random.RandomState(seed)
    rows, cols, vals = [], [], []
    for i in range(N):
        n = 1500 if i == 5 else (0 if i in (0, 100, N - 1) else rs.randint(1, 13))
        c = np.sort(rs.randint(0, N, size=n))
        if i == 7:
            c[0] = 7
            c = np.sort(c)
        rows.append(np.full(n, i)), cols.append(c), vals.append(rs.uniform(0.1, 2.0, size=n))
    indptr = np.concatenate([[0], np.cumsum([len(c) for c in cols])])
    A = scipy.sparse.csr_matrix((np.concatenate(vals), np.concatenate(cols), indptr), shape=(N, N))
    return A


@pytest.mark.parametrize("l", [1, 3, 16, 32])
def test_spmm_against_the_restatement(l):
    from vit_som_amd import ops
    A = _odd_matrix()
    N = A.shape[0]
    tri, d, s, heavy, st = _degrees(A)
    assert st[ops.SPECTRAL_HEAVY] == 1 and int(heavy[0]) == 5 and st[ops.SPECTRAL_BAD_INDEX] == st[ops.SPECTRAL_BAD_WEIGHT] == 0
    d_ref, s_ref = R.degrees(A)
    assert np.array_equal(d.cpu().numpy(), d_ref) and (np.abs(s.cpu().numpy() - s_ref) <= 2 * U52 * s_ref).all()      # sqrt, division
    s_ref = s.cpu().numpy()                                         # the restatement weighs with the very s the kernel reads
    assert st[ops.SPECTRAL_ISOLATED] == int((d_ref == 0).sum()) >= 3
    rs = np.random.RandomState(l)
    Y1, Y0 = rs.standard_normal((N, l)), rs.standard_normal((N, l))
    for (y0, alpha, c, beta) in ((None, 1.0, 0.0, 0.0), (Y0, 1.7, -0.4, 0.83)):
        want, bound = R.spmm(A, s_ref, Y1, y0, alpha, c, beta)
        new = lambda: torch.full((N, l), float("nan"), dtype=torch.float64, device=DEV)      # noqa: E731
        y0d = _dev(y0) if y0 is not None else None
        a = ops.spectral_spmm(*tri, s, _dev(Y1), y0d, new(), alpha, c, beta, heavy, 1)
        got = a.cpu().numpy()
        worst = np.abs(got - want) / np.maximum(bound, 1e-300)
        print(f"l {l}: max error / bound {worst.max():.3f}, long row {np.abs(got[5] - want[5]).max():.2e} of bound {bound[5].max():.2e}")
        assert np.isfinite(got).all() and (np.abs(got - want) <= bound).all()
        # twice the same bits; the same bits without the list of long rows; the same bits at a padded row stride
        b = ops.spectral_spmm(*tri, s, _dev(Y1), y0d, new(), alpha, c, beta, heavy, 1)
        assert torch.equal(a, b)
        inline = ops.spectral_spmm(*tri, s, _dev(Y1), y0d, new(), alpha, c, beta)
        assert torch.equal(a, inline)
        def pad(t):
            if t is None:
                return None
            wide = torch.full((N, 40), float("nan"), dtype=torch.float64, device=DEV)
            wide[:, :l] = _dev(t)
            return wide[:, :l]
        outp = torch.full((N, 40), float("nan"), dtype=torch.float64, device=DEV)
        padded = ops.spectral_spmm(*tri, s, pad(Y1), pad(y0), outp[:, :l], alpha, c, beta, heavy, 1)
        assert torch.equal(a, padded.contiguous()) and bool(torch.isnan(outp[:, l:]).all())


def test_spmm_wrapper_refusals():
    from vit_som_amd import ops
    A = _odd_matrix()
    tri, d, s, heavy, _ = _degrees(A)
    Y = torch.zeros(257, 4, dtype=torch.float64, device=DEV)
    with pytest.raises(Exception, match="overlaps"):
        ops.spectral_spmm(*tri, s, Y, None, Y)
    with pytest.raises(ValueError, match="row stride"):
        ops.spectral_spmm(*tri, s, Y, None, torch.zeros(257, 8, dtype=torch.float64, device=DEV)[:, :4])
    with pytest.raises(ValueError, match="float64"):
        ops.spectral_spmm(*tri, s, Y.float(), None, torch.zeros_like(Y))
    with pytest.raises(ValueError, match="Y1"):
        ops.spectral_spmm(*tri, s, torch.zeros(257, 33, dtype=torch.float64, device=DEV)[:200], None, torch.zeros_like(Y))


# ------------------------------------------------------------------ (b) Gram matrices, residuals, the rotation
def _long(a):
    return np.asarray(a, np.longdouble)


@pytest.mark.parametrize("N", [1, 63, 64, 65, 1025])
def test_gram_and_residual_against_numpy(N):
    """The reference sums in extended precision, so the bound is the kernel's own: a chain of N fma and the slab additions,
    (N + 4) 2^-52 sum |terms| (gamma_n with u = 2^-53, doubled).  Slab counts 1, 2 and 4: at N = 65 two slabs are one slab
    and one row."""
    from vit_som_amd import ops
    l = 7
    rs = np.random.RandomState(N)
    V, W, theta = rs.standard_normal((N, l)), rs.standard_normal((N, l)), rs.uniform(0.5, 1.0, l)
    Vd, Wd, td = _dev(V), _dev(W), _dev(theta)
    G_ref = np.asarray(_long(V).T @ _long(V), np.float64)
    H_ref = np.asarray(_long(V).T @ _long(W), np.float64)
    Gb = (N + 4) * U52 * (np.abs(V).T @ np.abs(V))
    Hb = (N + 4) * U52 * (np.abs(V).T @ np.abs(W))
    E = _long(W) - _long(theta) * _long(V)
    r_ref = np.asarray((E * E).sum(0), np.float64)
    rb = (N + 6) * U52 * r_ref                                      # a difference is one fma: one rounding, relative to itself
    seen = {}
    for slabs in (1, 2, 4):
        G, H = torch.empty(l, l, dtype=torch.float64, device=DEV), torch.empty(l, l, dtype=torch.float64, device=DEV)
        ops.spectral_gram(Vd, Wd, G, H, slabs)
        G1 = torch.empty_like(G)
        ops.spectral_gram(Vd, None, G1, None, slabs)
        res = ops.spectral_residual(Vd, Wd, td, torch.empty(l, dtype=torch.float64, device=DEV), slabs)
        g, h, r = G.cpu().numpy(), H.cpu().numpy(), res.cpu().numpy()
        print(f"N {N}, {slabs} slabs: G {np.abs(g - G_ref).max():.2e} (bound {Gb.max():.2e}), H {np.abs(h - H_ref).max():.2e}, "
              f"residual {np.abs(r - r_ref).max():.2e} (bound {rb.max():.2e})")
        assert (np.abs(g - G_ref) <= Gb).all() and (np.abs(h - H_ref) <= Hb).all() and (np.abs(r - r_ref) <= rb).all()
        assert np.array_equal(g, g.T) and torch.equal(G, G1)
        G2, H2 = torch.empty_like(G), torch.empty_like(H)             # the same slab count: the same bits
        ops.spectral_gram(Vd, Wd, G2, H2, slabs)
        assert torch.equal(G, G2) and torch.equal(H, H2)
        assert torch.equal(res, ops.spectral_residual(Vd, Wd, td, torch.empty(l, dtype=torch.float64, device=DEV), slabs))
        seen[slabs] = (g, h, r)
    for a, b in ((1, 2), (1, 4), (2, 4)):                             # different slab counts: each within its bound
        assert (np.abs(seen[a][0] - seen[b][0]) <= 2 * Gb).all() and (np.abs(seen[a][2] - seen[b][2]) <= 2 * rb).all()
    # a padded row stride and the rotation
    pad = torch.full((N, 12), float("nan"), dtype=torch.float64, device=DEV)
    pad[:, :l] = Vd
    Gp = torch.empty(l, l, dtype=torch.float64, device=DEV)
    ops.spectral_gram(pad[:, :l], None, Gp, None, 2)
    assert np.array_equal(Gp.cpu().numpy(), seen[2][0])
    T = rs.standard_normal((l, 5))
    out = torch.full((N, 9), float("nan"), dtype=torch.float64, device=DEV)
    ops.spectral_rotate(pad[:, :l], _dev(T), out[:, :5])
    want = np.asarray(_long(V) @ _long(T), np.float64)
    assert (np.abs(out[:, :5].cpu().numpy() - want) <= (l + 2) * U52 * (np.abs(V) @ np.abs(T))).all()
    assert bool(torch.isnan(out[:, 5:]).all())


def test_residual_is_computed_from_the_differences():
    """W = theta V + 1e-12 noise: from Gram entries the squared residual would drown at 1e-16 |W|^2."""
    from vit_som_amd import ops
    rs = np.random.RandomState(3)
    N, l = 700, 4
    V = np.linalg.qr(rs.standard_normal((N, l)))[0]
    theta = np.array([1.0, 0.99, 0.98, 0.5])
    noise = 1e-12 * rs.standard_normal((N, l))
    W = V * theta + noise
    from fractions import Fraction as F
    want = np.array([float(sum((F(float(W[i, j])) - F(float(theta[j])) * F(float(V[i, j]))) ** 2 for i in range(N))) for j in range(l)])
    got = ops.spectral_residual(_dev(V), _dev(W), _dev(theta), torch.empty(l, dtype=torch.float64, device=DEV)).cpu().numpy()
    assert (want > 1e-22).all() and (want < 1e-20).all()
    # fma(-theta, v, w) is the exact difference rounded once, so the sum is good to its own (N + 6) 2^-52
    print("residual from differences: relative error", (np.abs(got - want) / want).max())
    assert (np.abs(got - want) <= (N + 6) * U52 * want).all()


# ------------------------------------------------------------------ (c) the embedding's sign, the degrees' refusals
def test_embed_sign_rule_ties_and_isolated_rows():
    from vit_som_amd import ops
    N = 300
    rs = np.random.RandomState(0)
    V = rs.uniform(-1, 1, size=(N, 5))
    s = rs.uniform(0.5, 1.0, size=N)
    s[[3, 7, 10, 299]] = 1.0
    s[[20, 21]] = 0.0                                               # isolated rows
    V[3, 1], V[7, 1] = -2.5, 2.5                                    # a tie: the smaller row decides, negative
    V[10, 2], V[299, 2] = 3.0, -3.0                                 # a tie across the workgroup's threads, positive
    V[20, 3] = -50.0                                                # an isolated row never decides
    V[150, 3] = -4.0
    first, n = 1, 3
    E = torch.full((N, 4), float("nan"), dtype=torch.float32, device=DEV)
    sign = torch.empty(n, dtype=torch.float64, device=DEV)
    ops.spectral_embed(_dev(V), _dev(s), first, E[:, :n], sign)
    U = s[:, None] * V[:, first:first + n]
    want, sg = R.sign_flip(U)
    assert sg.tolist() == [-1.0, 1.0, -1.0] and sign.cpu().numpy().tolist() == sg.tolist()
    got = E[:, :n].cpu().numpy()
    assert np.array_equal(got, want.astype(np.float32)) and (got[[20, 21]] == 0).all() and bool(torch.isnan(E[:, n:]).all())


def test_degrees_refusals():
    from vit_som_amd import ops
    from vit_som_amd.spectral import DeviceGraph
    A = R.fixture("circles")[0]
    N = A.shape[0]

    def status(indptr=None, indices=None, data=None):
        B = A.copy()
        tri = [np.array(x) for x in (B.indptr if indptr is None else indptr, B.indices if indices is None else indices,
                                     B.data if data is None else data)]
        t = (_dev(tri[0], np.int64), _dev(tri[1], np.int64), _dev(tri[2], np.float64))
        d, s = torch.empty(N, dtype=torch.float64, device=DEV), torch.empty(N, dtype=torch.float64, device=DEV)
        heavy, st = torch.empty(N, dtype=torch.int32, device=DEV), torch.empty(ops.SPECTRAL_STATUS, dtype=torch.int64, device=DEV)
        ops.spectral_degrees(*t, d, s, heavy, st)
        return t, st.tolist(), d.cpu().numpy()

    _, st, d = status()
    assert st == [0, 0, 0, 0, 0] and np.array_equal(d, R.degrees(A)[0])
    idx = A.indices.copy()
    idx[[5, 900]] = [N, -1]
    t, st, _ = status(indices=idx)
    assert st[ops.SPECTRAL_BAD_INDEX] == 2
    with pytest.raises(ValueError, match=r"2 indices outside \[0, 600\)"):
        DeviceGraph(*t)
    data = A.data.copy()
    data[[1, 2, 3]] = [-0.5, np.nan, np.inf]
    t, st, _ = status(data=data)
    assert st[ops.SPECTRAL_BAD_WEIGHT] == 3
    with pytest.raises(ValueError, match="3 entries that are negative or not finite"):
        DeviceGraph(*t)
    ptr = A.indptr.copy()
    ptr[10] = ptr[11] + 1                                           # rows 9 and 10: one too long, one negative in length
    ptr2 = A.indptr.copy()
    ptr2[-1] = A.nnz + 5                                            # past the arrays: read as empty, nothing is loaded there
    t, st, _ = status(indptr=ptr)
    assert st[ops.SPECTRAL_BAD_INDPTR] == 1
    with pytest.raises(ValueError, match="malformed"):
        DeviceGraph(*t)
    _, st, d = status(indptr=ptr2)
    assert st[ops.SPECTRAL_BAD_INDPTR] == 1 and st[ops.SPECTRAL_ISOLATED] == 1 and d[-1] == 0.0
    # an isolated row is counted, not refused
    B = A.tolil(copy=True)
    for j in B.rows[17][:]:
        B[17, j] = 0
        B[j, 17] = 0
    B = B.tocsr()
    B.eliminate_zeros()
    g = DeviceGraph.from_scipy(B, DEV)
    assert g.n_isolated == 1 and float(g.s[17]) == 0.0 and float(g.d[17]) == 0.0


# ------------------------------------------------------------------ (d) fits
WANTED = {"moons": 2, "circles": 2, "blobs5": 5, "cube": 3, "blobs700": 3}      # n_components; one more vector is computed


def _fit(name, seed=0):
    from vit_som_amd import SpectralEmbedding
    with warnings.catch_warnings():
        warnings.filterwarnings("ignore", message="Graph is not fully connected")
        return SpectralEmbedding(WANTED[name], affinity="precomputed", random_state=seed).fit(R.fixture(name)[0])


@pytest.mark.parametrize("name", R.FOUR)
def test_eigenvalues_within_tol_of_dense_eigh(name):
    se = _fit(name)
    lam, _ = R.dense_spectrum(name)
    n = WANTED[name] + 1
    theta, res = se.eigenvalues_.cpu().numpy(), se.residuals_.cpu().numpy()
    print(f"{name}: {se.n_iter_} passes, max residual {res.max():.2e}, max |theta - lambda| {np.abs(theta - lam[:n]).max():.2e}")
    assert se.vectors_.dtype == torch.float64 and se.vectors_.shape == (R.fixture(name)[0].shape[0], n) and se.n_iter_ <= 10
    assert res.max() <= TOL and np.abs(theta - lam[:n]).max() <= TOL
    A = R.fixture(name)[0]
    assert se.n_connected_components_ == scipy.sparse.csgraph.connected_components(A, directed=False)[0]
    assert se.n_neighbors_ is None and abs(se.affinity_matrix_ - A).max() == 0
    # the residuals the device reports are the residuals of the vectors it returns
    M, _, _ = R.operator(A)
    V = se.vectors_.cpu().numpy()
    assert np.abs(np.linalg.norm(M @ V - V * theta, axis=0) - res).max() <= 1e-12
    assert np.abs(V.T @ V - np.eye(n)).max() <= 1e-12
    # a fit is bitwise reproducible for a given random_state
    again = _fit(name)
    assert torch.equal(se.vectors_, again.vectors_) and torch.equal(se.embedding_, again.embedding_)
    assert torch.equal(se.eigenvalues_, again.eigenvalues_) and se.n_iter_ == again.n_iter_


@pytest.mark.parametrize("name", ["blobs700", "cube"])
def test_vectors_and_embedding_against_sklearn(name):
    A = R.fixture(name)[0]
    se = _fit(name)
    n = WANTED[name] + 1
    lam, _ = R.dense_spectrum(name)
    V, res = se.vectors_.cpu().numpy(), se.residuals_.cpu().numpy()
    U = R.sklearn_vectors(A, n)
    for j in range(n):
        gap = np.abs(np.delete(lam, j) - lam[j]).min()             # Davis-Kahan, from the reference spectrum
        sine = np.linalg.norm(U[:, j] - (V[:, j] @ U[:, j]) * V[:, j])
        print(f"{name} column {j}: sine {sine:.2e}, bound {res.max() / gap:.2e}")
        assert sine <= res.max() / gap
    # embedding_ is the f32 rounding of s v with sklearn's sign, the first vector dropped
    _, _, s = R.operator(A)
    want, _ = R.sign_flip(s[:, None] * V[:, 1:])
    got = se.embedding_.cpu().numpy()
    assert got.dtype == np.float32 and np.array_equal(got, want.astype(np.float32))
    sk = R.sklearn_embedding(A, WANTED[name])
    top = np.argmax(np.abs(sk), axis=0)
    assert (got[top, np.arange(WANTED[name])] > 0).all() and (sk[top, np.arange(WANTED[name])] > 0).all()


@pytest.mark.parametrize("name", ["moons", "circles", "blobs5"])
def test_disconnected_fixtures_by_their_projector(name):
    A = R.fixture(name)[0]
    c, labels = scipy.sparse.csgraph.connected_components(A, directed=False)
    assert c == WANTED[name] > 1
    from vit_som_amd import SpectralEmbedding
    with pytest.warns(UserWarning, match="Graph is not fully connected, spectral embedding may not work as expected."):
        se = SpectralEmbedding(WANTED[name], affinity="precomputed", random_state=0).fit(A)
    theta, res = se.eigenvalues_.cpu().numpy(), se.residuals_.cpu().numpy()
    assert np.abs(theta[:c] - 1.0).max() <= TOL and theta[c] < 1.0 - 1e-4
    _, d, _ = R.operator(A)
    B = np.stack([np.sqrt(d) * (labels == k) for k in range(c)], axis=1)
    B /= np.linalg.norm(B, axis=0)
    V = se.vectors_.cpu().numpy()[:, :c]
    sine = np.linalg.norm(V - B @ (B.T @ V), 2)                      # |P - P_ref|_2 of two c-dimensional spaces
    lam, _ = R.dense_spectrum(name)
    print(f"{name}: {c} unit eigenvalues, projector distance {sine:.2e}, bound {np.sqrt(c) * res.max() / (1 - lam[c]):.2e}")
    assert sine <= np.sqrt(c) * res.max() / (1.0 - lam[c] - TOL)


@pytest.mark.parametrize("name", ["moons", "circles"])
def test_spectral_clustering_equals_the_truth_and_sklearn(name):
    from sklearn.cluster import SpectralClustering as SkSC
    from sklearn.metrics import adjusted_rand_score
    from vit_som_amd import SpectralClustering
    X, y = R.moons() if name == "moons" else R.circles()
    with warnings.catch_warnings():
        warnings.filterwarnings("ignore", message="Graph is not fully connected")
        sk = SkSC(2, affinity="nearest_neighbors", n_neighbors=10, random_state=0).fit(X).labels_
        sc = SpectralClustering(2, n_neighbors=10, random_state=0).fit(_dev(X, np.float32))
    got = sc.labels_.cpu().numpy()
    assert sc.labels_.dtype == torch.int64 and sc.labels_.is_cuda and got.shape == (600,)
    assert adjusted_rand_score(y, sk) == 1.0                         # sklearn alone reaches it
    assert adjusted_rand_score(y, got) == 1.0 and adjusted_rand_score(sk, got) == 1.0
    # the device graph has sklearn's structure: symmetric, 1 on the diagonal, 0.5 or 1 elsewhere, at least k entries a row
    G = sc.affinity_matrix_
    assert abs(G - G.T).max() == 0 and (G.diagonal() == 1.0).all() and set(np.unique(G.data)) <= {0.5, 1.0}
    assert np.diff(G.indptr).min() >= 10 and sc.embedding_.shape == (600, 2) and sc.embedding_.dtype == torch.float32
    again = SpectralClustering(2, n_neighbors=10, random_state=0)
    with warnings.catch_warnings():
        warnings.filterwarnings("ignore", message="Graph is not fully connected")
        assert torch.equal(again.fit(_dev(X, np.float32)).labels_, sc.labels_) and torch.equal(again.embedding_, sc.embedding_)


def test_nearest_neighbors_defaults_and_the_device_triple():
    from vit_som_amd import SpectralEmbedding
    X = R.blobs(700, 8, 3, 3.0, 1)[0]
    se = SpectralEmbedding(2, n_neighbors=15, random_state=0).fit(_dev(X, np.float32))
    assert se.n_neighbors_ == 15 and se.embedding_.shape == (700, 2) and se.embedding_.is_cuda
    assert se.residuals_.max().item() <= TOL
    A = se.affinity_matrix_
    tri = SpectralEmbedding(2, affinity="precomputed", random_state=0).fit(_csr(A))
    assert torch.equal(tri.vectors_, se.vectors_) and torch.equal(tri.embedding_, se.embedding_)
    out = SpectralEmbedding(2, n_neighbors=15, random_state=0).fit_transform(_dev(X, np.float32))
    assert torch.equal(out, se.embedding_)
    with pytest.raises(ValueError, match="n_neighbors = 70 must be at most 64"):
        SpectralEmbedding(2).fit(_dev(X, np.float32))                # None -> N // 10
    with pytest.raises(ValueError, match="metric must be one of"):
        SpectralEmbedding(2, n_neighbors=5, metric="manhattan").fit(_dev(X, np.float32))
    cos = SpectralEmbedding(2, n_neighbors=15, metric="cosine", random_state=0).fit(_dev(X, np.float32))
    assert cos.residuals_.max().item() <= TOL and abs(cos.affinity_matrix_ - A).max() > 0


# ------------------------------------------------------------------ (e) UMAP's init and the evaluation path
def test_umap_spectral_device_init():
    from vit_som_amd import UMAP
    from vit_som_amd import umap as UM
    X = _dev(R.blobs(600, 8, 1, 1.0, 3)[0], np.float32)
    host = UMAP(n_neighbors=15, random_state=0, n_epochs=20).fit(X)
    G = host.graph_
    assert scipy.sparse.csgraph.connected_components(G, directed=False)[0] == 1
    dim = 2
    a = UM.spectral_init(G, dim, np.random.RandomState(0), None)
    b = UM.spectral_init(G, dim, np.random.RandomState(0), None, X.device)
    assert a.shape == b.shape == (600, dim)
    M, _, _ = R.operator(G)
    lam = np.linalg.eigvalsh(M.toarray())[::-1]
    gap = min(lam[0] - lam[1], lam[dim] - lam[dim + 1])               # the wanted eigenvalues against the rest
    qa, qb = np.linalg.qr(a)[0], np.linalg.qr(b)[0]
    sine = np.linalg.norm(qb - qa @ (qa.T @ qb), 2)
    # ARPACK's tol = 1e-4 is relative to the eigenvalue, at most |L| = 2; the device's residual is 1e-8
    print(f"UMAP init: subspace sine {sine:.2e}, bound {(2e-4 + 1e-8) * np.sqrt(dim) / gap:.2e}")
    assert sine <= (2e-4 + 1e-8) * np.sqrt(dim) / gap
    dev = UMAP(n_neighbors=15, random_state=0, n_epochs=20, init="spectral_device").fit(X)
    emb = dev.embedding_.cpu().numpy()
    assert emb.shape == (600, 2) and np.isfinite(emb).all() and abs(dev.graph_ - G).max() == 0
    with pytest.raises(ValueError, match="'spectral_device'"):
        UMAP(init="spectral_gpu").fit(X)


def test_evaluate_spectral_on_the_tiny_model(tmp_path):
    from test_knn_gpu import _loaders, _model
    from vit_som_amd import SpectralReport, evaluate_spectral, visualize_spectral_map
    from vit_som_amd.evaluation import _Table, nmi_from_table, purity_from_table
    m, cfg = _model("ref_cluster_tiny")
    train, _ = _loaders(cfg, 4)                                      # 96 samples in batches of 10
    y = torch.cat([b[1] for b in train]).to(DEV).long()
    rep = evaluate_spectral(m, cfg, train, n_neighbors=10)
    k = 4                                                            # the config names no classes: the distinct labels
    assert isinstance(rep, SpectralReport) and (rep.n_clusters, rep.n_neighbors, rep.n_samples) == (k, 10, 96)
    assert rep.labels.shape == (96,) and rep.labels.dtype == torch.int64 and rep.embedding.shape == (96, k)
    assert rep.max_residual <= TOL and 1 <= rep.eigengap_k < len(rep.eigenvalues) and rep.n_connected_components >= 1
    assert (np.diff(rep.eigenvalues) <= 1e-12).all() and abs(rep.eigenvalues[0] - 1.0) <= TOL
    t = _Table(k, 256, DEV)
    t.add(rep.labels, y)
    assert rep.purity == purity_from_table(t.numpy()) and rep.nmi == nmi_from_table(t.numpy())
    assert torch.equal(evaluate_spectral(m, cfg, train, n_neighbors=10).labels, rep.labels)
    assert evaluate_spectral(m, cfg, train, n_clusters=2, n_neighbors=10, max_rows=50).n_samples == 50
    with pytest.raises(ValueError, match="metric must be"):
        evaluate_spectral(m, cfg, train, metric="manhattan")
    m.world_size = 2
    try:
        with pytest.raises(ValueError, match="world_size > 1 is not supported"):
            evaluate_spectral(m, cfg, train)
    finally:
        m.world_size = 1
    emb, labels = visualize_spectral_map(m, cfg, train, n_neighbors=10, output_dir=str(tmp_path))
    assert emb.shape == (96, 2) and emb.dtype == np.float32 and labels.shape == (96,)


def test_driver_reports_spectral(tmp_path):
    import copy
    from helpers import load_golden
    from vit_som_amd.train import main, synthetic_loaders
    _, cfg = load_golden("ref_cluster_tiny")
    cfg = copy.deepcopy(cfg)
    cfg["hyperparameters"]["batch_size"] = 16
    logs = []
    loaders = lambda c, r, w: synthetic_loaders(c, r, w, n_train=64, n_val=16, n_test=16)      # noqa: E731
    today = {"accuracy", "precision", "recall", "f1", "purity", "nmi", "run_duration", "inference_time"}
    new = {"spectral_purity", "spectral_nmi", "spectral_eigengap_k"}
    met = main(cfg, n_runs=1, max_epochs=1, make_loaders=loaders, model_states_dir=str(tmp_path / "a"), log=logs.append,
               spectral_eval=True)
    assert set(met) == today | new and all(len(met[k]) == 1 for k in new)
    assert 0.0 < met["spectral_purity"][0] <= 1.0 and 0.0 <= met["spectral_nmi"][0] <= 1.0 + 1e-12 and met["spectral_eigengap_k"][0] >= 1
    print([line for line in logs if "Spectral" in line])
    assert any(line.startswith("Spectral clustering:") for line in logs)
