"""The batch SOM on the MI355X: vsom_som_batch_accumulate bit for bit against np.add.at in fp64, vsom_som_batch_update within
the project's tolerance rule and at its edges, SOMLayer.fit_batch teacher-forced against the fp64 restatement of
batch_som_ref.py, the memory contract of both entries, and what is built on top (evaluation.fit_som_batch, the driver).

The rule (pca_ref.bound): a value is held to 4 x max(e32, 2^-23) against fp64, e32 being the error of the same formula in
numpy float32, errors measured as the largest absolute error over the largest absolute fp64 value.  The comparisons of
fit_batch are teacher-forced: W_new depends only on the assignments and X, and a free-running comparison of f32 BMUs
against fp64 ones cannot be asked for (the best and second-best distances come within 4e-12 of each other, relative, while
the radius is wide)."""
import copy
import functools
import signal

import numpy as np
import pytest
import torch

import batch_som_ref as B
import memcheck as MC
import pca_ref as R
from helpers import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IDS = [f"{n}x{d}-{r}x{c}" for n, d, (r, c) in B.SHAPES]


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
    a = np.array(a, dtype=dtype) if dtype is not None else np.array(a)
    return torch.from_numpy(a).to(DEV)                                   # a copy: the fixtures are read-only


def _host(t):
    return t.detach().cpu().numpy()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


def _rule(got, ref32, ref64, what):
    err, bound = R.rel_err(got, ref64), R.bound(ref32, ref64)
    print(f"{what}: error {err:.3e}, bound {bound:.3e} (e32 {R.rel_err(ref32, ref64):.3e})")
    assert np.isfinite(np.asarray(got)).all(), what
    assert err <= bound, what


def _strided(X, ld, offset=0, fill=float("nan")):
    """X on the device in rows of `ld` elements starting `offset` floats into an allocation, everything else `fill`."""
    N, D = X.shape
    buf = torch.full((N * ld + offset,), fill, dtype=torch.float32, device=DEV)
    v = buf[offset:].as_strided((N, D), (ld, 1))
    v.copy_(_dev(X))
    return v


def _accumulate(X, bmu, K, inv=None, sums=None, counts=None, accumulate=False, bad=None):
    from vit_som_amd import ops
    D = X.shape[1]
    sums = torch.full((K, D), float("nan"), dtype=torch.float64, device=DEV) if sums is None else sums
    counts = torch.full((K,), -7, dtype=torch.int64, device=DEV) if counts is None else counts
    ops.som_batch_accumulate(X, bmu, sums, counts, inv_norm=inv, accumulate=accumulate, bad=bad)
    return sums, counts


def _same(sums, counts, want):
    return np.array_equal(_bits(_host(sums)), _bits(want[0])) and np.array_equal(_host(counts), want[1])


# ------------------------------------------------------------------ 1. accumulate is exact
@pytest.mark.parametrize("N,D,grid", B.SHAPES, ids=IDS)
def test_accumulate_is_exact(N, D, grid):
    from vit_som_amd import ops
    K = grid[0] * grid[1]
    bmu = B.random_bmu(N, K, 5)
    assert K == 1 or (np.bincount(bmu, minlength=K) == 0).any()
    bd = _dev(bmu)
    Xi = np.random.RandomState(6).randint(-3, 4, size=(N, D)).astype(np.float32)
    assert _same(*_accumulate(_dev(Xi), bd, K), B.accumulate(Xi, bmu, K)), "integer data"
    X, _ = B.fixture(N, D, K)
    Xd = _dev(X)
    want = B.accumulate(X, bmu, K)
    assert _same(*_accumulate(Xd, bd, K), want), "float data"
    inv = ops.row_inv_norm(Xd, torch.empty(N, device=DEV))
    want_inv = B.accumulate(X, bmu, K, _host(inv))
    assert _same(*_accumulate(Xd, bd, K, inv), want_inv), "float data times inv_norm"
    assert not np.array_equal(want_inv[0], want[0])
    # a row pitch of D + 4 with NaN in the padding (the 16-byte path where D % 4 == 0)
    Xp = _strided(X, D + 4)
    assert Xp.stride(0) == D + 4 and Xp.data_ptr() % 16 == 0
    assert _same(*_accumulate(Xp, bd, K, inv), want_inv), "ldx = D + 4"
    # the element-wise path: an odd pitch, the first element one float into the allocation
    ld = D + 1 if D % 2 == 0 else D + 2
    Xo = _strided(X, ld, offset=1)
    assert Xo.stride(0) % 2 == 1 and Xo.data_ptr() % 16 == 4
    assert _same(*_accumulate(Xo, bd, K, inv), want_inv), "odd ldx, offset pointer"


@pytest.mark.parametrize("N,D,K,rows", [(257, 12288, 16, 257), (257, 12288, 16, 256), (2100, 192, 1600, 1500), (700, 40, 30, 321)])
def test_accumulate_long_segments(N, D, K, rows):
    """A unit with more than 256 rows is summed by the cooperative kernel of the 16-byte path (batches of 64 rows, the last
    one partial), one with exactly 256 by the one-wave kernel, in the same launch: the same chain, the same bits.  Also
    continued over two calls."""
    from vit_som_amd import ops
    X, _ = B.fixture(N, D, K)
    bmu = B.random_bmu(N, K, 12)
    full = K // 2
    bmu[bmu == full] = (full + 1) % K
    bmu[np.random.RandomState(13).permutation(N)[:rows]] = full
    assert np.bincount(bmu, minlength=K)[full] == rows
    Xd, bd = _dev(X), _dev(bmu)
    inv = ops.row_inv_norm(Xd, torch.empty(N, device=DEV))
    want = B.accumulate(X, bmu, K, _host(inv))
    assert _same(*_accumulate(Xd, bd, K, inv), want)
    assert _same(*_accumulate(_strided(X, D + 4), bd, K, inv), want), "ldx = D + 4"
    assert _same(*_accumulate(_strided(X, D + 3, offset=1), bd, K, inv), want), "element-wise path"
    cut = N // 2 + 3
    sums, counts = _accumulate(Xd[:cut], bd[:cut], K, inv[:cut])
    assert _same(*_accumulate(Xd[cut:], bd[cut:], K, inv[cut:], sums, counts, accumulate=True), want), "two calls"


# ------------------------------------------------------------------ 2. chunking does not matter
@pytest.mark.parametrize("N,D,grid", [B.SHAPES[0], B.SHAPES[1], B.SHAPES[2]], ids=IDS[:3])
def test_chunking_does_not_matter(N, D, grid):
    from vit_som_amd import ops
    K = grid[0] * grid[1]
    X, _ = B.fixture(N, D, K)
    bmu = B.random_bmu(N, K, 7)
    Xd, bd = _dev(X), _dev(bmu)
    inv = ops.row_inv_norm(Xd, torch.empty(N, device=DEV))
    want = B.accumulate(X, bmu, K, _host(inv))
    whole = _accumulate(Xd, bd, K, inv)
    again = _accumulate(Xd, bd, K, inv)
    assert _same(*whole, want) and torch.equal(whole[0].view(torch.int64), again[0].view(torch.int64))
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    for chunk in (1, 64, 100):
        sums = torch.full((K, D), float("nan"), dtype=torch.float64, device=DEV)
        counts = torch.full((K,), -7, dtype=torch.int64, device=DEV)
        for i in range(0, N, chunk):
            _accumulate(Xd[i:i + chunk], bd[i:i + chunk], K, inv[i:i + chunk], sums, counts, accumulate=i > 0, bad=bad)
        assert _same(sums, counts, want), f"chunks of {chunk}"
    assert int(bad.item()) == 0


# ------------------------------------------------------------------ 3. a BMU off the map
@pytest.mark.parametrize("off", [-1, "K"])
def test_a_bmu_off_the_map_is_flagged_and_not_dereferenced(off):
    from vit_som_amd import ops
    from vit_som_amd._lib import VsomError
    N, D, K = 333, 1003, 35
    X, _ = B.fixture(N, D, K)
    bmu = B.random_bmu(N, K, 8)
    wrong = [3, 170, 332]
    bmu[wrong] = K if off == "K" else -1
    keep = np.setdiff1d(np.arange(N), wrong)
    want = B.accumulate(X[keep], bmu[keep], K)
    x, hx = MC.guarded_copy(_dev(X))
    b, hb = MC.guarded_copy(_dev(bmu))
    sums, hs = MC.guarded((K, D), torch.float64, DEV)
    counts, hc = MC.guarded((K,), torch.int64, DEV)
    with pytest.raises(VsomError, match=rf"3 rows have a BMU outside \[0, {K}\)"):
        ops.som_batch_accumulate(x, b, sums, counts)
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.som_batch_accumulate(x, b, sums, counts, bad=bad)
    torch.cuda.synchronize()
    assert int(bad.item()) == 3
    for h, what in ((hx, "X"), (hb, "bmu"), (hs, "sums"), (hc, "counts")):
        h.check(what)
    hs.all_written("sums"); hc.all_written("counts")
    assert _same(sums, counts, want), "the rows with a BMU on the map"


# ------------------------------------------------------------------ 4. update within the rule
@functools.lru_cache(maxsize=None)
def _sums(N, D, K, seed=9):
    X, _ = B.fixture(N, D, K)
    sums, counts = B.accumulate(X, B.random_bmu(N, K, seed), K)
    sums.setflags(write=False); counts.setflags(write=False)
    return sums, counts


def _update(sums, counts, pos, sigma, normalize, ld=None):
    from vit_som_amd import ops
    K, D = sums.shape
    if ld is None:
        W = torch.full((K, D), float("nan"), device=DEV)
    else:
        W = torch.full((K, ld), float("nan"), device=DEV)[:, :D]
    ops.som_batch_update(_dev(sums), _dev(counts), _dev(pos), sigma, W, normalize=normalize)
    return _host(W)


@pytest.mark.parametrize("normalize", [False, True], ids=["plain", "normalized"])
@pytest.mark.parametrize("topology", ["square", "hexa"])
@pytest.mark.parametrize("N,D,grid", B.SHAPES, ids=IDS)
def test_update_within_the_rule(N, D, grid, topology, normalize):
    K = grid[0] * grid[1]
    sums, counts = _sums(N, D, K)
    pos = B.grid_positions(grid[0], grid[1], topology)
    for sigma in (max(grid) / 2.0, 1.0, 0.3):
        got = _update(sums, counts, pos, sigma, normalize)
        want64 = B.update(sums, counts, pos, sigma, normalize=normalize)
        want32 = B.update(sums, counts, pos, sigma, normalize=normalize, dtype=np.float32)
        _rule(got, want32, want64, f"update {N}x{D} {grid} {topology} sigma={sigma} normalize={normalize}")
        if normalize:
            assert np.abs(np.linalg.norm(got.astype(np.float64), axis=1) - 1.0).max() <= 4 * R.EPS32
        assert np.array_equal(_bits(got), _bits(_update(sums, counts, pos, sigma, normalize, ld=D + 3))), "row stride, second run"


# ------------------------------------------------------------------ 5. update at the edges
@pytest.mark.parametrize("N,D,grid", B.SHAPES, ids=IDS)
def test_update_at_the_edges(N, D, grid):
    K = grid[0] * grid[1]
    sums, counts = _sums(N, D, K)
    X, _ = B.fixture(N, D, K)
    pos = B.grid_positions(grid[0], grid[1], "square")
    hit = counts > 0
    # sigma = 0.05: a hit unit is its own mean, a unit without hits the pooled mean of its equidistant nearest hit units
    got = _update(sums, counts, pos, 0.05, False)
    _rule(got, B.update_limit_small(sums, counts, pos, np.float32), B.update_limit_small(sums, counts, pos), f"sigma = 0.05 {grid}")
    own64 = sums[hit] / counts[hit, None]
    _rule(got[hit], (sums[hit].astype(np.float32) / counts[hit, None].astype(np.float32)), own64, f"hit units at sigma = 0.05 {grid}")
    # sigma = 1e6: every unit is the global mean
    mean64 = np.repeat(X.astype(np.float64).mean(axis=0)[None, :], K, axis=0)
    got = _update(sums, counts, pos, 1e6, False)
    _rule(got, B.update(sums, counts, pos, 1e6, dtype=np.float32), mean64, f"sigma = 1e6 {grid}")
    # all rows in one unit; one row
    for rows, unit in ((X, K // 2), (X[:1], K - 1)):
        s1, c1 = B.accumulate(rows, np.full(len(rows), unit, dtype=np.int64), K)
        m64 = np.repeat(rows.astype(np.float64).mean(axis=0)[None, :], K, axis=0)
        for sigma in (0.3, max(grid) / 2.0):
            got = _update(s1, c1, pos, sigma, False)
            _rule(got, B.update(s1, c1, pos, sigma, dtype=np.float32), m64, f"{len(rows)} rows in unit {unit}, sigma={sigma} {grid}")
    # no unit has a hit: zeros, not NaN
    got = _update(np.zeros((K, D)), np.zeros(K, dtype=np.int64), pos, 1.0, True)
    assert np.array_equal(got, np.zeros((K, D), dtype=np.float32))


# ------------------------------------------------------------------ 6. - 8. fit_batch
def _layer(D, grid, topology="square", distance="euclidean", W0=None):
    from vit_som_amd import SOMLayer
    cfg = {"hyperparameters": {"model_arch": "desom", "total_epochs": 10, "batch_size": 8,
                               "som": {"map_size": list(grid), "Tmax": max(grid) / 2.0, "Tmin": 0.3, "distance_fcn": distance,
                                       "topology": topology},
                               "ae": {"encoder_dims": [D]}},
           "data": {"dataset": "synthetic"}}
    som = SOMLayer(cfg).to(DEV)
    if W0 is not None:
        som.prototypes.data.copy_(_dev(W0))
        som.invalidate_planes()
    return som


def _spy_accumulate(monkeypatch):
    """Record the BMU vector of every ops.som_batch_accumulate call."""
    from vit_som_amd import ops
    seen, real = [], ops.som_batch_accumulate

    def spy(X, bmu, *a, **k):
        seen.append(bmu.clone())
        return real(X, bmu, *a, **k)
    monkeypatch.setattr(ops, "som_batch_accumulate", spy)
    return seen


@pytest.mark.parametrize("topology,distance", [("square", "cosine"), ("hexa", "cosine"), ("square", "euclidean"), ("hexa", "euclidean")])
@pytest.mark.parametrize("N,D,grid", B.SHAPES[:3] + B.SHAPES[5:], ids=IDS[:3] + IDS[5:])
def test_one_epoch_teacher_forced(monkeypatch, N, D, grid, topology, distance):
    K = grid[0] * grid[1]
    X, W0 = B.fixture(N, D, K)
    som = _layer(D, grid, topology, distance, W0)
    Xd = _dev(X)
    dist, bmu = som.forward(Xd)
    qe = float(dist.detach().double().gather(1, bmu.view(-1, 1)).mean())
    seen = _spy_accumulate(monkeypatch)
    sigma = max(grid) / 2.0
    param, before = som.prototypes, som.prototypes.data_ptr()
    rep = som.fit_batch(Xd, epochs=1, sigma=sigma)
    assert som.prototypes is param and param.data_ptr() == before and param.requires_grad
    assert len(seen) == 1 and torch.equal(seen[0], bmu), "the BMUs of the epoch are those of forward() at W0"
    assert rep.moved.tolist() == [N] and rep.sigma.tolist() == [sigma]
    assert abs(rep.quantization_error[0] - qe) <= 1e-12 * qe
    pos = _host(som.grid_positions)
    assert np.array_equal(pos, B.grid_positions(grid[0], grid[1], topology))
    w64, w32, _ = B.epoch(X, W0, pos, sigma, distance, bmu=_host(bmu))
    _rule(_host(som.prototypes), w32, w64, f"one epoch {N}x{D} {grid} {topology} {distance}")
    # the chunking of the search changes nothing
    som2 = _layer(D, grid, topology, distance, W0)
    som2.fit_batch(Xd, epochs=1, sigma=sigma, chunk=100)
    assert torch.equal(som2.prototypes.view(torch.int32), som.prototypes.view(torch.int32))
    assert torch.equal(seen[1], bmu)


@pytest.mark.parametrize("distance", ["cosine", "euclidean"])
@pytest.mark.parametrize("N,D,grid", [B.SHAPES[1], B.SHAPES[3], B.TRAIN_SHAPES[0]], ids=[IDS[1], IDS[3], "600x40-6x5"])
def test_several_epochs_are_the_epochs(N, D, grid, distance):
    K = grid[0] * grid[1]
    X, W0 = B.fixture(N, D, K)
    Xd = _dev(X)
    radii = [max(grid) / 2.0, 1.7, 0.9, 0.3]
    a = _layer(D, grid, "hexa", distance, W0)
    rep = a.fit_batch(Xd, epochs=4, sigma=radii)
    b = _layer(D, grid, "hexa", distance, W0)
    singles = [b.fit_batch(Xd, epochs=1, sigma=s) for s in radii]
    assert torch.equal(a.prototypes.view(torch.int32), b.prototypes.view(torch.int32))
    assert rep.sigma.tolist() == radii and torch.equal(rep.bmu, singles[-1].bmu)
    assert np.array_equal(rep.quantization_error, [s.quantization_error[0] for s in singles])
    assert rep.final_quantization_error == singles[-1].final_quantization_error
    assert rep.quantization_error[1:].tolist() == [s.final_quantization_error for s in singles[:-1]]
    assert rep.moved[0] == N and (rep.moved[1:] <= N).all() and rep.moved.dtype == np.int64
    hits = np.bincount(_host(rep.bmu), minlength=K)
    assert rep.bmu.is_cuda and rep.bmu.dtype == torch.int64 and rep.bmu.shape == (N,)
    assert np.array_equal(rep.hits, hits) and rep.hits.sum() == N and rep.dead_units == int((hits == 0).sum())
    # the default schedule is the layer's own; a pair is the same schedule between two values
    c = _layer(D, grid, "hexa", distance, W0)
    rep = c.fit_batch(Xd, epochs=5)
    assert np.array_equal(rep.sigma, B.schedule(c.Tmax, c.Tmin, 5)) and rep.sigma[0] == c.Tmax
    d = _layer(D, grid, "hexa", distance, W0)
    rep2 = d.fit_batch(Xd, epochs=5, sigma=(c.Tmax, c.Tmin))
    assert np.array_equal(rep2.sigma, rep.sigma) and torch.equal(c.prototypes.view(torch.int32), d.prototypes.view(torch.int32))
    assert _layer(D, grid, "hexa", distance, W0).fit_batch(Xd, epochs=1).sigma.tolist() == [c.Tmax]


@pytest.mark.parametrize("topology,distance", [("square", "cosine"), ("hexa", "euclidean")])
@pytest.mark.parametrize("N,D,grid", B.TRAIN_SHAPES, ids=["600x40-6x5", "2100x192-40x40"])
def test_it_trains(N, D, grid, topology, distance):
    K = grid[0] * grid[1]
    X, W0 = B.fixture(N, D, K)
    som = _layer(D, grid, topology, distance, W0)
    rep = som.fit_batch(_dev(X), epochs=8)
    print(f"{grid} {topology} {distance}: QE {rep.quantization_error.tolist()} -> {rep.final_quantization_error}, "
          f"moved {rep.moved.tolist()}, dead units {rep.dead_units}/{K}")
    assert np.isfinite(rep.quantization_error).all() and rep.final_quantization_error < rep.quantization_error[1]
    W = _host(som.prototypes)
    assert np.isfinite(W).all()
    want = B.quantization_error(X, W, _host(rep.bmu), distance)
    assert abs(rep.final_quantization_error - want) <= 1e-6 * want, (rep.final_quantization_error, want)
    if distance == "cosine":
        assert np.abs(np.linalg.norm(W.astype(np.float64), axis=1) - 1.0).max() <= 4 * R.EPS32


# ------------------------------------------------------------------ 9. memory contract
@pytest.mark.parametrize("fill", MC.FILLS)
@pytest.mark.parametrize("entry", ["accumulate", "accumulate_more", "update", "update_normalized"])
def test_memory_contract(monkeypatch, entry, fill):
    """(333, 1003, 5 x 7): outputs in guard-banded poisoned buffers, scratch of exactly the queried size pre-filled with the
    pattern, X and W_out in rows of D + 8 whose padding is poisoned.  Guards intact, every output element written, the
    result bit for bit that of the plain run."""
    from vit_som_amd import ops
    N, D, K, PAD = 333, 1003, 35, 8
    X, _ = B.fixture(N, D, K)
    bmu = B.random_bmu(N, K, 10)
    sums_h, counts_h = B.accumulate(X, bmu, K)
    pos = B.grid_positions(5, 7, "hexa")
    Xd, bd = _dev(X), _dev(bmu)
    inv = ops.row_inv_norm(Xd, torch.empty(N, device=DEV))
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    f32, f64, i64 = torch.float32, torch.float64, torch.int64

    def run(x, outs):
        if entry.startswith("accumulate"):
            more = entry == "accumulate_more"
            if more:
                outs["sums"].copy_(_dev(sums_h)); outs["counts"].copy_(_dev(counts_h))
            ops.som_batch_accumulate(x, bd, outs["sums"], outs["counts"], inv_norm=inv, accumulate=more, bad=bad)
        else:
            ops.som_batch_update(_dev(sums_h), _dev(counts_h), _dev(pos), 0.8, outs["W"], normalize=entry == "update_normalized")

    shapes = ({"sums": ((K, D), f64, None), "counts": ((K,), i64, None)} if entry.startswith("accumulate")
              else {"W": ((K, D), f32, D + PAD)})
    plain = {k: torch.empty(shape, dtype=dt, device=DEV) for k, (shape, dt, _) in shapes.items()}
    run(Xd, plain)
    torch.cuda.synchronize()

    es = MC.ExactScratch(fill)
    handles, outs = {}, {}
    x, handles["X"] = MC.guarded_copy(Xd, ld=D + PAD)
    for k, (shape, dt, ld) in shapes.items():
        outs[k], handles[k] = MC.guarded(shape, dt, DEV, ld=ld)
    with monkeypatch.context() as mp:
        mp.setattr(ops, "scratch", es)
        run(x, outs)
    torch.cuda.synchronize()
    need = 8 * (K + 1) if entry.startswith("accumulate") else 8 * 4 * K
    assert es.calls == 1 and [key[2] for key in es.arenas] == [need]
    es.check()
    for name, h in handles.items():
        h.check(f"[{fill}] {name}")
    assert torch.equal(x, Xd) and int(bad.item()) == 0
    for k in shapes:
        handles[k].all_written(f"[{fill}] {k}")
        assert np.array_equal(_bits(_host(outs[k])), _bits(_host(plain[k]))), f"[{fill}] {k} differs from the plain run"


# ------------------------------------------------------------------ 10. on top
def _tiny(name, **som):
    import vit_som_amd
    from helpers import golden_params
    z, cfg = load_golden(name)
    cfg = copy.deepcopy(cfg)
    cfg["hyperparameters"]["som"].update(**som)
    cls = vit_som_amd.DESOM if cfg["hyperparameters"]["model_arch"] == "desom" else vit_som_amd.ViTSOM
    m = cls(copy.deepcopy(cfg), device=DEV)
    m.load_state_dict(golden_params(z))
    return m, cfg


@pytest.mark.parametrize("name,som", [("ref_cluster_tiny", {}), ("ref_desom_tiny", {"distance_fcn": "euclidean"})], ids=["vit_som", "desom"])
def test_fit_som_batch(name, som):
    from test_knn_gpu import _loaders
    from vit_som_amd import BatchSOMReport, SOMLayer, fit_som_batch
    from vit_som_amd.evaluation import _som_latents
    m, cfg = _tiny(name, **som)
    train, _ = _loaders(cfg, 4)                                    # 96 samples in batches of 10
    layer = m.som_layer
    K = layer.n_prototypes
    X, _ = _som_latents(m, cfg, train, "test")
    for init, max_rows in ((None, None), ("pca", None), ("sample", 50)):
        m.train()
        param, before, old = layer.prototypes, layer.prototypes.data_ptr(), layer.prototypes.detach().clone()
        rep = fit_som_batch(m, cfg, train, epochs=3, init=init, sigma=(2.0, 0.5), max_rows=max_rows)
        n = 96 if max_rows is None else max_rows
        assert isinstance(rep, BatchSOMReport) and m.training and layer.prototypes is param and param.data_ptr() == before
        assert rep.bmu.shape == (n,) and rep.hits.sum() == n and rep.hits.shape == (K,) and rep.sigma.shape == (3,)
        assert not torch.equal(old, layer.prototypes) and bool(torch.isfinite(layer.prototypes).all())
        assert np.isfinite(rep.quantization_error).all() and rep.final_quantization_error <= rep.quantization_error[1] * (1 + 1e-6)
        # the same as the steps by hand
        ref = SOMLayer(copy.deepcopy(cfg)).to(DEV)
        ref.prototypes.data.copy_(old)
        ref.invalidate_planes()
        if init is not None:
            ref.init_prototypes(X[:n], method=init)
        ref.fit_batch(X[:n], epochs=3, sigma=(2.0, 0.5))
        assert torch.equal(ref.prototypes.view(torch.int32), layer.prototypes.view(torch.int32))
    m.eval()
    fit_som_batch(m, cfg, train, epochs=1)
    assert not m.training
    # predict() sees the new map
    x = torch.cat([b[0] for b in train])[:10].to(DEV)
    d = cfg["data"]
    x = x.reshape(-1, d["num_channels"], d["input_size"], d["input_size"]) if name == "ref_cluster_tiny" else x.reshape(10, -1)
    bmu = m.predict(x)[0] if name == "ref_cluster_tiny" else m(x)[3]
    assert torch.equal(bmu.reshape(-1).long(), layer.forward(X[:10])[1])


def test_predict_after_fit_batch_does_not_use_a_stale_plane_image():
    """200 rows of 256 columns take the pre-split planes path of the cosine search: its image of the prototypes must be
    rebuilt after fit_batch wrote them through a raw pointer."""
    m, cfg = _tiny("ref_cluster_tiny")
    layer = m.som_layer
    K, D = layer.prototypes.shape
    X, _ = B.fixture(200, D, K)
    Xd = _dev(X)
    layer.forward(Xd)
    assert layer._planes_used, "200 x 256 against 15 units is meant to take the planes path"
    layer.fit_batch(Xd, epochs=2, sigma=(1.5, 0.5))
    dist, bmu = layer.forward(Xd)
    layer._wplanes, layer._wplanes_stamp = None, None
    dist2, bmu2 = layer.forward(Xd)
    assert torch.equal(bmu, bmu2) and torch.equal(dist, dist2)


def test_manhattan_is_refused():
    m, cfg = _tiny("ref_desom_tiny")
    assert m.som_layer.distance_fcn == "manhattan"
    D = m.som_layer.prototypes.shape[1]
    with pytest.raises(NotImplementedError, match="weighted median"):
        m.som_layer.fit_batch(torch.zeros(8, D, device=DEV))


def test_driver_som_batch_epochs(tmp_path, monkeypatch):
    import vit_som_amd
    from vit_som_amd.train import main, synthetic_loaders
    _, cfg = load_golden("ref_cluster_tiny")
    cfg = copy.deepcopy(cfg)
    cfg["hyperparameters"]["batch_size"] = 16
    loaders = lambda c, r, w: synthetic_loaders(c, r, w, n_train=64, n_val=16, n_test=16)      # noqa: E731
    steps, real = [], vit_som_amd.ViTSOM.train_step_fused

    def recording(self, *a, **k):
        loss = real(self, *a, **k)
        steps.append(torch.as_tensor(loss).detach().float().reshape(1).clone())      # the value itself, not its printed form
        return loss
    monkeypatch.setattr(vit_som_amd.ViTSOM, "train_step_fused", recording)

    def first_loss(tag, **kw):
        """-> (the bits of the loss of every training step of the run, the first one first; the log)."""
        logs = []
        del steps[:]
        main(cfg, n_runs=1, max_epochs=1, make_loaders=loaders, model_states_dir=str(tmp_path / tag), log=logs.append, **kw)
        assert len(steps) == 4
        return torch.cat(steps).view(torch.int32).cpu(), logs

    today, _ = first_loss("a")
    off, logs = first_loss("b", som_batch_epochs=0)
    assert torch.equal(off, today), "som_batch_epochs=0 leaves every step's loss, the first included, bit for bit as it is without it"
    assert not any("SOM batch map" in l for l in logs)
    on, logs = first_loss("c", som_batch_epochs=2, som_init="pca")
    line = [l for l in logs if "SOM batch map" in l]
    print(line, today.view(torch.float32).tolist(), on.view(torch.float32).tolist())
    assert len(line) == 1 and "2 epochs" in line[0] and " before, " in line[0] and " after" in line[0]
    before, after = (float(line[0].split("quantization error ")[1].split(" before, ")[0]),
                     float(line[0].split(" before, ")[1].split(" after")[0]))
    assert np.isfinite(before) and np.isfinite(after) and on[0] != today[0], "the fitted map changes the first step's loss"
    assert logs.index(line[0]) > [i for i, l in enumerate(logs) if "SOM initialised" in l][0]
    with pytest.raises(ValueError, match="som_batch_epochs"):
        main(cfg, n_runs=1, max_epochs=1, make_loaders=loaders, model_states_dir=str(tmp_path / "d"), log=logs.append, som_batch_epochs=-1)
