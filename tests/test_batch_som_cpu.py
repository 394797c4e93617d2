"""The batch SOM without a GPU: the ABI of the two new entries and their host refusals (status code, error text, no launch),
the fp64 reference of batch_som_ref.py against its own limits, the radius schedule and fit_batch's argument errors, the
driver's flag."""
import copy
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import batch_som_ref as B
from helpers import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 4096                     # stands for a non-null, 16-byte aligned device pointer: nothing is launched, nothing dereferenced
ENTRIES = ("vsom_som_batch_accumulate_parts", "vsom_som_batch_accumulate", "vsom_som_batch_update_parts", "vsom_som_batch_update")


def test_header_signatures_and_exports_agree():
    import vit_som_amd
    from vit_som_amd import evaluation, ops, train
    from vit_som_amd._lib import LIB_PATH, SIGNATURES
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vitsom_hip.h")).read(), flags=re.S)
    raw = ctypes.CDLL(LIB_PATH)
    for name in ENTRIES:
        assert hasattr(raw, name) and name in SIGNATURES and re.search(rf"\b{name}\s*\(", header), name
    assert len(SIGNATURES["vsom_som_batch_accumulate"][1]) == 15 and len(SIGNATURES["vsom_som_batch_update"][1]) == 12
    # no byte-sized scratch argument: the fixed table of test_memory_contract_cpu.py stays complete
    for name, params in re.findall(r"\b(vsom_som_batch_[a-z_]+)\s*\(([^)]*)\)", header):
        assert not re.search(r"\b(ws_bytes|part_bytes|planes_bytes|scratch_bytes)\b", params), name
    assert vit_som_amd.BatchSOMReport is vit_som_amd.som.BatchSOMReport and vit_som_amd.fit_som_batch is evaluation.fit_som_batch
    assert callable(ops.som_batch_accumulate) and callable(ops.som_batch_update) and callable(vit_som_amd.SOMLayer.fit_batch)
    assert inspect.signature(train.main).parameters["som_batch_epochs"].default == 0
    sig = inspect.signature(vit_som_amd.SOMLayer.fit_batch).parameters
    assert (sig["epochs"].default, sig["sigma"].default, sig["chunk"].default) == (10, None, 8192)
    sig = inspect.signature(evaluation.fit_som_batch).parameters
    assert [sig[k].default for k in ("epochs", "init", "sigma", "max_rows")] == [10, None, None, None]


def test_accumulate_refusals_without_a_launch():
    from vit_som_amd._lib import last_error, lib as L
    K, N, D = 16, 50, 12
    assert L.vsom_som_batch_accumulate_parts(K) == K + 1 and L.vsom_som_batch_accumulate_parts(0) == 0
    assert L.vsom_som_batch_accumulate_parts(-3) == 0 and L.vsom_som_batch_accumulate_parts(70000) == 0

    def call(X=P, ldx=D, N=N, D=D, bmu=P, order=P, inv=None, K=K, sums=P, counts=P, acc=0, bad=P, seg=P, n_seg=K + 1):
        return L.vsom_som_batch_accumulate(X, ldx, N, D, bmu, order, inv, K, sums, counts, acc, bad, seg, n_seg, None)

    for kw in (dict(sums=None), dict(counts=None), dict(bad=None), dict(X=None), dict(bmu=None), dict(order=None)):
        assert call(**kw) == -1 and "null pointer" in last_error(), kw
    for kw in (dict(N=-1), dict(K=0), dict(K=-2), dict(D=0), dict(ldx=D - 1)):
        assert call(**kw) == -1 and "bad sizes" in last_error(), kw
    assert call(K=65536, n_seg=1 << 20) == -3 and "65535" in last_error()
    assert call(n_seg=K) == -4
    msg = last_error()
    assert "segment buffer" in msg and ("too small" in msg or "<" in msg)
    assert call(seg=None, n_seg=1 << 30) == -4 and call(n_seg=0) == -4 and call(n_seg=-1) == -4


def test_update_refusals_without_a_launch():
    from vit_som_amd._lib import last_error, lib as L
    K, D = 16, 12
    assert L.vsom_som_batch_update_parts(K) == 4 * K and L.vsom_som_batch_update_parts(0) == 0 and L.vsom_som_batch_update_parts(-1) == 0

    def call(sums=P, counts=P, pos=P, K=K, D=D, sigma=1.0, normalize=0, W=P, ldw=D, part=P, n_part=4 * K):
        return L.vsom_som_batch_update(sums, counts, pos, K, D, sigma, normalize, W, ldw, part, n_part, None)

    for kw in (dict(sums=None), dict(counts=None), dict(pos=None), dict(W=None)):
        assert call(**kw) == -1 and "null pointer" in last_error(), kw
    for kw in (dict(K=0), dict(K=-1), dict(D=0), dict(ldw=D - 1)):
        assert call(**kw) == -1 and "bad sizes" in last_error(), kw
    for sigma in (0.0, -1.0, float("nan"), float("inf"), -float("inf"), 1e-200, 1e200):
        assert call(sigma=sigma) == -1 and "sigma" in last_error(), sigma
    assert call(n_part=4 * K - 1) == -4
    msg = last_error()
    assert "partial buffer" in msg and ("too small" in msg or "<" in msg)
    assert call(part=None, n_part=1 << 30) == -4 and call(n_part=0) == -4


# ------------------------------------------------------------------ the reference itself
def _case(N, D, rows, cols, seed):
    K = rows * cols
    X, _ = B.fixture(N, D, K)
    bmu = B.random_bmu(N, K, seed)
    return B.accumulate(X, bmu, K) + (X, bmu)


@pytest.mark.parametrize("topology", ["square", "hexa"])
def test_the_shift_cancels_where_nothing_underflows(topology):
    sums, counts, _, _ = _case(333, 40, 5, 7, 1)
    assert (counts == 0).any() and counts.sum() == 333
    pos = B.grid_positions(5, 7, topology)
    for sigma in (3.5, 1.0, 0.5):
        a, b = B.update(sums, counts, pos, sigma), B.update(sums, counts, pos, sigma, shifted=False)
        assert np.isfinite(a).all() and np.isfinite(b).all()
        assert np.abs(a - b).max() <= 1e-12 * np.abs(a).max()
    # at Tmin = 0.1 the unshifted form divides two underflowing numbers for a unit without hits; the shifted one does not
    with np.errstate(all="ignore"):
        assert not np.isfinite(B.update(sums, counts, pos, 0.02, shifted=False)).all()
    assert np.isfinite(B.update(sums, counts, pos, 0.02)).all()


def test_the_limits_of_the_update():
    sums, counts, X, bmu = _case(130, 3, 3, 3, 2)
    pos = B.grid_positions(3, 3, "square")
    hit = counts > 0
    assert hit.any() and not hit.all()
    small = B.update(sums, counts, pos, 0.05)
    assert np.allclose(small[hit], sums[hit] / counts[hit, None], rtol=1e-13, atol=0)
    assert np.allclose(small, B.update_limit_small(sums, counts, pos), rtol=1e-13, atol=0)
    wide = B.update(sums, counts, pos, 1e6)
    assert np.allclose(wide, X.astype(np.float64).mean(axis=0)[None, :], rtol=1e-9, atol=1e-12)
    # all rows in one unit, one row, a 1 x 1 map: every unit is that mean
    one = np.full(130, 4, dtype=np.int64)
    s1, c1 = B.accumulate(X, one, 9)
    assert np.allclose(B.update(s1, c1, pos, 0.3), X.astype(np.float64).mean(axis=0)[None, :], rtol=1e-12)
    s1, c1 = B.accumulate(X[:1], np.array([7]), 9)
    assert np.array_equal(B.update(s1, c1, pos, 0.3), np.repeat(X[:1].astype(np.float64), 9, axis=0))
    s1, c1 = B.accumulate(X, np.zeros(130, dtype=np.int64), 1)
    assert np.allclose(B.update(s1, c1, B.grid_positions(1, 1, "square"), 0.3), X.astype(np.float64).mean(axis=0)[None, :], rtol=1e-12)
    W = B.update(sums, counts, pos, 1.0, normalize=True)
    assert np.abs(np.linalg.norm(W, axis=1) - 1).max() < 1e-14


def test_accumulate_reference_does_not_depend_on_the_chunking():
    X, _ = B.fixture(333, 1003, 35)
    bmu = B.random_bmu(333, 35, 3)
    inv = B.inv_norm32(X)
    whole = B.accumulate(X, bmu, 35, inv)
    s, c = None, None
    for i in range(0, 333, 64):
        s, c = B.accumulate(X[i:i + 64], bmu[i:i + 64], 35, inv[i:i + 64], s, c)
    assert np.array_equal(whole[0].view(np.int64), s.view(np.int64)) and np.array_equal(whole[1], c)
    loop = np.zeros((35, 1003))
    for i in range(333):
        loop[bmu[i]] += X[i].astype(np.float64) * np.float64(inv[i])
    assert np.array_equal(loop.view(np.int64), whole[0].view(np.int64))


def _layer(distance="cosine", map_size=(3, 5)):
    from vit_som_amd import SOMLayer
    _, cfg = load_golden("ref_cluster_tiny")
    cfg = copy.deepcopy(cfg)
    cfg["hyperparameters"]["som"].update(map_size=list(map_size), distance_fcn=distance)
    return SOMLayer(cfg)


def test_schedule_endpoints_and_forms():
    som = _layer()
    s = som.batch_sigma_schedule(10)
    assert s.shape == (10,) and s.dtype == np.float64 and s[0] == som.Tmax and abs(s[-1] - som.Tmin) <= 1e-15 * som.Tmax
    assert np.allclose(s, B.schedule(som.Tmax, som.Tmin, 10), rtol=1e-15) and (np.diff(s) < 0).all()
    assert np.allclose(s[1:] / s[:-1], (som.Tmin / som.Tmax) ** (1 / 9), rtol=1e-12)
    assert np.array_equal(som.batch_sigma_schedule(1), [som.Tmax])
    assert np.array_equal(som.batch_sigma_schedule(3, 0.7), [0.7, 0.7, 0.7])
    assert np.allclose(som.batch_sigma_schedule(5, (2.0, 0.3)), B.schedule(2.0, 0.3, 5), rtol=1e-15)
    assert np.array_equal(som.batch_sigma_schedule(1, (2.0, 0.3)), [2.0])
    assert np.array_equal(som.batch_sigma_schedule(2, (2.0, 0.3)), [2.0, 0.3])
    assert np.array_equal(som.batch_sigma_schedule(4, [3.0, 1.0, 2.0, 0.5]), [3.0, 1.0, 2.0, 0.5])
    assert np.array_equal(B.schedule(2.0, 0.3, 1), [2.0]) and B.schedule(2.0, 0.3, 7)[0] == 2.0


def test_fit_batch_argument_errors():
    import torch
    som = _layer()
    D = som.prototypes.shape[1]
    X = torch.zeros(8, D)
    with pytest.raises(ValueError, match=rf"latents must be \[N, {D}\]"):
        som.fit_batch(torch.zeros(8, D + 1))
    with pytest.raises(ValueError, match="latents must be"):
        som.fit_batch(torch.zeros(D))
    with pytest.raises(ValueError, match="epochs must be >= 1"):
        som.fit_batch(X, epochs=0)
    with pytest.raises(ValueError, match="empty"):
        som.fit_batch(torch.zeros(0, D))
    for sigma in (0.0, -1.0, (2.0, 0.0), [1.0, -0.5, 1.0], float("nan"), float("inf")):
        with pytest.raises(ValueError, match="positive and finite"):
            som.fit_batch(X, epochs=3, sigma=sigma)
    with pytest.raises(ValueError, match="sigma must be None, a number, a pair"):
        som.fit_batch(X, epochs=5, sigma=[1.0, 0.9, 0.8])
    with pytest.raises(ValueError, match="chunk"):
        som.fit_batch(X, chunk=0)
    with pytest.raises(NotImplementedError, match="weighted median"):
        _layer("manhattan").fit_batch(X)


def test_driver_flag_parses_and_defaults_to_off():
    from vit_som_amd import train
    assert train._parser().parse_args(["--config", "c.yaml"]).som_batch_epochs == 0
    assert train._parser().parse_args(["--config", "c.yaml", "--som-batch-epochs", "7"]).som_batch_epochs == 7
    a = train._parser().parse_args(["--config", "c.yaml", "--som-init", "pca", "--som-batch-epochs", "2"])
    assert (a.som_init, a.som_batch_epochs) == ("pca", 2)
    with pytest.raises(ValueError, match="som_batch_epochs"):
        train.main({"hyperparameters": {}}, som_batch_epochs=-1)
