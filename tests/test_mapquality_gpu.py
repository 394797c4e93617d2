"""Map quality on the MI355X: vsom_map_stats and vsom_umatrix against their restatements (test_mapquality_cpu.py) on the same
tensors -- the integer results word for word -- and evaluate_map_quality / umatrix / the two pictures on the reference-pinned
fixtures: against the restatement fed with the model's own distances, against float64 from latents and prototypes, with
training undisturbed, over two ranks, and through the training driver."""
import copy
import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from helpers import golden_params, load_golden
from test_mapquality_cpu import NBR, adjacency, fresh_accumulators, grid_positions, map_stats_ref, neighbours_ref, umatrix_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _have_matplotlib():
    try:
        import matplotlib  # noqa: F401
        return True
    except ImportError:
        return False


# ------------------------------------------------------------------ vsom_map_stats
def _device_acc(K):
    return dict(hits=torch.zeros(K, dtype=torch.int64, device=DEV), qe_fix=torch.zeros(K, dtype=torch.int64, device=DEV),
                te=torch.zeros(1, dtype=torch.int64, device=DEV), nearest=torch.full((K,), -1, dtype=torch.int64, device=DEV),
                bad=torch.zeros(1, dtype=torch.int32, device=DEV))


def _fold(dist_dev, bmu, pos, adj, first, acc):
    from vit_som_amd import ops
    second = torch.full((dist_dev.shape[0],), -1, dtype=torch.int64, device=DEV)
    ops.map_stats(dist_dev, bmu, pos, adj, first, acc["hits"], acc["qe_fix"], acc["te"], acc["nearest"], acc["bad"], second=second)
    return second


def _same(acc, ref):
    """The device accumulators against the restatement's: every word equal."""
    torch.cuda.synchronize()
    assert int(acc["bad"].item()) == ref["bad"]
    assert int(acc["te"].item()) == ref["te"]
    assert np.array_equal(acc["hits"].cpu().numpy(), ref["hits"])
    assert np.array_equal(acc["qe_fix"].cpu().numpy(), ref["qe_fix"])
    assert np.array_equal(acc["nearest"].cpu().numpy().view(np.uint64), ref["nearest"])


def _synthetic(seed, B, K):
    """Distances on a grid of 1/128 around zero: ties for every place and small negative values come by themselves.
    The BMU is the first minimum, as the layer's argmin gives it."""
    g = torch.Generator().manual_seed(seed)
    dist = (torch.randint(0, 200, (B, K), generator=g).float() / 128.0 - 0.05).numpy().astype(np.float32)
    return dist, np.argmin(dist, axis=1).astype(np.int64)


@pytest.mark.parametrize("B,rows,cols,topology", [(1, 1, 2, "square"), (37, 5, 7, "square"), (37, 5, 7, "hexa"), (64, 1, 16, "square"),
                                                  (130, 40, 40, "square")])
def test_map_stats_against_restatement(B, rows, cols, topology):
    K = rows * cols
    dist, bmu = _synthetic(B + K, B, K)
    pos = grid_positions(rows, cols, topology)
    ref, second_ref = map_stats_ref(dist, bmu, pos, adjacency(topology), first_ordinal=5)
    assert ref["bad"] == 0 and (B == 1 or 0 < ref["te"] < B)
    assert int(ref["qe_fix"].sum()) == int(np.rint(dist[np.arange(B), bmu].astype(np.float64) * 2.0 ** 32).astype(np.int64).sum())
    dd, bd, pd = torch.from_numpy(dist).to(DEV), torch.from_numpy(bmu).to(DEV), torch.from_numpy(pos).to(DEV)
    runs = []
    for _ in range(2):
        acc = _device_acc(K)
        second = _fold(dd, bd, pd, adjacency(topology), 5, acc)
        _same(acc, ref)
        assert np.array_equal(second.cpu().numpy(), second_ref)
        runs.append((acc, second))
    for name in ("hits", "qe_fix", "te", "nearest", "bad"):                  # the same call twice: identical bytes
        assert torch.equal(runs[0][0][name], runs[1][0][name])
    # without the optional output
    from vit_som_amd import ops
    acc = _device_acc(K)
    ops.map_stats(dd, bd, pd, adjacency(topology), 5, acc["hits"], acc["qe_fix"], acc["te"], acc["nearest"], acc["bad"])
    _same(acc, ref)


def test_map_stats_folds_across_batches():
    """Three batches with advancing first_ordinal into the same accumulators."""
    rows, cols, B = 7, 9, 16
    K = rows * cols
    pos = grid_positions(rows, cols, "hexa")
    pd = torch.from_numpy(pos).to(DEV)
    acc, ref = _device_acc(K), fresh_accumulators(K)
    for n in range(3):
        dist, bmu = _synthetic(40 + n, B, K)
        _, second_ref = map_stats_ref(dist, bmu, pos, 1.5, first_ordinal=n * B, acc=ref)
        second = _fold(torch.from_numpy(dist).to(DEV), torch.from_numpy(bmu).to(DEV), pd, 1.5, n * B, acc)
        assert np.array_equal(second.cpu().numpy(), second_ref)
    _same(acc, ref)
    assert int(ref["hits"].sum()) == 3 * B and int((ref["nearest"] & np.uint64(0xFFFFFFFF)).max()) >= B


def test_map_stats_crafted_rows_and_unaligned_base():
    """Ties for the minimum, the second place and the column minimum across rows and workgroups; -0.0 and small negative
    distances; a NaN row, two BMUs off the map and two rows whose own distance is 2^31 or more in size (counted, skipped);
    the same batch from a base pointer 4 bytes off 16-byte alignment (the scalar path) and from an aligned one."""
    K, nan = 8, float("nan")
    rows = [
        ([0.5, 0.5, 0.75, 0.75, 1, 1, 1, 1], 0),              # the minimum twice: the runner-up equals the BMU's distance
        ([0.75, 1, 0.3, 0.1, 1, 0.3, 1, 1], 3),               # the second place twice: the lower index
        ([-0.0, 0.0, -1e-7, 1, 1, 1, 1, 1e-30], 2),           # -1e-7 < -0.0 == 0.0 for `second`, -0.0 < 0.0 for `nearest`
        ([0.5, 0.5, 0.75, 0.1, 1, 1, 1, 1], 3),               # column minima tied with rows 0 and 1: the lower ordinal
        ([0.2, nan, 0.1, 1, 1, 1, 1, 1], 2),                  # refused
        ([0.2, 0.3, 0.1, 1, 1, 1, 1, 1], 8),                  # refused
        ([0.2, 0.3, 0.1, 1, 1, 1, 1, 1], -1),                 # refused
        ([0.2, 0.3, 0.1, 1, 3e9, 1, 1, 1], 4),                # refused: |dist[i, bmu]| >= 2^31
        ([0.2, 0.3, 0.1, 1, 1, -2.0 ** 31, 1, 1], 5),         # refused (second workgroup from here on)
        ([0.5, 1, 1, 1, 1, 1, 1, -1e-7], 7),                  # ties rows 0 and 2 from another workgroup
        ([3e9, 1, 1, 1, 1, 1, 0.25, 1], 6),                   # a huge distance that is not the BMU's is just a distance
        ([0.0, -0.0, 1, 1, 1, 1, 1, 1], 0),
    ]
    dist = np.array([r for r, _ in rows], dtype=np.float32)
    bmu = np.array([b for _, b in rows], dtype=np.int64)
    pos = grid_positions(2, 4, "square")
    ref, second_ref = map_stats_ref(dist, bmu, pos, 2.25, first_ordinal=100)
    assert ref["bad"] == 5 and second_ref[:4].tolist() == [1, 2, 0, 0] and second_ref[11] == 1
    low = (ref["nearest"] & np.uint64(0xFFFFFFFF)).astype(np.int64) - 100
    assert low.tolist() == [2, 11, 2, 1, 0, 1, 10, 9]
    bd, pd = torch.from_numpy(bmu).to(DEV), torch.from_numpy(pos).to(DEV)
    buf = torch.zeros(dist.size + 4, device=DEV)
    for off in (1, 0):
        view = buf[off:off + dist.size].view(len(rows), K)
        view.copy_(torch.from_numpy(dist))
        assert (view.data_ptr() % 16 != 0) == bool(off)
        acc = _device_acc(K)
        second = _fold(view, bd, pd, 2.25, 100, acc)
        _same(acc, ref)
        assert np.array_equal(second.cpu().numpy(), second_ref)


# ------------------------------------------------------------------ vsom_umatrix
def _neighbours_np(pos, adj_r2):
    p = np.asarray(pos, dtype=np.float64)
    d2 = ((p[:, None, :] - p[None, :, :]) ** 2).sum(-1)
    near = (d2 <= adj_r2) & ~np.eye(len(p), dtype=bool)
    idx = np.full((len(p), NBR), -1, dtype=np.int32)
    for k in range(len(p)):
        js = np.nonzero(near[k])[0]
        idx[k, :len(js)] = js
    return idx


def _umatrix_ref_device(W64, idx, distance, block=100):
    """umatrix_ref's distances in float64 torch on the device, `block` units at a time -> float64 [K, 8] (0 in the padding)."""
    K = W64.shape[0]
    j = torch.from_numpy(idx.astype(np.int64)).to(W64.device)
    out = torch.zeros(K, NBR, dtype=torch.float64, device=W64.device)
    norm = W64.norm(dim=1).clamp_min(1e-12)
    for k0 in range(0, K, block):
        jj = j[k0:k0 + block]
        a, b = W64[k0:k0 + block, None, :], W64[jj.clamp_min(0)]
        if distance == 0:
            d = 1.0 - (a * b).sum(-1) / (norm[k0:k0 + block, None] * norm[jj.clamp_min(0)])
        elif distance == 1:
            d = (a - b).pow(2).sum(-1).sqrt()
        else:
            d = (a - b).abs().sum(-1)
        out[k0:k0 + block] = torch.where(jj >= 0, d, torch.zeros_like(d))
    return out.cpu().numpy()


def _check_umatrix(got, idx_ref, nd_ref, distance):
    """nbr_idx equal; nbr_dist within the rounding of one fp32 store of an fp64 result -- cosine 2.5e-7 absolute (two fp32 ulps at
    1.0), the other two 2.5e-7 of the value; u the fp64 mean of the device's own nbr_dist in slot order, exactly."""
    u, nbr_idx, nbr_dist = (t.cpu().numpy() for t in got)
    assert nbr_idx.dtype == np.int32 and np.array_equal(nbr_idx, idx_ref)
    err = np.abs(nbr_dist.astype(np.float64) - nd_ref)
    bound = 2.5e-7 if distance == 0 else 2.5e-7 * np.abs(nd_ref)
    worst = float((err / np.where(distance == 0, 1.0, np.maximum(np.abs(nd_ref), 1e-300))).max())
    print(f"umatrix distance {distance}: K {len(u)}, worst {'abs' if distance == 0 else 'rel'} error {worst:.3e}")
    assert (err <= bound).all(), worst
    assert (nbr_dist[idx_ref < 0] == 0).all()
    for k in range(len(u)):
        cnt, s = int((idx_ref[k] >= 0).sum()), 0.0
        for n in range(cnt):
            s += float(nbr_dist[k, n])
        assert u[k] == np.float32(s / cnt if cnt else 0.0), k


def _close_prototypes(seed, K, L, spread):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(1, L, generator=g) * (1.0 - spread) + spread * torch.rand(K, L, generator=g)


@pytest.mark.parametrize("distance", [0, 1, 2])
@pytest.mark.parametrize("rows,cols,L,topology,spread,offset", [(3, 4, 20, "square", 1.0, 0), (3, 4, 20, "square", 1.0, 1), (3, 4, 21, "hexa", 1.0, 0),
                                                                 (5, 7, 192, "square", 1.0, 0), (5, 7, 192, "hexa", 0.01, 0)])
def test_umatrix_against_fp64(rows, cols, L, topology, spread, offset, distance):
    """offset = 1: W starts 4 bytes off 16-byte alignment, and L = 21 is no multiple of 4: both take the scalar loads.
    spread = 0.01: neighbouring prototypes that are close, as on a trained map."""
    from vit_som_amd import ops
    K = rows * cols
    W = _close_prototypes(7 * rows + L, K, L, spread)
    pos = grid_positions(rows, cols, topology)
    idx_ref, nd_ref, _ = umatrix_ref(W, pos, adjacency(topology), distance)
    buf = torch.zeros(K * L + 4, device=DEV)
    Wd = buf[offset:offset + K * L].view(K, L)
    Wd.copy_(W)
    assert (Wd.data_ptr() % 16 != 0) == bool(offset)
    got = ops.umatrix(Wd, torch.from_numpy(pos).to(DEV), adjacency(topology), distance)
    _check_umatrix(got, idx_ref, nd_ref, distance)
    again = ops.umatrix(Wd, torch.from_numpy(pos).to(DEV), adjacency(topology), distance)
    assert all(torch.equal(a, b) for a, b in zip(got, again))


def test_umatrix_benchmark_map_against_fp64():
    """The benchmark map once: 40 x 40 units of 12 288 values, the three distances."""
    from vit_som_amd import ops
    g = torch.Generator().manual_seed(11)
    W = torch.nn.functional.normalize(torch.rand(1600, 12288, generator=g), dim=1).to(DEV)     # as the cosine layer starts
    pos = grid_positions(40, 40, "square")
    idx_ref = _neighbours_np(pos, 2.25)
    assert np.array_equal(idx_ref[:41], neighbours_ref(pos[:200], 2.25)[:41])                  # the fast form, where rows 0 - 4 decide
    W64, pd = W.double(), torch.from_numpy(pos).to(DEV)
    for distance in (0, 1, 2):
        _check_umatrix(ops.umatrix(W, pd, 2.25, distance), idx_ref, _umatrix_ref_device(W64, idx_ref, distance), distance)


def test_umatrix_identical_prototypes_and_crowded_neighbourhood():
    from vit_som_amd import ops
    from vit_som_amd._lib import VsomError
    g = torch.Generator().manual_seed(2)
    W = torch.rand(1, 192, generator=g).repeat(35, 1).to(DEV)
    pd = torch.from_numpy(grid_positions(5, 7, "hexa")).to(DEV)
    for distance in (0, 1, 2):
        u, _, nbr_dist = ops.umatrix(W, pd, 1.5, distance)
        assert (u == 0).all() and (nbr_dist == 0).all(), distance
    # a radius that takes in 12 units around an interior cell of the square lattice: refused, with the count
    ps = torch.from_numpy(grid_positions(5, 5, "square")).to(DEV)
    with pytest.raises(VsomError, match="12 units"):
        ops.umatrix(W[:25].contiguous(), ps, 4.0, 1)
    one = ops.umatrix(W[:1].contiguous(), ps[:1].contiguous(), 2.25, 0)                        # a map of one unit has no neighbour
    assert one[0].tolist() == [0.0] and one[1].tolist() == [[-1] * 8]


# ------------------------------------------------------------------ evaluate_map_quality on the fixtures
FIXTURES = ["ref_cluster_tiny", "ref_hexa_euclid_tiny", "ref_manhattan_tiny", "ref_desom_tiny"]


def _model(name):
    import vit_som_amd
    z, cfg = load_golden(name)
    cls = vit_som_amd.DESOM if cfg["hyperparameters"]["model_arch"] == "desom" else vit_som_amd.ViTSOM
    m = cls(copy.deepcopy(cfg), device=DEV)
    m.load_state_dict(golden_params(z))
    return m, cfg, z


def _batches(cfg, nb=10):
    """108 samples in batches of 10: ten full batches and a short last one."""
    from test_kmeans_gpu import _separable_images
    d = cfg["data"]
    return _separable_images(9, 27, 4, d["num_channels"], d["input_size"], nb)


def _shape(x, cfg):
    d = cfg["data"]
    if cfg["hyperparameters"]["model_arch"] == "vit_som":
        return x.reshape(-1, d["num_channels"], d["input_size"], d["input_size"])
    return x.reshape(x.shape[0], -1)


def _collect(m, cfg, batches):
    """Per batch, what the model's forward returns: (dist float32 [B, K], bmu [B]) and the latent rows the SOM layer saw."""
    vit = cfg["hyperparameters"]["model_arch"] == "vit_som"
    out = []
    for x, _ in batches:
        x = _shape(x.to(DEV), cfg)
        res = m(x)
        dist, bmu = (res[3], res[4]) if vit else (res[2], res[3])
        z = m.get_latent_representation(x).clone() if vit else res[1].clone()
        out.append((dist.cpu().numpy(), bmu.cpu().numpy(), z.reshape(z.shape[0], -1).double()))
    return out


def _restated_report(m, parts):
    som = m.som_layer
    pos = som.grid_positions.cpu().numpy()
    ref, seen, seconds = fresh_accumulators(som.n_prototypes), 0, []
    for dist, bmu, _ in parts:
        _, second = map_stats_ref(dist, bmu, pos, som.adjacency_radius2(), first_ordinal=seen, acc=ref)
        seconds.append(second)
        seen += len(bmu)
    return ref, seen, np.concatenate(seconds)


def _d64(z, W64, distance_fcn):
    if distance_fcn == "cosine":
        return 1.0 - torch.nn.functional.normalize(z, dim=1, eps=1e-12) @ torch.nn.functional.normalize(W64, dim=1, eps=1e-12).T
    return torch.cdist(z, W64, p=2 if distance_fcn == "euclidean" else 1, compute_mode="donot_use_mm_for_euclid_dist")


@pytest.mark.parametrize("name", FIXTURES)
def test_evaluate_map_quality_on_fixture(name, tmp_path):
    from vit_som_amd.evaluation import MapQuality, evaluate_map_quality, umatrix, visualize_hit_map, visualize_umatrix
    m, cfg, _ = _model(name)
    m.current_epoch = 3
    arch = cfg["hyperparameters"]["model_arch"]
    som = m.som_layer
    rows, cols = som.map_size
    K = rows * cols
    batches = _batches(cfg)
    assert len(batches) == 11 and len(batches[-1][1]) == 8
    parts = _collect(m, cfg, batches)
    ref, N, second_ref = _restated_report(m, parts)
    assert N == 108 and ref["bad"] == 0

    rep = evaluate_map_quality(m, cfg, batches)
    assert isinstance(rep, MapQuality) and rep.n_samples == N and rep.inference_time > 0
    assert rep.hits.dtype == np.int64 and rep.hits.shape == (rows, cols) and np.array_equal(rep.hits.reshape(-1), ref["hits"])
    assert rep.dead_units == int((ref["hits"] == 0).sum())
    assert rep.topographic_error == ref["te"] / N
    assert rep.nearest_sample.dtype == np.int64
    assert np.array_equal(rep.nearest_sample.reshape(-1), (ref["nearest"] & np.uint64(0xFFFFFFFF)).astype(np.int64))
    all_dist = np.concatenate([p[0] for p in parts])
    all_bmu = np.concatenate([p[1] for p in parts])
    assert np.array_equal(rep.nearest_sample.reshape(-1), np.argmin(all_dist, axis=0))
    assert np.array_equal(rep.nearest_distance.reshape(-1), all_dist.min(axis=0))
    qe64 = float(all_dist[np.arange(N), all_bmu].astype(np.float64).mean())
    print(f"{name}: QE {rep.quantization_error:.6f} (fp64 mean of the fp32 distances {qe64:.6f}), TE {rep.topographic_error:.4f}, "
          f"dead {rep.dead_units}/{K}")
    assert abs(rep.quantization_error - qe64) <= N * 2.0 ** -33 + 1e-12
    with np.errstate(invalid="ignore", divide="ignore"):
        cell = np.where(ref["hits"] > 0, ref["qe_fix"] / 2.0 ** 32 / np.maximum(ref["hits"], 1), np.nan)
    assert np.array_equal(rep.cell_quantization_error.reshape(-1), cell, equal_nan=True)
    again = evaluate_map_quality(m, cfg, batches)
    assert again.quantization_error == rep.quantization_error and np.array_equal(again.nearest_sample, rep.nearest_sample)

    # against float64 from the latents and the prototypes: the device's runner-up is within 2 e_i of the true one
    from vit_som_amd import ops
    W64 = som.prototypes.detach().double()
    adj, pos64 = som.adjacency_radius2(), som.grid_positions.double().cpu().numpy()
    differ = te64 = 0
    for dist, bmu, z in parts:
        d64 = _d64(z, W64, som.distance_fcn).cpu().numpy()
        acc = _device_acc(K)
        second = _fold(torch.from_numpy(dist).to(DEV), torch.from_numpy(bmu).to(DEV), som.grid_positions, adj, 0, acc).cpu().numpy()
        for i in range(len(bmu)):
            e = float(np.abs(dist[i].astype(np.float64) - d64[i]).max())
            rest = np.delete(d64[i], bmu[i])
            assert d64[i, second[i]] <= rest.min() + 2 * e, (i, e)
            order = np.argsort(d64[i], kind="stable")
            differ += int(order[0] != bmu[i] or order[1] != second[i])
            te64 += int(float(((pos64[order[0]] - pos64[order[1]]) ** 2).sum()) > adj)
    print(f"{name}: TE fp64 {te64 / N:.4f}, rows whose (best, second) differ from fp64's: {differ}")
    assert abs(rep.topographic_error - te64 / N) <= differ / N + 1e-15

    # the U-matrix of the same model
    u, nbr_idx, nbr_dist = umatrix(m)
    assert u.shape == (rows, cols) and u.dtype == np.float32
    mode = {"cosine": 0, "euclidean": 1, "manhattan": 2}[som.distance_fcn]
    idx_ref, nd_ref, _ = umatrix_ref(som.prototypes.detach().cpu(), som.grid_positions.cpu().numpy(), adj, mode)
    _check_umatrix((torch.from_numpy(u.reshape(-1)), torch.from_numpy(nbr_idx), torch.from_numpy(nbr_dist)), idx_ref, nd_ref, mode)

    # the pictures
    assert np.array_equal(visualize_umatrix(m, cfg, output_dir=str(tmp_path)), u)
    assert np.array_equal(visualize_hit_map(m, cfg, batches, output_dir=str(tmp_path)), rep.hits)
    if _have_matplotlib():
        assert os.path.getsize(tmp_path / f"{arch}_epoch_3_umatrix.png") > 0
        assert os.path.getsize(tmp_path / f"{arch}_epoch_3_hit_map.png") > 0


def test_evaluate_map_quality_on_a_model_built_on_the_unindexed_device():
    """device="cuda" and device="cuda:0" name the same GPU: the evaluator must read the buffers predict() wrote, not a fresh
    set allocated under the other spelling."""
    import vit_som_amd
    from vit_som_amd.evaluation import evaluate_map_quality
    m0, cfg, z = _model("ref_cluster_tiny")
    m = vit_som_amd.ViTSOM(copy.deepcopy(cfg), device="cuda")
    m.load_state_dict(golden_params(z))
    batches = _batches(cfg)
    a, b = evaluate_map_quality(m0, cfg, batches), evaluate_map_quality(m, cfg, batches)
    assert a.quantization_error == b.quantization_error and a.topographic_error == b.topographic_error
    assert np.array_equal(a.hits, b.hits) and np.array_equal(a.nearest_sample, b.nearest_sample)
    assert len(m.som_layer._bufs) <= 2 and all(s.bmu.device == torch.device("cuda:0") for s in m.som_layer._bufs.values())


def test_evaluate_map_quality_refuses_what_the_kernel_refused():
    from vit_som_amd.evaluation import evaluate_map_quality
    m, cfg, _ = _model("ref_cluster_tiny")
    x, y = _batches(cfg)[0]
    real = m.predict

    def poisoned(xb):                                          # one NaN in the distances predict() left behind
        out = real(xb)
        m.som_layer._buffers_for(out[0].shape[0], xb.device).dist[1, 2] = float("nan")
        return out
    m.predict = poisoned
    with pytest.raises(ValueError, match="^2 rows .* NaN"):
        evaluate_map_quality(m, cfg, [(x, y), (x, y)])
    m.predict = real
    assert evaluate_map_quality(m, cfg, [(x, y)]).n_samples == len(y)
    with pytest.raises(ValueError, match="model_arch"):
        evaluate_map_quality(m, {**cfg, "hyperparameters": {**cfg["hyperparameters"], "model_arch": "vit"}}, [(x, y)])


def test_map_quality_leaves_buffers_and_training_alone(tmp_path):
    """Three training steps at batch 8 (the third records the launch tape), every map-quality call, two more steps (replayed
    from the tape): parameters bitwise those of a twin that made no call; vit._acts holds the same objects."""
    from test_mapviz_gpu import _same_objects, _snapshot
    from vit_som_amd.evaluation import evaluate_map_quality, umatrix, visualize_hit_map, visualize_umatrix
    from vit_som_amd.tuning import hooks
    assert hooks.launch_tape
    g = torch.Generator().manual_seed(0)
    z, cfg = load_golden("ref_cluster_tiny")
    d = cfg["data"]
    xs = [torch.rand(8, d["num_channels"], d["input_size"], d["input_size"], generator=g).to(DEV) for _ in range(5)]
    ys = [torch.randint(0, 4, (8,), generator=g).to(DEV) for _ in range(5)]
    loader = [(x.cpu(), y.cpu()) for x, y in zip(xs, ys)]
    models = []
    for call in (True, False):
        m, _, _ = _model("ref_cluster_tiny")
        m.set_schedule(int(z["n_train"]), int(z["est_steps"]))
        (opt,), _ = m.configure_optimizers()
        for i in range(3):
            m.train_step_fused(xs[i], ys[i])
            opt.step()
        a = m.vit._acts[8]
        tape = a.__dict__.get("tape")
        assert tape is not None and tape.id
        if call:
            snap = _snapshot(m.vit)
            version = a.version
            umatrix(m)
            visualize_umatrix(m, cfg, output_dir=str(tmp_path))
            _same_objects(snap, m.vit)                                 # the U-matrix touches no buffer of the model
            assert a.version == version
            rep = evaluate_map_quality(m, cfg, loader)
            visualize_hit_map(m, cfg, loader, output_dir=str(tmp_path))
            assert rep.n_samples == 40
            _same_objects(snap, m.vit, strict=False)                   # predict runs in the batch-8 buffers, as ever
            assert a.__dict__.get("tape") is tape and tape.valid(m, a)
            m.train()
        for i in range(3, 5):
            m.train_step_fused(xs[i], ys[i])
            opt.step()
        assert m.vit._acts[8].__dict__.get("tape") is tape                  # replayed, not re-recorded
        torch.cuda.synchronize()
        models.append(m)
    assert torch.equal(models[0].arena.params, models[1].arena.params)
    assert torch.equal(models[0].arena.exp_avg, models[1].arena.exp_avg)


def _report_arrays(rep):
    return dict(hits=rep.hits, nearest_sample=rep.nearest_sample, nearest_distance=rep.nearest_distance,
                cell=rep.cell_quantization_error, scalars=np.array([rep.quantization_error, rep.topographic_error, rep.dead_units,
                                                                     rep.n_samples], dtype=np.float64))


def _dp_worker(rank, world, port, out):
    import torch.distributed as dist
    from vit_som_amd.evaluation import evaluate_map_quality
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    m, cfg, _ = _model("ref_cluster_tiny")
    m.world_size, m.rank = world, rank
    mine = [b for i, b in enumerate(_batches(cfg)) if i % world == rank]
    np.savez(f"{out}.{rank}.npz", **_report_arrays(evaluate_map_quality(m, cfg, mine)))
    dist.barrier()
    dist.destroy_process_group()


def test_evaluate_map_quality_two_ranks(tmp_path):
    """Both ranks return the single-process report of the set in rank order (rank 0's batches, then rank 1's)."""
    from test_distributed import _free_port
    from vit_som_amd.evaluation import evaluate_map_quality
    out = str(tmp_path / "mq")
    mp.spawn(_dp_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    m, cfg, _ = _model("ref_cluster_tiny")
    batches = _batches(cfg)
    order = [b for i, b in enumerate(batches) if i % 2 == 0] + [b for i, b in enumerate(batches) if i % 2 == 1]
    single = _report_arrays(evaluate_map_quality(m, cfg, order))
    assert single["scalars"][3] == 108 and single["nearest_sample"].max() >= 58            # a sample of rank 1's shard is nearest somewhere
    for rank in (0, 1):
        got = np.load(f"{out}.{rank}.npz")
        for k, v in single.items():
            assert np.array_equal(got[k], v, equal_nan=True), (rank, k)


def test_driver_reports_map_quality(tmp_path):
    from vit_som_amd.train import main, synthetic_loaders
    _, cfg = load_golden("ref_cluster_tiny")
    cfg = copy.deepcopy(cfg)
    cfg["hyperparameters"]["batch_size"] = 16
    logs = []
    loaders = lambda c, r, w: synthetic_loaders(c, r, w, n_train=64, n_val=16, n_test=16)      # noqa: E731
    today = {"accuracy", "precision", "recall", "f1", "purity", "nmi", "run_duration", "inference_time"}
    met = main(cfg, n_runs=1, max_epochs=1, make_loaders=loaders, model_states_dir=str(tmp_path / "a"), log=logs.append)
    assert set(met) == today
    met = main(cfg, n_runs=1, max_epochs=1, make_loaders=loaders, model_states_dir=str(tmp_path / "b"), log=logs.append, map_quality=True)
    assert set(met) == today | {"quantization_error", "topographic_error"}
    (qe,), (te,) = met["quantization_error"], met["topographic_error"]
    assert np.isfinite(qe) and qe >= 0.0 and 0.0 <= te <= 1.0
    assert len(met["purity"]) == 1 and any("Map quality: quantization error" in l for l in logs)
