"""Map quality without a GPU: the numpy / torch restatements of vsom_map_stats and vsom_umatrix that the GPU tests
(test_mapquality_gpu.py) compare the kernels with, checked here against hand-computed 2 x 3 and 3 x 3 maps of both
topologies; SOMLayer.adjacency_radius2; the host-side refusals of the two C entries; the public names."""
import inspect
import math

import numpy as np
import pytest
import torch

NBR = 8
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)


# ------------------------------------------------------------------ restatements
def grid_positions(rows, cols, topology):
    """SOMLayer.create_grid_positions, restated: square (row, col); hexa (col + 0.5 on odd rows, row * sqrt(3) / 2)."""
    pos = np.zeros((rows * cols, 2), dtype=np.float32)
    for k in range(rows * cols):
        r, c = divmod(k, cols)
        pos[k] = (r, c) if topology == "square" else (c + (0.5 if r % 2 == 1 else 0.0), r * np.sqrt(3) / 2)
    return pos


def adjacency(topology):
    return {"square": 2.25, "hexa": 1.5}[topology]


def ordered_key(v):
    """fp32 -> uint32, order-preserving: the sign bit set for v >= +0, every bit flipped otherwise."""
    b = np.asarray(v, dtype=np.float32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def fresh_accumulators(K):
    return dict(hits=np.zeros(K, dtype=np.int64), qe_fix=np.zeros(K, dtype=np.int64), te=0, bad=0,
                nearest=np.full(K, EMPTY, dtype=np.uint64))


def map_stats_ref(dist, bmu, pos, adj_r2, first_ordinal=0, acc=None):
    """vsom_map_stats on host arrays: returns (acc, second [B] int64 with -1 on the skipped rows).  dist is float32."""
    dist = np.asarray(dist, dtype=np.float32)
    B, K = dist.shape
    acc = fresh_accumulators(K) if acc is None else acc
    second = np.full(B, -1, dtype=np.int64)
    p64 = np.asarray(pos, dtype=np.float64)
    for i in range(B):
        b, row = int(bmu[i]), dist[i]
        if not 0 <= b < K or np.isnan(row).any() or not abs(float(row[b])) < 2.0 ** 31:
            acc["bad"] += 1
            continue
        others = [k for k in range(K) if k != b]
        s = others[int(np.argmin(row[others]))]            # first minimum; -0.0 == 0.0
        second[i] = s
        if float(((p64[b] - p64[s]) ** 2).sum()) > adj_r2:
            acc["te"] += 1
        acc["hits"][b] += 1
        acc["qe_fix"][b] += int(np.rint(np.float64(row[b]) * 2.0 ** 32))       # exact: a 24-bit mantissa times 2^32
        words = (ordered_key(row).astype(np.uint64) << np.uint64(32)) | np.uint64(first_ordinal + i)
        acc["nearest"] = np.minimum(acc["nearest"], words)
    return acc, second


def neighbours_ref(pos, adj_r2):
    p = np.asarray(pos, dtype=np.float64)
    K = len(p)
    idx = np.full((K, NBR), -1, dtype=np.int32)
    for k in range(K):
        near = [j for j in range(K) if j != k and float(((p[j] - p[k]) ** 2).sum()) <= adj_r2]
        assert len(near) <= NBR
        idx[k, :len(near)] = near
    return idx


def umatrix_ref(W, pos, adj_r2, distance):
    """-> (nbr_idx int32 [K, 8], nbr_dist float64 [K, 8], u float64 [K]) in float64 torch; distance 0 / 1 / 2 = cosine /
    euclidean (difference form) / manhattan."""
    W = torch.as_tensor(W).double()
    idx = neighbours_ref(pos, adj_r2)
    K = W.shape[0]
    nd = np.zeros((K, NBR))
    u = np.zeros(K)
    for k in range(K):
        js = [int(j) for j in idx[k] if j >= 0]
        if not js:
            continue
        a, b = W[k:k + 1], W[js]
        if distance == 0:
            d = 1.0 - (a * b).sum(1) / (a.norm(dim=1).clamp_min(1e-12) * b.norm(dim=1).clamp_min(1e-12))
        elif distance == 1:
            d = (a - b).pow(2).sum(1).sqrt()
        else:
            d = (a - b).abs().sum(1)
        nd[k, :len(js)] = d.numpy()
        u[k] = nd[k, :len(js)].sum() / len(js)
    return idx, nd, u


# ------------------------------------------------------------------ the restatements on hand-computed maps
H = math.sqrt(3) / 2


def test_grid_positions_and_neighbours_2x3_and_3x3():
    sq = grid_positions(2, 3, "square")
    assert sq.tolist() == [[0, 0], [0, 1], [0, 2], [1, 0], [1, 1], [1, 2]]
    n = neighbours_ref(sq, 2.25)
    assert n[0].tolist() == [1, 3, 4, -1, -1, -1, -1, -1]                   # corner
    assert n[1].tolist() == [0, 2, 3, 4, 5, -1, -1, -1]                     # edge
    assert n[5].tolist() == [1, 2, 4, -1, -1, -1, -1, -1]
    hx = grid_positions(2, 3, "hexa")
    assert np.allclose(hx, [[0, 0], [1, 0], [2, 0], [0.5, H], [1.5, H], [2.5, H]], atol=1e-7)      # the odd row sits half a cell right
    n = neighbours_ref(hx, 1.5)
    assert [r[r >= 0].tolist() for r in n] == [[1, 3], [0, 2, 3, 4], [1, 4, 5], [0, 1, 4], [1, 2, 3, 5], [2, 4]]
    # interior cells: 8 neighbours on the square lattice, 6 on the hexagonal one
    assert neighbours_ref(grid_positions(3, 3, "square"), 2.25)[4].tolist() == [0, 1, 2, 3, 5, 6, 7, 8]
    assert neighbours_ref(grid_positions(3, 3, "hexa"), 1.5)[4].tolist() == [1, 2, 3, 5, 7, 8, -1, -1]
    assert neighbours_ref(grid_positions(3, 3, "hexa"), 1.5)[3].tolist() == [0, 1, 4, 6, 7, -1, -1, -1]


@pytest.mark.parametrize("topology,te", [("square", 1), ("hexa", 2)])
def test_map_stats_restatement_by_hand(topology, te):
    dist = np.array([[0.5, 0.25, 1, 1, 1, 1],          # bmu 1, second 0: neighbours on both lattices
                     [1, 1, 0.125, 1, 1, 0.25],        # bmu 2, second 5: neighbours on both
                     [0.25, 1, 0.5, 1, 1, 1],          # bmu 0, second 2: two cells apart
                     [0.25, 1, 1, 1, 0.5, 1]],         # bmu 0, second 4: diagonal -- a neighbour on the square lattice only
                    dtype=np.float32)
    bmu = np.array([1, 2, 0, 0])
    acc, second = map_stats_ref(dist, bmu, grid_positions(2, 3, topology), adjacency(topology), first_ordinal=10)
    assert second.tolist() == [0, 5, 2, 4] and acc["te"] == te and acc["bad"] == 0
    assert acc["hits"].tolist() == [2, 1, 1, 0, 0, 0]
    assert acc["qe_fix"].tolist() == [2 ** 31, 2 ** 30, 2 ** 29, 0, 0, 0]
    assert (acc["nearest"] & np.uint64(0xFFFFFFFF)).tolist() == [12, 10, 11, 10, 13, 11]          # ties: the lowest ordinal
    assert (acc["nearest"] >> np.uint64(32)).tolist() == ordered_key(np.float32([0.25, 0.25, 0.125, 1, 0.5, 0.25])).tolist()
    # refused rows leave no trace
    bad = dist.copy()
    bad[1, 3] = np.nan
    acc2, second2 = map_stats_ref(bad, np.array([1, 2, 6, -1]), grid_positions(2, 3, topology), adjacency(topology))
    assert acc2["bad"] == 3 and second2.tolist() == [0, -1, -1, -1] and acc2["hits"].tolist() == [0, 1, 0, 0, 0, 0]
    assert (acc2["nearest"] & np.uint64(0xFFFFFFFF)).tolist() == [0] * 6


def test_ordered_key_order():
    v = np.float32([-1e-7, -0.0, 0.0, 1e-30, 1, np.inf])
    key = ordered_key(v)
    assert (np.diff(key.astype(np.int64)) > 0).all()
    assert key[1] == 0x7FFFFFFF and key[2] == 0x80000000
    from vit_som_amd.evaluation import _key_to_float
    assert np.array_equal(_key_to_float(key).view(np.uint32), v.view(np.uint32))


def test_umatrix_restatement_by_hand():
    W = np.array([[1, 0], [0, 1], [1, 1], [2, 0], [0, 0], [3, 4]], dtype=np.float32)
    pos = grid_positions(2, 3, "hexa")
    idx, nd, u = umatrix_ref(W, pos, 1.5, 1)
    assert idx[0].tolist()[:2] == [1, 3] and np.allclose(nd[0, :2], [math.sqrt(2), 1]) and abs(u[0] - (math.sqrt(2) + 1) / 2) < 1e-15
    _, nd, u = umatrix_ref(W, pos, 1.5, 2)
    assert nd[5, :2].tolist() == [5.0, 7.0] and u[5] == 6.0             # units 2 and 4
    _, nd, _ = umatrix_ref(W, pos, 1.5, 0)
    assert abs(nd[0, 0] - 1.0) < 1e-15 and abs(nd[0, 1]) < 1e-15        # orthogonal; parallel
    assert abs(nd[3, 2] - 1.0) < 1e-15                                  # unit 4 is the zero vector: the epsilon keeps 1 - 0


def test_adjacency_radius2():
    from vit_som_amd.som import SOMLayer

    class Layer:
        adjacency_radius2 = SOMLayer.adjacency_radius2
    for topology, r2, most in (("square", 2.25, 8), ("hexa", 1.5, 6)):
        layer = Layer()
        layer.topology = topology
        assert layer.adjacency_radius2() == r2 == adjacency(topology)
        counts = (neighbours_ref(grid_positions(5, 7, topology), r2) >= 0).sum(1)
        assert counts.max() == most and counts.min() == (3 if topology == "square" else 2)


# ------------------------------------------------------------------ the C-ABI on the host
def test_map_quality_entries_reject_bad_calls_on_the_host():
    """Each refusal carries its status code and is made before any launch (this process has no device to launch on)."""
    from vit_som_amd._lib import last_error, lib
    ok = dict(dist=16, bmu=16, B=4, K=6, pos=16, r2=2.25, first=0, hits=16, qe=16, te=16, nearest=16, bad=16, second=None)

    def stats(**kw):
        a = {**ok, **kw}
        return lib.vsom_map_stats(a["dist"], a["bmu"], a["B"], a["K"], a["pos"], a["r2"], a["first"], a["hits"], a["qe"], a["te"],
                                  a["nearest"], a["bad"], a["second"], None)
    for name in ("dist", "bmu", "pos", "hits", "qe", "te", "nearest", "bad"):
        assert stats(**{name: None}) == -1 and "null" in last_error(), name
    assert stats(K=1) == -1 and "second-best" in last_error()
    assert stats(K=0) == -1 and stats(B=-1) == -1 and stats(first=-1) == -1
    assert stats(first=2 ** 31 - 4) == -3 and "2^31" in last_error()
    assert stats(B=2 ** 31) == -3
    assert stats(B=0) == 0 and stats(B=0, second=16) == 0                   # nothing to fold, nothing launched

    oku = dict(W=16, K=6, L=8, pos=16, r2=1.5, distance=0, idx=16, nd=16, u=16, status=16)

    def um(**kw):
        a = {**oku, **kw}
        return lib.vsom_umatrix(a["W"], a["K"], a["L"], a["pos"], a["r2"], a["distance"], a["idx"], a["nd"], a["u"], a["status"], None)
    for name in ("W", "pos", "idx", "nd", "u", "status"):
        assert um(**{name: None}) == -1 and "null" in last_error(), name
    assert um(K=0) == -1 and um(L=0) == -1 and um(r2=-1.0) == -1
    assert um(distance=7) == -3 and "distance 7" in last_error()
    assert um(distance=-1) == -3


def test_public_names():
    import vit_som_amd
    from vit_som_amd import ops, train
    ev = vit_som_amd.evaluation
    for name in ("evaluate_map_quality", "umatrix", "visualize_umatrix", "visualize_hit_map"):
        assert callable(getattr(ev, name))
    assert vit_som_amd.MapQuality is ev.MapQuality and vit_som_amd.evaluate_map_quality is ev.evaluate_map_quality
    fields = [f.name for f in ev.MapQuality.__dataclass_fields__.values()]
    assert fields == ["quantization_error", "topographic_error", "hits", "dead_units", "cell_quantization_error", "nearest_sample",
                      "nearest_distance", "n_samples", "inference_time"]
    assert callable(ops.map_stats) and callable(ops.umatrix)
    assert inspect.signature(train.main).parameters["map_quality"].default is False
