"""Timing of the batch SOM at the sizes users run (profiles/r16_batch_som.txt).

    python tools/batch_som_bench.py [--out profiles/r16_batch_som.txt] [--repeats 7] [--rows 10000 50000] [--no-model]

kernels: per epoch at N rows, D = 12 288, K = 1 600 (40 x 40, square, cosine): the BMU search (SOMLayer._bmu_search, chunks of
8 192 rows), ops.som_batch_accumulate (torch.sort of the BMUs + vsom_som_batch_accumulate) with the BMUs of an EARLY epoch
(the first search from the random start) and of a LATE one (after ten epochs), with SKEWED ones (the late BMUs with nine rows
in ten moved into four units: what a wide radius does to a map started far from the data), the sort alone, and
ops.som_batch_update; alternated in one process, one warm-up round, device events around each call.  Accumulate is set
against X read once at the gathered-row rate (5.5 TB/s, the lower figure measured for 1-2 KiB rows), update against
2 K^2 D FLOP at the 157.3 TF f32 matrix-core peak.
end to end: SOMLayer.fit_batch(epochs=10) by wall clock around calls that end in a device synchronise.
model (skipped with --no-model): evaluation.fit_som_batch on the flagship ViT-SOM (bench.py's c3 config) over a synthetic
loader, wall clock; quantization error, topographic error and dead units from evaluate_map_quality on the same loader after
init="pca" alone and after init="pca" plus ten batch epochs.
Everything is printed and written to --out."""
import argparse
import copy
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_F32_TF = 157.3
GATHER_TBS = 5.5
D, GRID = 12288, (40, 40)
K = GRID[0] * GRID[1]


def _row(say, name, t, unit="ms"):
    med = statistics.median(t)
    say(f"{name:30s} " + " ".join(f"{v:9.3f}" for v in t) + f"   median {med:9.3f}  min {min(t):9.3f}  max {max(t):9.3f}  "
        f"spread {(max(t) - min(t)) / med:.4f}  ({unit})")
    return med


def _layer():
    import torch
    from vit_som_amd import SOMLayer
    cfg = {"hyperparameters": {"model_arch": "desom", "total_epochs": 10, "batch_size": 512,
                               "som": {"map_size": list(GRID), "Tmax": 4.0, "Tmin": 0.1, "distance_fcn": "cosine", "topology": "square"},
                               "ae": {"encoder_dims": [D]}}, "data": {"dataset": "synthetic"}}
    torch.manual_seed(0)
    return SOMLayer(cfg).to("cuda")


def data(N):
    """Clustered rows, like real latents: 64 centres in a 32-dimensional subspace, noise, a column mean."""
    import torch
    g = torch.Generator(device="cuda").manual_seed(0)
    C = torch.randn(64, 32, device="cuda", generator=g) @ torch.randn(32, D, device="cuda", generator=g) / 32 ** 0.5
    lab = torch.randint(0, 64, (N,), device="cuda", generator=g)
    X = C[lab]
    X.add_(0.6 * torch.randn(N, D, device="cuda", generator=g)).add_(0.5)
    return X


def kernels(N, repeats, say):
    import torch
    from vit_som_amd import ops
    X = data(N)
    som = _layer()
    early = torch.empty(N, dtype=torch.int64, device="cuda")
    som._bmu_search(X, early, 8192)
    t0 = time.perf_counter()
    rep = som.fit_batch(X, epochs=10)
    torch.cuda.synchronize()
    first = time.perf_counter() - t0
    late = rep.bmu
    g = torch.Generator(device="cuda").manual_seed(1)
    skewed = torch.where(torch.rand(N, device="cuda", generator=g) < 0.9, torch.randint(0, 4, (N,), device="cuda", generator=g) * 401, late)
    inv = ops.row_inv_norm(X, torch.empty(N, device="cuda"))
    sums = torch.empty(K, D, dtype=torch.float64, device="cuda")
    counts = torch.empty(K, dtype=torch.int64, device="cuda")
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    W = torch.empty(K, D, device="cuda")
    scratch_bmu = torch.empty(N, dtype=torch.int64, device="cuda")
    pos = som.grid_positions.float().contiguous()
    arms = {"search": lambda: som._bmu_search(X, scratch_bmu, 8192),
            "accumulate early": lambda: ops.som_batch_accumulate(X, early, sums, counts, inv_norm=inv, bad=bad),
            "accumulate late": lambda: ops.som_batch_accumulate(X, late, sums, counts, inv_norm=inv, bad=bad),
            "accumulate skewed": lambda: ops.som_batch_accumulate(X, skewed, sums, counts, inv_norm=inv, bad=bad),
            "sort alone": lambda: torch.sort(late, stable=True),
            "update sigma=4": lambda: ops.som_batch_update(sums, counts, pos, 4.0, W, normalize=True),
            "update sigma=0.3": lambda: ops.som_batch_update(sums, counts, pos, 0.3, W, normalize=True)}
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
    he, hl, hs = torch.bincount(early, minlength=K), torch.bincount(late, minlength=K), torch.bincount(skewed, minlength=K)
    say(f"## kernels: N {N}, D {D}, K {K} (40 x 40 square, cosine); ms per call (device events), {repeats} repeats after one warm-up "
        f"round, alternated")
    say(f"early BMUs: {int((he > 0).sum())} units hit, the fullest holds {int(he.max())} rows ({100 * int(he.max()) / N:.1f} %); "
        f"late BMUs: {int((hl > 0).sum())} units hit, the fullest holds {int(hl.max())} rows; skewed BMUs: {int((hs > 0).sum())} units hit, "
        f"the four fullest hold {int(hs.topk(4).values.sum())} rows")
    med = {name: _row(say, name, times[name]) for name in arms}
    floor = N * D * 4 / (GATHER_TBS * 1e12) * 1e3
    for name in ("accumulate early", "accumulate late", "accumulate skewed"):
        say(f"{name}: bound = X read once at {GATHER_TBS} TB/s = {floor:.3f} ms -> {100 * floor / med[name]:.1f} % of the bound's rate "
            f"with the sort, {100 * floor / max(med[name] - med['sort alone'], 1e-9):.1f} % without it")
    flop = 2.0 * K * K * D
    floor = flop / (PEAK_F32_TF * 1e12) * 1e3
    for name in ("update sigma=4", "update sigma=0.3"):
        say(f"{name}: {flop / 1e9:.1f} GFLOP, bound at {PEAK_F32_TF} TF = {floor:.3f} ms -> {flop / (med[name] * 1e-3) / 1e12:.1f} TF = "
            f"{100 * floor / med[name]:.1f} % of the f32 matrix peak (pre-pass and row normalisation included)")
    say(f"per epoch (search + accumulate late + update sigma=0.3): {med['search'] + med['accumulate late'] + med['update sigma=0.3']:.3f} ms")
    wall = []
    for r in range(repeats):
        som2 = _layer()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        som2.fit_batch(X, epochs=10)
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
    say(f"## end to end: SOMLayer.fit_batch(X [{N}, {D}], epochs=10) from the random start; wall ms, {repeats} repeats (the first call "
        f"of the process, allocations included: {first * 1e3:.1f} ms)")
    _row(say, "fit_batch(epochs=10)", wall)
    say(f"that run: QE {rep.quantization_error[0]:.5f} before the first update, {rep.quantization_error[1]:.5f} after it, "
        f"{rep.final_quantization_error:.5f} at the end; dead units {rep.dead_units}/{K}")


def model(n_images, say):
    import torch
    import bench
    import vit_som_amd
    from vit_som_amd.evaluation import evaluate_map_quality, fit_som_batch, init_som_from_data
    from vit_som_amd.train import synthetic_loaders
    cfg = bench.c3_config(500)
    torch.manual_seed(0)
    m = vit_som_amd.ViTSOM(copy.deepcopy(cfg), device="cuda:0")
    m.eval()
    train, _, _ = synthetic_loaders(cfg, n_train=n_images, n_val=500, n_test=500)
    init_som_from_data(m, cfg, train, method="pca")
    a = evaluate_map_quality(m, cfg, train)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rep = fit_som_batch(m, cfg, train, epochs=10, init="pca")
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    b = evaluate_map_quality(m, cfg, train)
    say(f"## model: flagship ViT-SOM (bench.py c3: 40 x 40 cosine map on 12 288-wide latents, untrained encoder), {a.n_samples} synthetic "
        f"images in batches of 500")
    say(f"fit_som_batch(epochs=10, init='pca') end to end (encoder pass, PCA, ten epochs), one call, wall: {wall * 1e3:.1f} ms")
    say(f"init='pca' alone:          QE {a.quantization_error:.6f}  TE {a.topographic_error:.4f}  dead units {a.dead_units}/{K}")
    say(f"init='pca' + 10 epochs:    QE {b.quantization_error:.6f}  TE {b.topographic_error:.4f}  dead units {b.dead_units}/{K}")
    say(f"fit_batch's own report: QE {rep.quantization_error.tolist()} -> {rep.final_quantization_error:.6f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16_batch_som.txt"))
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--rows", type=int, nargs="+", default=[10000, 50000])
    ap.add_argument("--images", type=int, default=10000)
    ap.add_argument("--no-model", action="store_true")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("batch_som_bench: no GPU; a timing taken anywhere else says nothing")
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    arch = getattr(torch.cuda.get_device_properties(0), "gcnArchName", "?").split(":")[0]
    say(f"# batch SOM on one MI355X ({arch}; torch reports the device name {torch.cuda.get_device_name(0)!r}): "
        f"tools/batch_som_bench.py --repeats {a.repeats}")
    for N in a.rows:
        kernels(N, a.repeats, say)
    if not a.no_model:
        model(a.images, say)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
