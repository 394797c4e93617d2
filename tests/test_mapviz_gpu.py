"""The map pictures on the MI355X: vsom_proto_mosaic and vsom_last_label against their restatements (test_mapviz_cpu.py),
visualize_decoded_prototypes / decode_prototype against the oracle's decoder on the reference-pinned fixtures and at the
benchmark architecture, the decoder-only buffers (memory, training undisturbed), visualize_label_heatmap against the
reference's loop (ViTSOM, DESOM, two ranks) and the epoch in the file names."""
import copy
import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from helpers import golden_params, load_golden
from test_mapviz_cpu import check_canvas, last_label_loop, unpatchify_np

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _have_matplotlib():
    try:
        import matplotlib  # noqa: F401
        return True
    except ImportError:
        return False


# ------------------------------------------------------------------ vsom_proto_mosaic
def _synthetic_pred(seed, K, n, p, C, kind):
    g = torch.Generator().manual_seed(seed)
    pred = torch.rand(K, n + 1, p * p * C, generator=g)
    if kind == "unit":                       # fractions spread over [0, 1]
        pass
    elif kind == "wide":                     # well outside [0, 1]: C == 3 clips, C == 1 rescales
        pred = pred * 60.0 - 25.0
    else:
        pred = pred * 2.0 - 0.5
    pred[:, 0] = 1e6                         # the CLS rows: must never show
    return pred


MOSAIC_CASES = [  # (C, p, g, rows, cols, gap, kind)
    (1, 2, 3, 3, 5, 1, "unit"), (3, 2, 3, 3, 5, 0, "unit"), (1, 4, 2, 5, 4, 3, "wide"), (3, 4, 8, 3, 5, 1, "wide"),
    (1, 16, 2, 2, 3, 0, "mixed"), (3, 16, 2, 4, 4, 3, "mixed"), (3, 4, 8, 7, 9, 1, "unit"), (1, 1, 5, 3, 5, 1, "mixed"),
    (3, 1, 3, 2, 2, 1, "mixed"),
]


@pytest.mark.parametrize("C,p,g,rows,cols,gap,kind", MOSAIC_CASES)
def test_proto_mosaic_against_restatement(C, p, g, rows, cols, gap, kind):
    """Float output: bitwise the torch index shuffle.  Canvas: the float64 restatement outside 1e-3 of a level around the
    rounding boundaries (at most 1 % of the pixels: ~0.2 % for spread fractions), within one level everywhere.  Written in
    two chunks at offsets 0 and K // 2 - 1 into a canvas full of a sentinel; one constant image (C == 1: all 0)."""
    from vit_som_amd import ops
    K, n, S = rows * cols, g * g, g * p
    pred = _synthetic_pred(100 * C + 10 * p + gap + rows, K, n, p, C, kind)
    pred[2, 1:] = 0.625                      # a constant image
    ref = unpatchify_np(pred.numpy(), n, p, C)
    # the restatement alone: the zone holds few pixels for this seed
    cut = K // 2 - 1
    runs = []
    for _ in range(2):
        images = torch.full((K, C, S, S), float("nan"), device=DEV)
        canvas = torch.full((rows * S + (rows - 1) * gap, cols * S + (cols - 1) * gap, 3), 7, dtype=torch.uint8, device=DEV)
        for k0, k1 in ((0, cut), (cut, K)):
            chunk = pred[k0:k1].to(DEV).reshape(-1, p * p * C).contiguous()
            ops.proto_mosaic(chunk, n, p, C, k0, (rows, cols), images=images, canvas=canvas, gap=gap)
        torch.cuda.synchronize()
        runs.append((images.cpu().numpy(), canvas.cpu().numpy()))
    (img, cv), (img2, cv2) = runs
    assert np.array_equal(img, img2) and np.array_equal(cv, cv2)
    assert np.array_equal(img.view(np.uint32), ref.view(np.uint32))
    check_canvas(cv, ref, rows, cols, gap, zone=1e-3, max_excused=0.01)
    r, c = divmod(2, cols)
    cell = cv[r * (S + gap):r * (S + gap) + S, c * (S + gap):c * (S + gap) + S]
    assert (cell == (0 if C == 1 else 159)).all()            # 255 * 0.625 + 0.5 = 159.875
    # either output alone
    only_img = torch.empty(K, C, S, S, device=DEV)
    only_cv = torch.full_like(torch.from_numpy(cv), 9).to(DEV)
    full = pred.to(DEV).reshape(-1, p * p * C).contiguous()
    ops.proto_mosaic(full, n, p, C, 0, (rows, cols), images=only_img)
    ops.proto_mosaic(full, n, p, C, 0, (rows, cols), canvas=only_cv, gap=gap)
    assert np.array_equal(only_img.cpu().numpy(), img) and np.array_equal(only_cv.cpu().numpy(), cv)


def test_proto_mosaic_unaligned_pred():
    """A pred that does not start on 16 bytes takes the scalar path: same output."""
    from vit_som_amd import ops
    C, p, g, rows, cols = 3, 2, 3, 2, 3
    K, n, S = 6, 9, 6
    pred = _synthetic_pred(5, K, n, p, C, "mixed")
    ref = unpatchify_np(pred.numpy(), n, p, C)
    buf = torch.empty(pred.numel() + 1, device=DEV)
    view = buf[1:].view(-1, p * p * C)
    view.copy_(pred.reshape(-1, p * p * C))
    assert view.data_ptr() % 16 != 0
    images = torch.empty(K, C, S, S, device=DEV)
    canvas = torch.zeros(rows * S + rows - 1, cols * S + cols - 1, 3, dtype=torch.uint8, device=DEV)
    ops.proto_mosaic(view, n, p, C, 0, (rows, cols), images=images, canvas=canvas, gap=1)
    assert np.array_equal(images.cpu().numpy(), ref)
    check_canvas(canvas.cpu().numpy(), ref, rows, cols, 1, zone=1e-3, max_excused=0.01)


# ------------------------------------------------------------------ vsom_last_label
def _fold(bmu, label, K, cuts):
    from vit_som_amd import ops
    cells = torch.zeros(K, dtype=torch.int64, device=DEV)
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    edges = [0] + list(cuts) + [len(bmu)]
    for a, b in zip(edges[:-1], edges[1:]):
        ops.last_label(bmu[a:b].contiguous(), label[a:b].contiguous(), a, cells, bad)
    torch.cuda.synchronize()
    return cells.cpu().numpy(), int(bad.item())


def test_last_label_against_the_reference_loop():
    g = torch.Generator().manual_seed(3)
    N, K = 1_000_000, 16
    bmu = torch.randint(0, K - 3, (N,), generator=g)          # cells 13, 14, 15 are never hit
    label = torch.randint(0, 1001, (N,), generator=g)
    ref = last_label_loop(bmu.numpy(), label.numpy(), 4, 4)
    assert (ref.reshape(-1)[13:] == 0).all()
    bd, ld = bmu.to(DEV), label.to(DEV)
    one, bad = _fold(bd, ld, K, [])
    assert bad == 0 and np.array_equal((one & 0xFFFFFFFF).reshape(4, 4), ref)
    assert ((one >> 32)[:13] >= N - 200).all() and (one[13:] == 0).all()      # the winners are the last samples
    split, bad2 = _fold(bd, ld, K, [1, 17, 4099, 500_000, 999_999])
    again, _ = _fold(bd, ld, K, [])
    assert bad2 == 0 and np.array_equal(split, one) and np.array_equal(again, one)
    # big labels survive; a label of 0 on the last hit shows as 0
    b2 = torch.tensor([5, 5, 2, 2], device=DEV)
    y2 = torch.tensor([7, 2 ** 31 - 1, 9, 0], device=DEV)
    c2, bad3 = _fold(b2, y2, 8, [])
    assert bad3 == 0 and (c2 & 0xFFFFFFFF).tolist() == [0, 0, 0, 0, 0, 2 ** 31 - 1, 0, 0] and c2[2] == 4 << 32 and (c2 >= 0).all()


def test_last_label_counts_what_is_out_of_range():
    b = torch.tensor([0, -1, 16, 3, 3, 2], device=DEV)
    y = torch.tensor([4, 5, 6, -7, 2 ** 31, 8], device=DEV)
    cells, bad = _fold(b, y, 16, [])
    assert bad == 4
    assert (cells & 0xFFFFFFFF).tolist() == [4, 0, 8] + [0] * 13


# ------------------------------------------------------------------ visualize_decoded_prototypes on the fixtures
def _vitsom(name="ref_cluster_tiny"):
    import vit_som_amd
    z, cfg = load_golden(name)
    m = vit_som_amd.ViTSOM(copy.deepcopy(cfg), device=DEV)
    m.load_state_dict(golden_params(z))
    return m, cfg, z


def _oracle_images(P, protos, cfg, block=400):
    """O.unpatchify(O.vit_forward_decoder(P, tokens, d)[0], p) with decode_prototype's zero-CLS tokens."""
    from oracle import vitsom_oracle as O
    d = O.Dims(cfg)
    out = []
    for k0 in range(0, protos.shape[0], block):
        w = protos[k0:k0 + block]
        tokens = torch.cat([torch.zeros(w.shape[0], 1, d.E, dtype=w.dtype, device=w.device), w.reshape(w.shape[0], d.n, d.E)], dim=1)
        out.append(O.unpatchify(O.vit_forward_decoder(P, tokens, d)[0], d.p))
    return torch.cat(out)


@pytest.mark.parametrize("name", ["ref_cluster_tiny", "ref_mnistlike_tiny", "ref_cls_tiny"])
def test_visualize_decoded_prototypes_against_oracle(name, tmp_path, capsys):
    from vit_som_amd.evaluation import decode_prototype, decoded_prototype_canvas, visualize_decoded_prototypes
    m, cfg, z = _vitsom(name)
    m.current_epoch = 5
    P = golden_params(z)
    rows, cols = m.som_layer.map_size
    C, S = cfg["data"]["num_channels"], cfg["data"]["input_size"]
    ref = _oracle_images(P, P["som_layer.prototypes"], cfg).numpy()
    got = visualize_decoded_prototypes(m, cfg, output_dir=str(tmp_path), return_decoded=True)
    assert isinstance(got, np.ndarray) and got.shape == (rows * cols, C, S, S) and got.dtype == np.float32
    err = float(np.abs(got.astype(np.float64) - ref).max())
    print(f"{name}: decoded prototypes vs oracle, max abs err {err:.3e}")
    assert err <= 2e-5, err
    if _have_matplotlib():
        assert os.path.getsize(tmp_path / "vit_som_epoch_5_decoded_prototypes.png") > 0
        assert "Saved decoded prototypes visualization" in capsys.readouterr().out
    assert visualize_decoded_prototypes(m, cfg, output_dir=str(tmp_path)) is None          # return_decoded=False
    # the canvas against the restatement applied to the ORACLE's images: the zone is 255 x 2e-5 of a level, doubled
    img, canvas = decoded_prototype_canvas(m, cfg)
    assert np.array_equal(img, got)
    assert canvas.shape == (rows * S + rows - 1, cols * S + cols - 1, 3)
    check_canvas(canvas, ref, rows, cols, 1, zone=1e-2, max_excused=0.05)
    _, canvas0 = decoded_prototype_canvas(m, cfg, gap=0)
    assert canvas0.shape == (rows * S, cols * S, 3)
    # decode_prototype, the reference's helper: one prototype
    vit_hp = cfg["hyperparameters"]["vit"]
    n = (S // vit_hp["patch_size"]) ** 2
    for k in (0, rows * cols - 1):
        one = decode_prototype(m.vit, m.som_layer.prototypes[k].detach().cpu(), n, vit_hp["emb_dim"], m.arena.device)
        assert one.shape == (1, C, S, S) and one.is_cuda
        assert float((one[0].cpu() - torch.from_numpy(got[k])).abs().max()) <= 2e-5
        assert float((one[0].cpu().double() - torch.from_numpy(ref[k]).double()).abs().max()) <= 2e-5
    # chunks: 4 against 512 within 2e-5; the same chunk twice bitwise
    a4, c4 = decoded_prototype_canvas(m, cfg, chunk=4)
    b4, d4 = decoded_prototype_canvas(m, cfg, chunk=4)
    assert np.array_equal(a4, b4) and np.array_equal(c4, d4)
    assert float(np.abs(a4.astype(np.float64) - got).max()) <= 2e-5
    img2, canvas2 = decoded_prototype_canvas(m, cfg)
    assert np.array_equal(img2, img) and np.array_equal(canvas2, canvas)


def test_decoded_prototypes_refusals(capsys):
    import vit_som_amd
    from vit_som_amd.evaluation import visualize_decoded_prototypes
    msg = "Visualization supported only for vit_som with use_reduced=False."
    m, cfg, _ = _vitsom()
    red = copy.deepcopy(cfg)
    red["hyperparameters"]["som"]["use_reduced"] = True
    mr = vit_som_amd.ViTSOM(copy.deepcopy(red), device=DEV)
    assert visualize_decoded_prototypes(mr, red) is None and msg in capsys.readouterr().out
    zd, cfgd = load_golden("ref_desom_tiny")
    dm = vit_som_amd.DESOM(copy.deepcopy(cfgd), device=DEV)
    assert visualize_decoded_prototypes(dm, cfgd) is None and msg in capsys.readouterr().out
    from test_classifier_gpu import vit_config
    cfgc = vit_config(3, 16, 4, 48, 1, 3, 10, 8)
    vc = vit_som_amd.ViTClassifier(copy.deepcopy(cfgc), device=DEV)
    assert visualize_decoded_prototypes(vc, cfgc) is None and msg in capsys.readouterr().out
    # a wrong prototype width
    bad = copy.deepcopy(cfg)
    bad["hyperparameters"]["vit"]["emb_dim"] += 4
    with pytest.raises(ValueError, match="Prototype dimensions mismatch for decoding."):
        visualize_decoded_prototypes(m, bad)
    with pytest.raises(ValueError):
        m.vit.decode_prototypes(m.som_layer.prototypes[:, :-1])


# ------------------------------------------------------------------ the benchmark architecture
def _bench_arch_config():
    """bench.py's architecture (E = 192, decoder 96 x 2, 40 x 40 map, L = 12 288) with ONE encoder block: only the
    decoder runs here."""
    from oracle.gen_golden import make_config
    return make_config(3, 32, 4, 192, 1, 3, 96, 2, (40, 40), 0, 512)


def test_fullsize_decoded_prototypes_fp64_memory_and_time():
    """All 1600 prototypes of the benchmark architecture against the oracle's decoder in float64 (parameters perturbed as
    the decoder goldens' were: N(0, 0.1) on every 1-D parameter), bound 1e-4 absolute as for recon at large shapes.
    Measured on an MI355X: max abs error 2.3e-6 (values span -3.0 .. 2.6).  The extra peak device memory of the call
    stays below 1 GiB (derived: the decoder-only set of a 512-prototype chunk is ~3.5 k floats x 33 280 rows = 0.47 GB,
    + 20 MB of images + the canvas, doubled; measured 470.8 MiB).  The canvas is held to the restatement outside
    2 x 255 x 1e-4 of a level around the rounding boundaries (uniformly spread fractions would put 10 % of the pixels
    there: bound 15 %; measured 3.0 %, most values being clipped).  The batched path is timed against the only way
    without it, 1600 forward_decoder calls at batch 1 + unpatchify: measured 1.75 ms against 391 ms, device events."""
    import vit_som_amd
    from test_fullsize_fp64_gpu import _perturbed_params
    from vit_som_amd.evaluation import decoded_prototype_canvas
    cfg = _bench_arch_config()
    P = _perturbed_params(cfg, seed=7)
    m = vit_som_amd.ViTSOM(copy.deepcopy(cfg), device=DEV)
    m.load_state_dict(P)
    vit, protos = m.vit, m.som_layer.prototypes.detach()
    assert tuple(protos.shape) == (1600, 12288)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    images, canvas = decoded_prototype_canvas(m, cfg)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - before
    print(f"full size: extra peak device memory {extra / 2 ** 20:.1f} MiB")
    assert extra < 2 ** 30, extra
    assert set(vit._acts) == set()                                          # no training-size buffer set was built
    assert images.shape == (1600, 3, 32, 32) and canvas.shape == (40 * 32 + 39, 40 * 32 + 39, 3)

    P64 = {k: (v.to(DEV).double() if v.is_floating_point() else v.to(DEV)) for k, v in P.items()}
    ref = _oracle_images(P64, P64["som_layer.prototypes"], cfg).cpu().numpy()
    err = float(np.abs(images.astype(np.float64) - ref).max())
    print(f"full size: decoded prototypes vs fp64 oracle, max abs err {err:.3e} (values span {ref.min():.2f} .. {ref.max():.2f})")
    assert err <= 1e-4, err
    check_canvas(canvas, ref, 40, 40, 1, zone=255 * 1e-4 * 2, max_excused=0.15)

    # time: compute part, device events, after the warm-up call above
    import time
    e0, e1, e2, e3 = (torch.cuda.Event(enable_timing=True) for _ in range(4))
    torch.cuda.synchronize()
    e0.record()
    vit.decode_prototypes(protos, m.som_layer.map_size)
    e1.record()
    zero = torch.zeros(1, 1, 192, device=DEV)
    with torch.no_grad():
        vit.forward_decoder(torch.cat([zero, protos[0].view(1, 64, 192)], dim=1))  # warm-up of the batch-1 buffers
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e2.record()
    with torch.no_grad():                                                          # as evaluation.py:168 runs it
        for k in range(1600):
            patches, _ = vit.forward_decoder(torch.cat([zero, protos[k].view(1, 64, 192)], dim=1))
            one = vit.unpatchify(patches)
    e3.record()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    batched, single = e0.elapsed_time(e1), e2.elapsed_time(e3)
    print(f"full size: batched decode + mosaic {batched:.2f} ms; 1600 x forward_decoder(batch 1) + unpatchify {single:.1f} ms "
          f"(wall {wall * 1e3:.1f} ms)")
    assert float((one[0].cpu().double() - torch.from_numpy(ref[1599])).abs().max()) <= 1e-4
    assert batched < single, (batched, single)


# ------------------------------------------------------------------ buffers and training undisturbed
def _leaves(obj, path=""):
    """(path, value) of every tensor and plain value reachable through buffer holders and lists."""
    from vit_som_amd._base import _Acts
    if isinstance(obj, _Acts):
        for k, v in obj.__dict__.items():
            yield from _leaves(v, f"{path}.{k}")
    elif isinstance(obj, (list, tuple)):
        for i, v in enumerate(obj):
            yield from _leaves(v, f"{path}[{i}]")
    else:
        yield path, obj


def _snapshot(vit):
    return {B: (a, list(_leaves(a))) for B, a in vit._acts.items()}


def _same_objects(before, vit, strict=True):
    """vit._acts holds the same keys, holders and tensor objects as at the snapshot; strict: nothing added and the same
    `version` too."""
    assert list(vit._acts) == list(before)
    for B, (a, leaves) in before.items():
        assert vit._acts[B] is a
        now = dict(_leaves(a))
        if strict:
            assert list(now) == [p for p, _ in leaves]
        for path, v in leaves:
            if isinstance(v, torch.Tensor):
                assert now[path] is v, path
            elif strict and isinstance(v, (int, float, str, bool)):
                assert now[path] == v, path


def test_visualisations_leave_buffers_and_training_alone(tmp_path):
    """Three training steps at batch 8 (the third records the launch tape), both visualisations, two more steps (replayed
    from the tape): parameters bitwise those of a twin that made no call; vit._acts holds the same objects."""
    from vit_som_amd.evaluation import visualize_decoded_prototypes, visualize_label_heatmap
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
        m, _, _ = _vitsom()
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
            out = visualize_decoded_prototypes(m, cfg, output_dir=str(tmp_path), return_decoded=True)
            assert out is not None
            _same_objects(snap, m.vit)
            assert a.version == version and a.__dict__.get("tape") is tape and tape.valid(m, a)
            visualize_label_heatmap(m, cfg, loader, output_dir=str(tmp_path))
            _same_objects(snap, m.vit, strict=False)                  # predict runs in the batch-8 buffers, as ever
            assert a.__dict__.get("tape") is tape and tape.valid(m, a)
            m.train()
        for i in range(3, 5):
            m.train_step_fused(xs[i], ys[i])
            opt.step()
        assert m.vit._acts[8].__dict__.get("tape") is tape                 # replayed, not re-recorded
        torch.cuda.synchronize()
        models.append(m)
    assert torch.equal(models[0].arena.params, models[1].arena.params)
    assert torch.equal(models[0].arena.exp_avg, models[1].arena.exp_avg)


# ------------------------------------------------------------------ visualize_label_heatmap
def _batches(cfg, nb=12):
    from test_kmeans_gpu import _separable_images
    d = cfg["data"]
    return _separable_images(9, 27, 4, d["num_channels"], d["input_size"], nb)


def _reference_heatmap(m, cfg, batches, arch):
    d = cfg["data"]
    bmus, labels = [], []
    for x, y in batches:
        x = x.to(DEV)
        x = x.reshape(-1, d["num_channels"], d["input_size"], d["input_size"]) if arch == "vit_som" else x.reshape(x.shape[0], -1)
        bmus.append(m.predict(x)[0].cpu().numpy().copy())
        labels.append(y.numpy())
    rows, cols = m.som_layer.map_size
    return last_label_loop(np.concatenate(bmus), np.concatenate(labels), rows, cols), np.concatenate(bmus)


def test_visualize_label_heatmap_vitsom(tmp_path):
    from vit_som_amd.evaluation import visualize_label_heatmap
    m, cfg, _ = _vitsom()
    m.current_epoch = 2
    batches = _batches(cfg)
    assert len(batches) == 9 and sum(len(y) for _, y in batches) == 108
    ref, bmus = _reference_heatmap(m, cfg, batches, "vit_som")
    assert len(np.unique(bmus)) < 108                                       # 108 samples on 15 cells: collisions
    got = visualize_label_heatmap(m, cfg, batches, output_dir=str(tmp_path))
    assert got.dtype == np.int64 and got.shape == (3, 5) and np.array_equal(got, ref)
    assert np.array_equal(visualize_label_heatmap(m, cfg, batches, output_dir=str(tmp_path)), got)
    if _have_matplotlib():
        assert os.path.getsize(tmp_path / "vit_som_epoch_2_label_heatmap.png") > 0
    # reversed batch order gives the reference loop's answer for THAT order
    rev = list(reversed(batches))
    assert np.array_equal(visualize_label_heatmap(m, cfg, rev, output_dir=str(tmp_path)), _reference_heatmap(m, cfg, rev, "vit_som")[0])
    with pytest.raises(ValueError, match="outside"):
        visualize_label_heatmap(m, cfg, [(batches[0][0], batches[0][1] - 1)], output_dir=str(tmp_path))


def test_visualize_label_heatmap_desom(tmp_path):
    import vit_som_amd
    from vit_som_amd.evaluation import visualize_label_heatmap
    z, cfg = load_golden("ref_desom_tiny")
    m = vit_som_amd.DESOM(copy.deepcopy(cfg), device=DEV)
    m.load_state_dict(golden_params(z))
    batches = _batches(cfg)
    ref, _ = _reference_heatmap(m, cfg, batches, "desom")
    got = visualize_label_heatmap(m, cfg, batches, output_dir=str(tmp_path))
    assert got.shape == tuple(m.som_layer.map_size) and np.array_equal(got, ref)
    if _have_matplotlib():
        assert os.path.getsize(tmp_path / "desom_epoch_0_label_heatmap.png") > 0


def _dp_worker(rank, world, port, out):
    import torch.distributed as dist
    from vit_som_amd.evaluation import visualize_label_heatmap
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    m, cfg, _ = _vitsom()
    m.world_size, m.rank = world, rank
    mine = [b for i, b in enumerate(_batches(cfg)) if i % world == rank]
    heat = visualize_label_heatmap(m, cfg, mine, output_dir=f"{out}_plots")
    np.save(f"{out}.{rank}.npy", heat)
    dist.barrier()
    dist.destroy_process_group()


def test_visualize_label_heatmap_two_ranks(tmp_path):
    from test_distributed import _free_port
    from vit_som_amd.evaluation import visualize_label_heatmap
    out = str(tmp_path / "hm")
    mp.spawn(_dp_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    r0, r1 = np.load(f"{out}.0.npy"), np.load(f"{out}.1.npy")
    assert np.array_equal(r0, r1)
    m, cfg, _ = _vitsom()
    batches = _batches(cfg)
    order = [b for i, b in enumerate(batches) if i % 2 == 0] + [b for i, b in enumerate(batches) if i % 2 == 1]
    single = visualize_label_heatmap(m, cfg, order, output_dir=str(tmp_path / "single"))
    assert np.array_equal(r0, single)
    assert np.array_equal(single, _reference_heatmap(m, cfg, order, "vit_som")[0])


# ------------------------------------------------------------------ the epoch in the file names
def test_fit_sets_current_epoch(tmp_path):
    import vit_som_amd
    from vit_som_amd.evaluation import visualize_decoded_prototypes, visualize_label_heatmap
    from vit_som_amd.train import fit, synthetic_loaders
    _, cfg = load_golden("ref_cluster_tiny")
    cfg = copy.deepcopy(cfg)
    cfg["hyperparameters"]["batch_size"] = 16
    m = vit_som_amd.ViTSOM(copy.deepcopy(cfg), device=DEV)
    assert m.current_epoch == 0
    train, val, test = synthetic_loaders(cfg, n_train=64, n_val=16, n_test=16)
    os.makedirs(tmp_path / "ck")
    fit(m, cfg, train, val, str(tmp_path / "ck"), "synthetic", False, max_epochs=3, log=lambda s: None)
    assert m.current_epoch == 2
    visualize_decoded_prototypes(m, cfg, output_dir=str(tmp_path))
    visualize_label_heatmap(m, cfg, test, output_dir=str(tmp_path))
    if _have_matplotlib():
        assert os.path.exists(tmp_path / "vit_som_epoch_2_decoded_prototypes.png")
        assert os.path.exists(tmp_path / "vit_som_epoch_2_label_heatmap.png")
