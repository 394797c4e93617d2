"""The device data pipeline on the MI355X: vsom_augment_batch against PIL's bytes (tests/golden/pil_bicubic_crops.npz, made
by tools/gen_pil_crops.py), normalisation bitwise against torch, vsom_augment_plan against its numpy restatement, random
erasing, independence of an image from batch size / position / rank count, the two-batch ring, and the train driver fed by
DeviceLoader."""
import copy
import math
import os
import signal

import numpy as np
import pytest
import torch

import data_ref as R
from helpers import load_golden
from test_data_cpu import fixture_groups

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CIFAR_MEAN, CIFAR_STD = (0.4914, 0.4822, 0.4465), (0.2023, 0.1994, 0.2010)


@pytest.fixture(autouse=True)
def time_limit(request):
    """A limit of its own (seconds) for every test here.  It is a SIGALRM handler, and Python runs those between bytecodes
    only: it ends a test whose host side is slow or loops, not one stuck inside a device call -- that case is bounded by
    the `timeout` the suite runs under on the GPU machine, as for every other GPU test of the project."""
    limit = 300 if "driver" in request.node.name else 120

    def expired(signum, frame):
        raise TimeoutError(f"{request.node.name}: no result after {limit} s")
    old = signal.signal(signal.SIGALRM, expired)
    signal.alarm(limit)
    yield
    signal.alarm(0)
    signal.signal(signal.SIGALRM, old)


def run_batch(src, index, params, S, Rr, off, mean=None, std=None, seed=0, epoch=0):
    """(fp32 output, 8-bit image) of one vsom_augment_batch launch; numpy in, torch (device) out."""
    from vit_som_amd import ops
    src = torch.as_tensor(src).to(DEV)
    C, B = src.shape[1], len(index)
    mean = torch.tensor(mean if mean is not None else (0.0,) * C, dtype=torch.float32, device=DEV)
    std = torch.tensor(std if std is not None else (1.0,) * C, dtype=torch.float32, device=DEV)
    out = torch.full((B, C, S, S), float("nan"), device=DEV)
    out8 = torch.full((B, C, S, S), 77, dtype=torch.uint8, device=DEV)
    p = None if params is None else torch.as_tensor(params).to(DEV).contiguous()
    ops.augment_batch(src, torch.as_tensor(index).to(DEV), p, out, S, Rr, off, mean, std, seed, epoch, out_u8=out8)
    torch.cuda.synchronize()
    return out, out8


def torch_normalise(u8, mean, std):
    """ToTensor + Normalize in their operation order, every operand a device tensor: torch divides by a Python scalar
    through its reciprocal, by a tensor with a true division."""
    C = u8.shape[1]
    m = torch.tensor(mean, dtype=torch.float32, device=u8.device).view(1, C, 1, 1)
    s = torch.tensor(std, dtype=torch.float32, device=u8.device).view(1, C, 1, 1)
    return (u8.float() / torch.tensor(255.0, device=u8.device) - m) / s


# ------------------------------------------------------------------ 6. resampling is exact
GROUPS = dict(fixture_groups())


@pytest.mark.parametrize("k", sorted(GROUPS))
def test_resampling_equals_pil_bytes(k):
    src, index, params, geom, want = GROUPS[k]
    S, Rr, off, use = (int(v) for v in geom)
    out, out8 = run_batch(src, index, params if use else None, S, Rr, off)
    diff = int((out8.cpu().numpy() != want).sum())
    print(f"group {k}: C={src.shape[1]} H={src.shape[2]} S={S} R={Rr} off={off}: {len(index)} cases, {diff} of {want.size} bytes differ")
    assert diff == 0
    assert torch.equal(out, out8.float() / torch.tensor(255.0, device=DEV))                       # mean 0, std 1
    if use:
        flipped = params.copy()
        flipped[:, 8] = 1
        _, f8 = run_batch(src, index, flipped, S, Rr, off)
        assert np.array_equal(f8.cpu().numpy(), np.flip(want, axis=-1))


def test_size_not_a_multiple_of_four_against_restatement():
    """S = 30 takes the kernel's scalar store path; PIL is pinned by the restatement (test_data_cpu.py)."""
    rng = np.random.default_rng(3)
    src = rng.integers(0, 256, (4, 3, 32, 32), dtype=np.uint8)
    index = np.array([3, 0, 2, 1, 1, 3], np.int64)
    params, _ = R.plan(index, 0, 11, H=32, S=30, scale=(0.08, 1.0), ratio=(0.75, 1.3333), two_stage=True, flip_p=0.5, erase_p=0.0)
    out, out8 = run_batch(src, index, params, 30, 30, 0, CIFAR_MEAN, CIFAR_STD)
    want = np.stack([R.transform_u8(src[i], p, 30, 30, 0) for i, p in zip(index, params)])
    assert np.array_equal(out8.cpu().numpy(), want)
    assert torch.equal(out, torch_normalise(out8, CIFAR_MEAN, CIFAR_STD))


# ------------------------------------------------------------------ 7. normalisation
@pytest.mark.parametrize("k,mean,std", [(1, CIFAR_MEAN, CIFAR_STD), (3, (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)),
                                        (0, (0.5,), (0.5,)), (5, CIFAR_MEAN, CIFAR_STD), (6, (0.0,), (1.0,))])
def test_normalisation_is_bitwise_torch(k, mean, std):
    src, index, params, geom, want = GROUPS[k]
    S, Rr, off, use = (int(v) for v in geom)
    out, out8 = run_batch(src, index, params if use else None, S, Rr, off, mean, std)
    assert np.array_equal(out8.cpu().numpy(), want)
    ref = torch_normalise(out8, mean, std)
    print(f"group {k}: {int((out != ref).sum())} of {out.numel()} floats differ, max |diff| {float((out - ref).abs().max()):.3g}")
    assert torch.equal(out, ref)
    # every level 0..255 of every channel
    lv = np.tile(np.arange(256, dtype=np.uint8).reshape(1, 1, 16, 16), (1, len(mean), 1, 1))
    out, out8 = run_batch(lv, np.zeros(1, np.int64), None, 16, 16, 0, mean, std)
    assert np.array_equal(out8.cpu().numpy(), lv) and torch.equal(out, torch_normalise(out8, mean, std))


# ------------------------------------------------------------------ 8. the plan
@pytest.mark.parametrize("case", range(3))
def test_plan_equals_restatement(case):
    """Identical integers for every sample: the restatement meets no rounding boundary within 1e-9 for these seeds
    (test_data_cpu.py::test_plan_cases_of_the_gpu_test_meet_no_rounding_boundary inspects all 6 144 samples)."""
    from vit_som_amd import ops
    seed, epoch, index, kw = list(R.gpu_plan_cases())[case]
    want, margin = R.plan(index, epoch, seed, **kw)
    assert margin.min() > 1e-9
    params = torch.full((len(index), ops.AUGMENT_PARAMS), -5, dtype=torch.int32, device=DEV)
    lr = (math.log(kw["ratio"][0]), math.log(kw["ratio"][1]))
    lr2 = (math.log(R.TIMM_RATIO[0]), math.log(R.TIMM_RATIO[1]))
    ops.augment_plan(torch.as_tensor(index).to(DEV), params, int(index.max()) + 1, kw["H"], kw["S"], kw["scale"], lr,
                     R.TIMM_SCALE if kw["two_stage"] else None, lr2, kw["flip_p"], kw["erase_p"], seed, epoch)
    got = params.cpu().numpy()
    bad = np.flatnonzero((got != want).any(1))
    print(f"case {case}: {len(bad)} of {len(index)} samples differ; smallest rounding margin {margin.min():.3g}")
    assert len(bad) == 0, (bad[:5], got[bad[:2]], want[bad[:2]])


# ------------------------------------------------------------------ 9. random erasing
def test_erase_noise():
    """Outside the box nothing changes, inside every element is a fresh N(0, 1) draw, one per channel.
    Two channels of a pixel CAN hold the same fp32 value by chance: measured on the device over 51 M erased pixels the
    rate is about 1e-7 per pixel (about twice what the spacing of fp32 values under a normal density gives), so about
    0.07 such pixels are expected among the 737 k this test erases.  The assertion is exact all the same."""
    from vit_som_amd import ops
    n, S, C = 4096, 32, 3
    g = torch.Generator().manual_seed(1)
    src = torch.randint(0, 256, (n, C, S, S), dtype=torch.uint8, generator=g).to(DEV)
    index = torch.randperm(n, generator=g).to(DEV)
    params = torch.zeros(n, ops.AUGMENT_PARAMS, dtype=torch.int32, device=DEV)
    lr = (math.log(0.75), math.log(1.3333))
    ops.augment_plan(index, params, n, S, S, (0.08, 1.0), lr, R.TIMM_SCALE, (math.log(0.75), math.log(4 / 3)), 0.5, 1.0, 9, 4)
    plain = params.clone()
    plain[:, 9:13] = 0
    mean = torch.tensor(CIFAR_MEAN, device=DEV)
    std = torch.tensor(CIFAR_STD, device=DEV)
    erased, clean = torch.empty(n, C, S, S, device=DEV), torch.empty(n, C, S, S, device=DEV)
    ops.augment_batch(src, index, params, erased, S, S, 0, mean, std, 9, 4)
    ops.augment_batch(src, index, plain, clean, S, S, 0, mean, std, 9, 4)
    p = params.cpu().numpy()
    assert (p[:, 11] > 0).all() and (p[:, 12] > 0).all()                   # erase_p = 1: every sample has a box
    yy = torch.arange(S, device=DEV).view(1, S, 1)
    xx = torch.arange(S, device=DEV).view(1, 1, S)
    t, l, h, w = (params[:, c].view(n, 1, 1) for c in (9, 10, 11, 12))
    box = ((yy >= t) & (yy < t + h) & (xx >= l) & (xx < l + w)).view(n, 1, S, S).expand(n, C, S, S)
    assert torch.equal(erased[~box], clean[~box])                           # outside: bitwise the un-erased output
    assert bool((erased[box] != clean[box]).all())                          # inside: every element replaced
    noise = erased[box].double()
    m = noise.numel()
    # m independent N(0, 1) draws: the mean has standard deviation 1 / sqrt(m), the sample variance sqrt(2 / m); 3.5 of
    # each (two-sided tail 4.7e-4).  The 24-bit uniforms of the Box-Muller step cut the tails at 5.8: a variance loss
    # below 1e-5, far inside the band for any m this test can reach.
    mu, var = float(noise.mean()), float(noise.var())
    print(f"{m} erased elements: mean {mu:.3g} (band {3.5 / math.sqrt(m):.3g}), variance {var:.6f} (band {3.5 * math.sqrt(2 / m):.3g})")
    assert m > 500000
    assert abs(mu) <= 3.5 / math.sqrt(m) and abs(var - 1.0) <= 3.5 * math.sqrt(2.0 / m)
    # pixel mode: a draw per channel, not one value per pixel or per box
    pix = box[:, 0]
    e0, e1, e2 = erased[:, 0][pix], erased[:, 1][pix], erased[:, 2][pix]
    assert not bool(((e0 == e1) | (e1 == e2) | (e0 == e2)).any())
    # the noise of an image depends on its dataset index and the epoch, not on its row in the batch
    again = torch.empty(8, C, S, S, device=DEV)
    ops.augment_batch(src, index[100:108].contiguous(), params[100:108].contiguous(), again, S, S, 0, mean, std, 9, 4)
    assert torch.equal(again, erased[100:108])
    ops.augment_batch(src, index[100:108].contiguous(), params[100:108].contiguous(), again, S, S, 0, mean, std, 9, 5)
    assert not torch.equal(again, erased[100:108])


# ------------------------------------------------------------------ 10. independence from batching
def _epoch_images(ds, tr, bs, rank, world, epoch, seed=3):
    from vit_som_amd.data import DeviceLoader
    dl = DeviceLoader(ds, bs, tr, shuffle=True, rank=rank, world_size=world, seed=seed)
    dl.set_epoch(epoch)
    got = {}
    for x, y in dl:
        x, y = x.cpu(), y.cpu()
        for b in range(len(y)):
            assert int(y[b]) not in got
            got[int(y[b])] = x[b].clone()
    return got


def test_image_depends_on_index_and_epoch_only():
    from vit_som_amd.data import DeviceDataset, DeviceTransform
    n = 1024
    g = torch.Generator().manual_seed(2)
    ds = DeviceDataset(torch.randint(0, 256, (n, 3, 32, 32), dtype=torch.uint8, generator=g), torch.arange(n), DEV)   # label = index
    tr = DeviceTransform(True, 3, 32, CIFAR_MEAN, CIFAR_STD)
    for epoch in (0, 1):
        a = _epoch_images(ds, tr, 64, 0, 1, epoch)
        b = _epoch_images(ds, tr, 512, 0, 1, epoch)
        assert sorted(a) == sorted(b) == list(range(n))
        assert all(torch.equal(a[k], b[k]) for k in a)                      # batch size 64 and 512
        r0, r1 = _epoch_images(ds, tr, 64, 0, 2, epoch), _epoch_images(ds, tr, 64, 1, 2, epoch)
        assert not set(r0) & set(r1) and sorted(set(r0) | set(r1)) == list(range(n))
        assert all(torch.equal(a[k], v) for k, v in {**r0, **r1}.items())   # two ranks: other batches, other positions
        again = _epoch_images(ds, tr, 64, 0, 1, epoch)
        assert all(torch.equal(a[k], again[k]) for k in a)                  # two runs
        if epoch == 0:
            first = a
    changed = sum(not torch.equal(first[k], a[k]) for k in a)
    assert changed > n * 0.99                                               # another epoch, another augmentation
    other = _epoch_images(ds, tr, 64, 0, 1, 1, seed=4)
    assert sum(not torch.equal(other[k], a[k]) for k in a) > n * 0.99      # another seed


# ------------------------------------------------------------------ 12. the ring
def test_ring_keeps_the_previous_batch_and_allocates_nothing():
    from vit_som_amd.data import DeviceDataset, DeviceLoader, DeviceTransform
    n = 64 * 12 + 7
    g = torch.Generator().manual_seed(5)
    ds = DeviceDataset(torch.randint(0, 256, (n, 3, 32, 32), dtype=torch.uint8, generator=g), torch.arange(n) % 10, DEV)
    dl = DeviceLoader(ds, 64, DeviceTransform(True, 3, 32, CIFAR_MEAN, CIFAR_STD), shuffle=True, seed=1)
    assert len(dl) == 13
    order = list(DeviceLoader(ds, 64, dl.transform, shuffle=True, seed=1).index_batches())
    labels = ds.labels.cpu()
    keep_x, keep_y = torch.empty(64, 3, 32, 32, device=DEV), torch.empty(64, dtype=torch.int64, device=DEV)
    prev, mem, seen = None, None, 0
    for t, (x, y) in enumerate(dl):
        torch.cuda.synchronize()
        b = x.shape[0]
        assert x.dtype == torch.float32 and y.dtype == torch.int64 and x.is_cuda and y.is_cuda and x.data_ptr() % 16 == 0
        assert torch.equal(y.cpu(), labels[order[t]])
        if prev is not None:                                                # batch t - 1, after batch t has been produced
            assert torch.equal(prev[0], keep_x[:prev[2]]) and torch.equal(prev[1], keep_y[:prev[2]])
            assert x.data_ptr() != prev[0].data_ptr() and y.data_ptr() != prev[1].data_ptr()
        if t == 1:
            mem = torch.cuda.memory_allocated()
        if 1 <= t <= 9:                                                     # between the second and the tenth batch
            assert torch.cuda.memory_allocated() == mem, (t, torch.cuda.memory_allocated(), mem)
        keep_x[:b].copy_(x)
        keep_y[:b].copy_(y)
        prev = (x, y, b)
        seen += b
    assert seen == n and b == 7 and bool(torch.isfinite(x).all())           # the short last batch is a view of the ring too


# ------------------------------------------------------------------ 11. end to end
@pytest.mark.parametrize("name", ["ref_cls_tiny", "ref_cluster_tiny"])
def test_driver_trains_on_device_loaders(name, tmp_path):
    from vit_som_amd.data import DeviceLoader
    from vit_som_amd.train import device_loaders, main
    _, cfg = load_golden(name)
    cfg = copy.deepcopy(cfg)
    cfg["hyperparameters"]["batch_size"] = 32
    logs, made = [], []

    def loaders(c, r, w):
        made.append(device_loaders(c, r, w, n_train=256, n_val=64, n_test=64))
        return made[-1]
    with pytest.warns(UserWarning, match="RandAugment"):
        met = main(cfg, n_runs=1, max_epochs=2, make_loaders=loaders, model_states_dir=str(tmp_path / "states"), log=logs.append)
    assert all(isinstance(l, DeviceLoader) for l in made[0])
    losses = [float(l.split("train/total_loss=")[1].split()[0]) for l in logs if "train/total_loss=" in l]
    assert len(losses) == 2 and all(math.isfinite(v) for v in losses)
    assert made[0][0].epoch >= 2
    if cfg["data"]["num_classes"] > 0:
        assert os.path.exists(tmp_path / "states" / "vit_som_synthetic_best.ckpt")
        assert len(met["accuracy"]) == 1 and 0.0 <= met["accuracy"][0] <= 1.0 and math.isfinite(met["f1"][0])
    else:
        assert os.path.exists(tmp_path / "states" / "last.ckpt")
        assert 0.0 < met["purity"][0] <= 1.0 and 0.0 <= met["nmi"][0] <= 1.0


def test_device_loaders_from_npz(tmp_path):
    """--data-npz: images [N, H, W, C] / labels from a local file; without test arrays the last tenth is held out."""
    from vit_som_amd.train import device_loaders
    _, cfg = load_golden("ref_cls_tiny")
    cfg = copy.deepcopy(cfg)
    cfg["hyperparameters"]["batch_size"] = 16
    cfg["data"]["augment"] = {"randaug_n": 0, "autoaugment": False, "reprob": 0.0, "horizontal_flip": 0.5,
                              "resize_scale": [1.0, 1.0], "resize_ratio": [1.0, 1.0]}
    C, S = cfg["data"]["num_channels"], cfg["data"]["input_size"]
    rng = np.random.default_rng(0)
    images = rng.integers(0, 256, (100, S, S, C), dtype=np.uint8)
    labels = np.arange(100) % 5
    np.savez(tmp_path / "set.npz", images=images, labels=labels)
    train, val, test = device_loaders(cfg, npz=str(tmp_path / "set.npz"), strict=True)
    assert len(train.dataset) == 90 and len(val.dataset) == len(test.dataset) == 10 and len(train) == 5 and len(test) == 1
    x, y = next(iter(test))
    assert tuple(x.shape) == (10, C, S, S) and y.tolist() == labels[90:].tolist()
    # the evaluation transform of the held-out rows, against the restatement and torch
    t = test.transform
    want = np.stack([R.transform_u8(np.ascontiguousarray(im.transpose(2, 0, 1)), None, S, t.R, t.off) for im in images[90:]])
    assert torch.equal(x, torch_normalise(torch.from_numpy(want).to(DEV), t.mean, t.std))
    np.savez(tmp_path / "both.npz", images=images, labels=labels, test_images=images[:7], test_labels=labels[:7])
    train, val, test = device_loaders(cfg, npz=str(tmp_path / "both.npz"), strict=True)
    assert len(train.dataset) == 100 and len(test.dataset) == 7


# ------------------------------------------------------------------ labels outlive the ring
def test_labels_collected_over_a_loader_are_not_overwritten():
    """A consumer may keep every y of a loader and concatenate afterwards (evaluate_kmeans, visualize_umap_progression do):
    six batches through the two-slot ring, labels = dataset indices."""
    from vit_som_amd.data import DeviceDataset, DeviceLoader, DeviceTransform
    n = 16 * 6 - 3
    g = torch.Generator().manual_seed(8)
    ds = DeviceDataset(torch.randint(0, 256, (n, 1, 8, 8), dtype=torch.uint8, generator=g), torch.arange(n), DEV)
    for train in (True, False):
        tr = DeviceTransform(train, 1, 8, (0.5,), (0.5,))
        dl = DeviceLoader(ds, 16, tr, shuffle=train, seed=2)
        want = torch.cat(list(DeviceLoader(ds, 16, tr, shuffle=train, seed=2).index_batches()))
        kept = [y.reshape(-1).long() for _, y in dl]                        # no-ops on an int64 device tensor: aliases if y were a view
        torch.cuda.synchronize()
        assert len(kept) == 6 and torch.equal(torch.cat(kept).cpu(), want)


def test_evaluate_kmeans_and_umap_accept_a_device_loader(tmp_path):
    """Same batches through the DeviceLoader and as a list of clones: same purity / NMI, same UMAP labels."""
    import vit_som_amd
    from vit_som_amd.data import DeviceDataset, DeviceLoader, DeviceTransform
    from vit_som_amd.evaluation import evaluate_kmeans, visualize_umap_progression
    _, cfg = load_golden("ref_cluster_tiny")
    cfg = copy.deepcopy(cfg)
    C, S = cfg["data"]["num_channels"], cfg["data"]["input_size"]
    n, ncls = 16 * 6, 4
    g = torch.Generator().manual_seed(3)
    labels = torch.randint(0, ncls, (n,), generator=g)
    templates = torch.randint(0, 256, (ncls, C, S, S), generator=g)
    images = (templates[labels] + torch.randint(-20, 21, (n, C, S, S), generator=g)).clamp_(0, 255).to(torch.uint8)
    ds = DeviceDataset(images, labels, DEV)
    dl = DeviceLoader(ds, 16, DeviceTransform.from_config(cfg, False))
    clones = [(x.clone(), y.clone()) for x, y in dl]
    assert torch.equal(torch.cat([y for _, y in clones]).cpu(), labels)
    torch.manual_seed(0)
    model = vit_som_amd.ViTSOM(cfg, device=DEV)
    p0, n0, _ = evaluate_kmeans(model, cfg, clones)
    p1, n1, _ = evaluate_kmeans(model, cfg, dl)
    assert (p1, n1) == (p0, n0) and 0.0 < p1 <= 1.0
    _, y0 = visualize_umap_progression(model, cfg, clones, output_dir=str(tmp_path / "a"))
    _, y1 = visualize_umap_progression(model, cfg, dl, output_dir=str(tmp_path / "b"))
    assert np.array_equal(y1, y0) and np.array_equal(y1, labels.numpy())
