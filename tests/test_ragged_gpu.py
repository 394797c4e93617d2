"""The variable-size data pipeline on the MI355X: vsom_augment_batch_ragged against PIL's bytes
(tests/golden/pil_ragged_crops.npz, made by tools/gen_pil_ragged.py), bit-for-bit equality with the fixed-size entries on
sets of one shape, seeded random rectangles against the numpy restatement, independence of an image from batch size /
position / rank count, index clamping, and the train driver fed by a DeviceLoader over a ragged set."""
import copy
import math
import signal

import numpy as np
import pytest
import torch
import yaml

import data_ref as R
import ragged_ref as G
from test_ragged_cpu import FLOWERS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


@pytest.fixture(autouse=True)
def time_limit(request):
    """A limit of its own for every test here (a SIGALRM handler: it ends a slow host side, see tests/test_data_gpu.py)."""
    def expired(signum, frame):
        raise TimeoutError(f"{request.node.name}: no result after 120 s")
    old = signal.signal(signal.SIGALRM, expired)
    signal.alarm(120)
    yield
    signal.alarm(0)
    signal.signal(signal.SIGALRM, old)


def ragged_set(images, labels=None):
    from vit_som_amd.data import RaggedDeviceDataset
    return RaggedDeviceDataset.from_arrays(images, np.arange(len(images)) if labels is None else labels, DEV, layout="CHW")


def run_ragged(ds, index, params, S, Rr, mean=None, std=None, seed=0, epoch=0):
    """(fp32 output, 8-bit image) of one vsom_augment_batch_ragged call; params None: the evaluation transform."""
    from vit_som_amd import ops
    C, B = ds.C, len(index)
    mean = torch.tensor(mean if mean is not None else (0.0,) * C, dtype=torch.float32, device=DEV)
    std = torch.tensor(std if std is not None else (1.0,) * C, dtype=torch.float32, device=DEV)
    out = torch.full((B, C, S, S), float("nan"), device=DEV)
    out8 = torch.full((B, C, S, S), 77, dtype=torch.uint8, device=DEV)
    p = None if params is None else torch.as_tensor(params).to(DEV).contiguous()
    scratch = None if params is None else torch.full((ops.augment_ragged_scratch_bytes(B, C, S),), 99, dtype=torch.uint8, device=DEV)
    ops.augment_batch_ragged(ds.data, ds.offsets, ds.shapes, ds.C, ds.max_h, ds.max_w, torch.as_tensor(index).to(DEV), p, out, S, Rr,
                             mean, std, seed, epoch, scratch=scratch, out_u8=out8)
    torch.cuda.synchronize()
    return out, out8


# ------------------------------------------------------------------ 1. every golden case, byte for byte
def golden_groups():
    """One launch per (channels, S, R, training / evaluation): one- and two-crop rows share a launch."""
    groups = {}
    for row, out in G.golden_cases():
        c = dict(zip(G.COLS, (int(v) for v in row)))
        groups.setdefault((c["c"], c["S"], c["R"], c["mode"] == G.EVAL), []).append((row, out))
    return groups


GROUPS = golden_groups()


@pytest.mark.parametrize("key", sorted(GROUPS), ids=lambda k: f"C{k[0]}-S{k[1]}-R{k[2]}-{'eval' if k[3] else 'train'}")
def test_golden_cases_equal_pil_bytes(key):
    C, S, Rr, is_eval = key
    rows = [row for row, _ in GROUPS[key]]
    want = np.stack([out for _, out in GROUPS[key]])
    ds = ragged_set([G.formula_image(int(r[0]), int(r[1]), int(r[2]), int(r[3])) for r in rows])
    index = np.arange(len(rows), dtype=np.int64)
    params = None if is_eval else G.params_of(rows)
    out, out8 = run_ragged(ds, index, params, S, Rr)
    got = out8.cpu().numpy()
    for b, row in enumerate(rows):
        print(f"case {row.tolist()}: {int((got[b] != want[b]).sum())} of {want[b].size} bytes differ")
    assert np.array_equal(got, want)
    assert torch.equal(out, out8.float() / torch.tensor(255.0, device=DEV))                       # mean 0, std 1
    if not is_eval:
        params[:, 8] = 1
        _, f8 = run_ragged(ds, index, params, S, Rr)
        assert np.array_equal(f8.cpu().numpy(), np.flip(want, axis=-1))


def test_golden_groups_cover_all_three_paths():
    modes = {int(row[4]) for rows in GROUPS.values() for row, _ in rows}
    assert modes == {G.ONE_CROP, G.TWO_CROPS, G.EVAL} and sum(len(v) for v in GROUPS.values()) >= 40


# ------------------------------------------------------------------ 2. a set of one shape: the fixed-size entries, bit for bit
@pytest.mark.parametrize("C,H,mean,std", [(3, 32, IMAGENET_MEAN, IMAGENET_STD), (1, 28, (0.5,), (0.5,))])
def test_uniform_shapes_equal_the_fixed_size_entries(C, H, mean, std):
    from vit_som_amd import ops
    N, B, S, seed, epoch = 96, 64, H, 20240611, 3
    g = torch.Generator().manual_seed(C)
    images = torch.randint(0, 256, (N, C, H, H), dtype=torch.uint8, generator=g)
    ds = ragged_set(list(images.numpy()))
    assert ds.shapes.tolist() == [[H, H]] * N
    src = images.to(DEV)
    index = torch.randint(0, N, (B,), generator=g).to(DEV)
    args = (S, (0.08, 1.0), (math.log(0.75), math.log(1.3333)), R.TIMM_SCALE, (math.log(R.TIMM_RATIO[0]), math.log(R.TIMM_RATIO[1])),
            0.5, 0.6, seed, epoch)
    p_fixed = ops.augment_plan(index, torch.zeros(B, 16, dtype=torch.int32, device=DEV), N, H, *args)
    p_ragged = ops.augment_plan_ragged(index, ds.shapes, torch.zeros(B, 16, dtype=torch.int32, device=DEV), *args)
    assert torch.equal(p_fixed, p_ragged)
    assert 0 < int(p_fixed[:, 8].sum()) < B and 0 < int((p_fixed[:, 11] > 0).sum()) < B          # flips and erasures both happen
    m, s = torch.tensor(mean, device=DEV), torch.tensor(std, device=DEV)
    want, want8 = torch.empty(B, C, S, S, device=DEV), torch.empty(B, C, S, S, dtype=torch.uint8, device=DEV)
    ops.augment_batch(src, index, p_fixed, want, S, S, 0, m, s, seed, epoch, out_u8=want8)
    got, got8 = run_ragged(ds, index.cpu(), p_ragged, S, S, mean, std, seed, epoch)
    assert torch.equal(got8, want8)
    assert torch.equal(got, want)                                                                  # the erase noise included
    # one crop only: the second pass takes the image as it is
    p_one = p_fixed.clone()
    p_one[:, 4:8] = 0
    ops.augment_batch(src, index, p_one, want, S, S, 0, m, s, seed, epoch, out_u8=want8)
    got, got8 = run_ragged(ds, index.cpu(), p_one, S, S, mean, std, seed, epoch)
    assert torch.equal(got8, want8) and torch.equal(got, want)
    # the evaluation geometry
    Rr = int(S / 0.875)
    off = int(round((Rr - S) / 2.0))
    ops.augment_batch(src, index, None, want, S, Rr, off, m, s, seed, epoch, out_u8=want8)
    got, got8 = run_ragged(ds, index.cpu(), None, S, Rr, mean, std, seed, epoch)
    assert torch.equal(got8, want8) and torch.equal(got, want)


# ------------------------------------------------------------------ 3. forty random rectangles against the restatement
def random_box(rng, h, w, S):
    """A box inside h x w whose sides are at most 8 S (the entry's limit holds for the whole image already)."""
    bh, bw = int(rng.integers(1, h + 1)), int(rng.integers(1, w + 1))
    return int(rng.integers(0, h - bh + 1)), int(rng.integers(0, w - bw + 1)), bh, bw


@pytest.mark.parametrize("S,C", [(7, 3), (30, 1), (32, 3), (56, 1)])
def test_random_rectangles_equal_the_restatement(S, C):
    rng = np.random.default_rng(1000 + S)
    top = min(200, 8 * S)
    sides = rng.integers(1, top + 1, (10, 2))
    sides[0] = (top, top)                                               # shrink by exactly 8 at S = 7
    sides[1] = (1, top)
    images = [G.formula_image(int(h), int(w), C, 2 * k) for k, (h, w) in enumerate(sides)]
    ds = ragged_set(images)
    index = rng.permutation(10).astype(np.int64)
    params = np.zeros((10, 16), np.int32)
    want = []
    for b, n in enumerate(index):
        h, w = (int(v) for v in sides[n])
        params[b, 0:4] = random_box(rng, h, w, S)
        if b % 2:
            params[b, 4:8] = random_box(rng, S, S, S)
        params[b, 8] = b % 3 == 0
        img = G.train_u8(images[n], params[b, 0:4], params[b, 4:8] if b % 2 else None, S)
        want.append(img[:, :, ::-1] if params[b, 8] else img)
    out, out8 = run_ragged(ds, index, params, S, S)
    got = out8.cpu().numpy()
    for b in range(10):
        print(f"S={S} image {sides[index[b]].tolist()} plan {params[b, :9].tolist()}: {int((got[b] != want[b]).sum())} bytes differ")
    assert np.array_equal(got, np.stack(want))
    assert torch.equal(out, out8.float() / torch.tensor(255.0, device=DEV))
    Rr = int(S / 0.875)
    _, ev8 = run_ragged(ds, index, None, S, Rr)
    want = np.stack([G.eval_u8(images[n], Rr, S) for n in index])
    assert np.array_equal(ev8.cpu().numpy(), want)


# ------------------------------------------------------------------ 4. a sample depends on (seed, epoch, index) alone
def mixed_set(n, lo, hi, C=3, seed=0):
    rng = np.random.default_rng(seed)
    sides = rng.integers(lo, hi + 1, (n, 2))
    return ragged_set([G.formula_image(int(h), int(w), C, k) for k, (h, w) in enumerate(sides)]), sides


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
    from vit_som_amd.data import DeviceTransform
    n = 192
    ds, _ = mixed_set(n, 8, 72)                                         # label = index
    tr = DeviceTransform(True, 3, 32, IMAGENET_MEAN, IMAGENET_STD, variable_size=True)
    a = _epoch_images(ds, tr, 16, 0, 1, 0)
    b = _epoch_images(ds, tr, 64, 0, 1, 0)
    assert sorted(a) == sorted(b) == list(range(n))
    assert all(torch.equal(a[k], b[k]) for k in a)                      # batch size 16 and 64
    r0, r1 = _epoch_images(ds, tr, 16, 0, 2, 0), _epoch_images(ds, tr, 16, 1, 2, 0)
    assert not set(r0) & set(r1) and sorted(set(r0) | set(r1)) == list(range(n))
    assert all(torch.equal(a[k], v) for k, v in {**r0, **r1}.items())   # two ranks: other batches, other positions
    assert all(bool(torch.isfinite(v).all()) for v in a.values())
    other = _epoch_images(ds, tr, 64, 0, 1, 1)
    assert sum(not torch.equal(other[k], a[k]) for k in a) > n * 0.95   # another epoch, another augmentation


# ------------------------------------------------------------------ 5. indices outside the set
def _clamped(ds, tr_args, index):
    from vit_som_amd import ops
    B, S = len(index), 32
    idx = torch.tensor(index, dtype=torch.int64, device=DEV)
    p = ops.augment_plan_ragged(idx, ds.shapes, torch.zeros(B, 16, dtype=torch.int32, device=DEV), S, *tr_args)
    out, out8 = run_ragged(ds, np.array(index, np.int64), p, S, S, IMAGENET_MEAN, IMAGENET_STD, tr_args[-2], tr_args[-1])
    ev, _ = run_ragged(ds, np.array(index, np.int64), None, S, 36, IMAGENET_MEAN, IMAGENET_STD)
    return p, out, out8, ev


def test_out_of_range_indices_are_clamped():
    N = 12
    ds, _ = mixed_set(N, 20, 60, seed=5)
    args = ((0.08, 1.0), (math.log(0.75), math.log(1.3333)), R.TIMM_SCALE, (math.log(R.TIMM_RATIO[0]), math.log(R.TIMM_RATIO[1])),
            0.5, 0.9, 77, 2)
    bad = _clamped(ds, args, [-1, N, -(1 << 40), 1 << 40, 5])
    good = _clamped(ds, args, [0, N - 1, 0, N - 1, 5])
    for got, want in zip(bad, good):
        assert torch.equal(got, want)
    assert int((good[0][:, 11] > 0).sum()) > 0                          # the noise is keyed by the clamped index too


# ------------------------------------------------------------------ 6. end to end
def tiny_flowers_config():
    with open([p for p in FLOWERS if "vit_som_flowers-17" in p][0]) as fh:
        cfg = yaml.safe_load(fh)
    hp = cfg["hyperparameters"]
    cfg["data"]["input_size"] = 32
    hp["batch_size"] = 16
    hp["som"]["map_size"] = [6, 6]
    hp["som"]["Tmax"] = 6
    hp["vit"].update(patch_size=8, emb_dim=48, depth=2, dec_emb_dim=24, dec_depth=1, heads=3)
    return cfg


def test_fit_runs_on_a_synthetic_ragged_set(tmp_path):
    import vit_som_amd
    from vit_som_amd.data import DeviceLoader, RaggedDeviceDataset
    from vit_som_amd.train import device_loaders, fit
    cfg = tiny_flowers_config()
    with pytest.warns(UserWarning, match="RandAugment"):
        train, val, test = device_loaders(cfg, n_train=32, n_val=16, n_test=16)
    assert all(isinstance(l, DeviceLoader) and isinstance(l.dataset, RaggedDeviceDataset) for l in (train, val, test))
    sides = train.dataset.shapes.cpu()
    assert int(sides.min()) >= 32 and int(sides.max()) <= 64 and len(set(map(tuple, sides.tolist()))) > 8
    assert len(train) == 2 and len(val) == 1 and train.transform.variable_size and val.transform.R == 36
    model = vit_som_amd.ViTSOM(copy.deepcopy(cfg), device=DEV)
    logs = []
    out = fit(model, cfg, train, val, str(tmp_path), "flowers-17", True, max_epochs=1, log=logs.append)
    torch.cuda.synchronize()
    rec = out["history"][0]
    assert math.isfinite(rec["train/total_loss"]) and math.isfinite(rec["val/total_loss"]) and 0.0 <= rec["val/accuracy"] <= 1.0
    assert int(model.iteration) == 2 and model._it == 2 and train.epoch == 1
    x, y = next(iter(test))
    assert tuple(x.shape) == (16, 3, 32, 32) and bool(torch.isfinite(x).all()) and y.dtype == torch.int64
    with pytest.raises(NotImplementedError, match="LDS"):
        device_loaders(cfg, n_train=16, n_val=16, n_test=16, auto_augment=True)


def test_device_loaders_from_a_ragged_npz(tmp_path):
    from vit_som_amd.data import RaggedDeviceDataset
    from vit_som_amd.train import device_loaders
    cfg = tiny_flowers_config()
    cfg["data"]["augment"].update(randaug_n=0, autoaugment=False)
    rng = np.random.default_rng(0)
    sides = rng.integers(20, 70, (50, 2))
    images = [G.formula_image(int(h), int(w), 3, k) for k, (h, w) in enumerate(sides)]
    labels = np.arange(50) % 17
    whole = RaggedDeviceDataset.from_arrays(images, labels, "cpu", layout="CHW")
    np.savez(tmp_path / "set.npz", **whole.to_npz_arrays())
    train, val, test = device_loaders(cfg, npz=str(tmp_path / "set.npz"), strict=True)
    assert len(train.dataset) == 45 and len(val.dataset) == len(test.dataset) == 5 and len(train) == 2 and len(test) == 1
    x, y = next(iter(test))
    assert tuple(x.shape) == (5, 3, 32, 32) and y.tolist() == labels[45:].tolist()
    # the evaluation transform of the held-out images, against the restatement
    t = test.transform
    want = torch.from_numpy(np.stack([G.eval_u8(im, t.R, 32) for im in images[45:]])).to(DEV)
    m, s = (torch.tensor(v, device=DEV).view(1, 3, 1, 1) for v in (t.mean, t.std))
    assert torch.equal(x, (want.float() / torch.tensor(255.0, device=DEV) - m) / s)
    held = RaggedDeviceDataset.from_arrays(images[:7], labels[:7], "cpu", layout="CHW")
    np.savez(tmp_path / "both.npz", **whole.to_npz_arrays(), **{k: v for k, v in held.to_npz_arrays("test_").items() if k != "channels"})
    train, val, test = device_loaders(cfg, npz=str(tmp_path / "both.npz"), strict=True)
    assert len(train.dataset) == 50 and len(test.dataset) == 7 and len(train) == 3
    xb, yb = next(iter(train))
    assert tuple(xb.shape) == (16, 3, 32, 32) and bool(torch.isfinite(xb).all())
