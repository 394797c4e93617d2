"""The device data pipeline without a GPU: the resampler restatement against PIL and the committed fixture, the plan's
formulas and frequencies, DeviceTransform.from_config on the reference's configs, DeviceLoader's order, argument checks."""
import glob
import math
import os

import numpy as np
import pytest
import torch
import yaml

import data_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CIFAR = dict(H=32, S=32, scale=(0.08, 1.0), ratio=(0.75, 1.3333), two_stage=True, flip_p=0.5, erase_p=0.25)


def fixture_groups():
    z = np.load(os.path.join(GOLDEN, "pil_bicubic_crops.npz"))
    k = 0
    while f"g{k}_src" in z:
        yield k, tuple(z[f"g{k}_{n}"] for n in ("src", "index", "params", "geom", "out"))
        k += 1


def test_resampler_restatement_equals_fixture():
    cases = 0
    for k, (src, index, params, geom, out) in fixture_groups():
        S, Rr, off, use = (int(v) for v in geom)
        for b in range(len(index)):
            got = R.transform_u8(src[index[b]], params[b] if use else None, S, Rr, off)
            assert np.array_equal(got, out[b]), f"group {k} case {b}: {(got != out[b]).sum()} bytes differ from PIL"
            cases += 1
    assert cases >= 150


def test_fixture_covers_the_edges():
    groups = dict(fixture_groups())
    assert len(groups) == 9
    shapes = {(g[0].shape[1], g[0].shape[2], int(g[3][0])) for g in groups.values()}
    assert {(1, 28, 28), (3, 32, 32), (3, 64, 32), (3, 64, 64)} <= shapes
    p = np.concatenate([g[2] for g in groups.values() if g[3][3]])
    assert (p[:, 3] == 1).any() and (p[:, 2] == 1).any() and (p[:, 2] != p[:, 3]).any() and (p[:, 6] > 0).sum() >= 40
    assert any(g[3][3] == 0 and tuple(g[3][:3]) == (32, 36, 2) for g in groups.values())       # evaluation: 32 -> 36 -> window
    assert os.path.getsize(os.path.join(GOLDEN, "pil_bicubic_crops.npz")) < (1 << 20)


def test_resampler_restatement_equals_pil_on_fresh_boxes():
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(7)
    for C, H, S in ((1, 28, 28), (3, 32, 32), (3, 64, 32), (3, 64, 64)):
        for t in range(25):
            src = rng.integers(0, 256, (C, H, H), dtype=np.uint8)
            u = rng.random(4)
            (i, j, h, w), _ = R.box_from_uniforms(u[0], u[1], u[2], u[3], H, H, (0.08, 1.0), (math.log(0.75), math.log(1.3333)))
            im = Image.fromarray(src[0]) if C == 1 else Image.fromarray(np.ascontiguousarray(src.transpose(1, 2, 0)))
            a = np.asarray(im.crop((j, i, j + w, i + h)).resize((S, S), Image.BICUBIC))
            a = a[None] if C == 1 else a.transpose(2, 0, 1)
            p = np.array([i, j, h, w] + [0] * 12, np.int32)
            assert np.array_equal(R.transform_u8(src, p, S, S, 0), a), (C, H, S, i, j, h, w)


def test_philox_known_answers():
    """Random123's known-answer vectors for philox4x32-10."""
    assert [int(v) for v in R.philox4x32_10(0, 0, 0, 0, 0, 0)] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    f = 0xffffffff
    assert [int(v) for v in R.philox4x32_10(f, f, f, f, f, f)] == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    assert [int(v) for v in R.philox4x32_10(0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344, 0xa4093822, 0x299f31d0)] == \
        [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]


def reference_get_params(ua, ur, ui, uj, height, width, scale, ratio):
    """tools/utils.py:93-113 line by line, the four random draws replaced by the given uniforms (randint(0, n) = floor(u n))."""
    area = height * width
    target_area = area * (scale[0] + ua * (scale[1] - scale[0]))
    log_ratio = (math.log(ratio[0]), math.log(ratio[1]))
    aspect_ratio = math.exp(log_ratio[0] + ur * (log_ratio[1] - log_ratio[0]))
    w = int(round(math.sqrt(target_area * aspect_ratio)))
    h = int(round(math.sqrt(target_area / aspect_ratio)))
    w = min(w, width)
    h = min(h, height)
    i = int(ui * (height - h + 1))
    j = int(uj * (width - w + 1))
    return i, j, h, w


def reference_erase(uniforms, img_h, img_w, min_area=0.02, max_area=1 / 3, min_aspect=0.3, count=1):
    """timm RandomErasing._erase's search for a box, as its source gives it, with random.uniform(a, b) = a + (b - a) u and
    random.randint(0, n) = floor(u (n + 1)) fed from `uniforms` (an iterator) -> (top, left, h, w) or None."""
    log_aspect_ratio = (math.log(min_aspect), math.log(1 / min_aspect))
    area = img_h * img_w
    for attempt in range(10):
        target_area = (min_area + (max_area - min_area) * next(uniforms)) * area / count
        aspect_ratio = math.exp(log_aspect_ratio[0] + (log_aspect_ratio[1] - log_aspect_ratio[0]) * next(uniforms))
        h = int(round(math.sqrt(target_area * aspect_ratio)))
        w = int(round(math.sqrt(target_area / aspect_ratio)))
        if w < img_w and h < img_h:
            top = int(next(uniforms) * (img_h - h + 1))
            left = int(next(uniforms) * (img_w - w + 1))
            return top, left, h, w
        next(uniforms), next(uniforms)               # the plan gives every attempt its own four uniforms
    return None


def test_plan_restatement_erase_box_equals_timm_formula():
    """The erase box of the plan against reference_erase fed the same uniforms (blocks 5 + 2a, 6 + 2a of a sample).  A
    sample whose unrounded h or w lies within 1e-9 of k + 1/2 is left out (the two write the products in another order);
    S = 32 and S = 8: at 8 some attempts are refused (h >= S) and later attempts are used."""
    for S, seed in ((32, 99), (8, 7)):
        n, epoch = 5000, 2
        index = np.arange(n)
        kw = dict(CIFAR, H=S, S=S, erase_p=1.0)
        p, margin = R.plan(index, epoch, seed, **kw)
        u = R.plan_uniforms(index, epoch, seed)
        compared = later = 0
        for s in range(n):
            if margin[s] <= 1e-9:
                continue
            want = reference_erase(iter(u[s, 5:].reshape(-1)), S, S)
            assert want is not None and tuple(p[s, 9:13]) == want, (s, p[s, 9:13], want)
            compared += 1
            later += tuple(p[s, 9:13]) != reference_first_attempt(u[s], S)
        assert compared >= n - 2 and (later > 0 if S == 8 else True)


def reference_first_attempt(us, S):
    """What attempt 0 alone would give (None when it is refused): tells whether a later attempt was used."""
    area = (S * S) * (0.02 + us[5, 0] * (1.0 / 3.0 - 0.02))
    ar = math.exp(math.log(0.3) + us[5, 1] * (math.log(1 / 0.3) - math.log(0.3)))
    h, w = int(round(math.sqrt(area * ar))), int(round(math.sqrt(area / ar)))
    return (int(us[6, 0] * (S - h + 1)), int(us[6, 1] * (S - w + 1)), h, w) if h < S and w < S else None


def test_plan_restatement_boxes_and_frequencies():
    n, epoch, seed = 10000, 2, 99
    index = np.arange(n)
    p, _ = R.plan(index, epoch, seed, **CIFAR)
    u = R.plan_uniforms(index, epoch, seed)
    S = H = 32
    for s in range(n):
        want = reference_get_params(u[s, 0, 0], u[s, 0, 1], u[s, 1, 0], u[s, 1, 1], H, H, CIFAR["scale"], CIFAR["ratio"])
        if want[2] >= 1 and want[3] >= 1:            # the reference leaves h, w >= 1 to chance; the plan clamps
            assert tuple(p[s, 0:4]) == want
        want = reference_get_params(u[s, 2, 0], u[s, 2, 1], u[s, 3, 0], u[s, 3, 1], S, S, R.TIMM_SCALE, R.TIMM_RATIO)
        if want[2] >= 1 and want[3] >= 1:
            assert tuple(p[s, 4:8]) == want
    for o, size in ((0, H), (4, S)):
        assert (p[:, o + 2] >= 1).all() and (p[:, o + 3] >= 1).all() and (p[:, o] >= 0).all() and (p[:, o + 1] >= 0).all()
        assert (p[:, o] + p[:, o + 2] <= size).all() and (p[:, o + 1] + p[:, o + 3] <= size).all()
    erased = p[:, 11] > 0
    assert (p[erased, 12] > 0).all() and (p[~erased, 9:13] == 0).all()
    assert (p[erased, 11] < S).all() and (p[erased, 12] < S).all() and (p[:, 9] >= 0).all() and (p[:, 10] >= 0).all()
    assert (p[:, 9] + p[:, 11] <= S).all() and (p[:, 10] + p[:, 12] <= S).all()
    # Frequencies.  A count of n Bernoulli(q) draws has standard deviation sqrt(n q (1 - q)); the band is 3.5 of them
    # (two-sided tail 4.7e-4 for a fair generator).  All ten erase attempts failing needs sqrt(A r) >= S ten times in a
    # row, each time with probability below 0.05: below 1e-13, so the erase count is Bernoulli(reprob) to that accuracy.
    for count, q in ((int(p[:, 8].sum()), CIFAR["flip_p"]), (int(erased.sum()), CIFAR["erase_p"])):
        assert abs(count - n * q) <= 3.5 * math.sqrt(n * q * (1 - q)), (count, n * q)
    # a sample's plan depends on (seed, epoch, index) and on nothing else
    q, _ = R.plan(index[5000:5010][::-1].copy(), epoch, seed, **CIFAR)
    assert np.array_equal(q[::-1], p[5000:5010])
    assert not np.array_equal(R.plan(index[:64], epoch + 1, seed, **CIFAR)[0], p[:64])
    assert not np.array_equal(R.plan(index[:64], epoch, seed + 1, **CIFAR)[0], p[:64])


def test_plan_cases_of_the_gpu_test_meet_no_rounding_boundary():
    """tests/test_data_gpu.py compares the device plan with the restatement for these (seed, epoch, index) and allows no
    exception; that is legitimate only if no unrounded h, w lies within 1e-9 of k + 1/2 here."""
    inspected = 0
    for seed, epoch, index, kw in R.gpu_plan_cases():
        _, margin = R.plan(index, epoch, seed, **kw)
        assert margin.min() > 1e-9, (seed, epoch, int(margin.argmin()), float(margin.min()))
        inspected += len(index)
    assert inspected >= 4000


def reference_build_transform(name, input_size, num_channels):
    """Mean / std / geometry as data/data.py:270-313 chooses them."""
    if name in ("mnist", "fmnist", "usps"):
        return (0.0,) * num_channels, (1.0,) * num_channels, input_size, 0
    if num_channels == 1:
        mean, std = (0.5,), (0.5,)
    elif name in ("cifar-10", "cifar-100"):
        mean, std = (0.4914, 0.4822, 0.4465), (0.2023, 0.1994, 0.2010)
    elif name in ("medmnist",):
        mean, std = (0.5, 0.5, 0.5), (0.5, 0.5, 0.5)
    else:
        mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    size = int(input_size / (0.875 if input_size <= 224 else 1.0))
    return mean, std, size, int(round((size - input_size) / 2.0))


CONFIGS = sorted(glob.glob(os.path.join(GOLDEN, "config_vit*.yaml")))


def test_config_fixtures_present():
    assert len(CONFIGS) == 17


@pytest.mark.parametrize("path", CONFIGS, ids=[os.path.basename(p)[7:-5] for p in CONFIGS])
def test_transform_from_config(path):
    from vit_som_amd.data import DeviceTransform
    with open(path) as fh:
        cfg = yaml.safe_load(fh)
    d = cfg["data"]
    name, S, C, a = d["dataset"], d["input_size"], d["num_channels"], d["augment"]
    if name.startswith("flowers"):
        with pytest.raises(ValueError, match="fixed-size"):
            DeviceTransform.from_config(cfg, True)
        return
    mean, std, size, off = reference_build_transform(name, S, C)
    plain = name in ("mnist", "fmnist", "usps")
    if plain:
        tr = DeviceTransform.from_config(cfg, True, strict=True)           # nothing to refuse: ToTensor() alone
    else:
        with pytest.warns(UserWarning, match="RandAugment"):
            tr = DeviceTransform.from_config(cfg, True)
        with pytest.raises(NotImplementedError, match="RandAugment"):
            DeviceTransform.from_config(cfg, True, strict=True)
    ev = DeviceTransform.from_config(cfg, False, strict=True)
    for t in (tr, ev):
        assert (t.C, t.S) == (C, S) and t.mean == tuple(mean) and t.std == tuple(std)
    assert (tr.R, tr.off, tr.augment) == (S, 0, not plain)
    assert (ev.R, ev.off, ev.augment) == (size, off, False)
    if not plain:
        assert tr.scale == tuple(a["resize_scale"]) and tr.ratio == tuple(a["resize_ratio"]) and tr.two_stage
        p1 = a["horizontal_flip"]
        assert tr.flip_p == pytest.approx(p1 * 0.5 + 0.5 * (1 - p1)) and tr.erase_p == a["reprob"]


@pytest.mark.parametrize("world", [1, 4])
@pytest.mark.parametrize("drop_last", [False, True])
@pytest.mark.parametrize("shuffle", [False, True])
def test_loader_order_equals_tensorloader(world, drop_last, shuffle):
    from vit_som_amd.data import DeviceDataset, DeviceLoader, DeviceTransform
    from vit_som_amd.train import TensorLoader
    n, bs = 203, 16
    images = torch.zeros(n, 8, 8, 3, dtype=torch.uint8)                   # [N, H, W, C] is permuted once
    labels = torch.arange(n)
    ds = DeviceDataset(images, labels, device="cpu")
    assert tuple(ds.images.shape) == (n, 3, 8, 8) and len(ds) == n
    tr = DeviceTransform(True, 3, 8, (0.5,) * 3, (0.5,) * 3)
    for rank in range(world):
        ref = TensorLoader(labels.float().view(n, 1), labels, bs, shuffle=shuffle, rank=rank, world_size=world, seed=5, drop_last=drop_last)
        dl = DeviceLoader(ds, bs, tr, shuffle=shuffle, rank=rank, world_size=world, seed=5, drop_last=drop_last)
        assert len(dl) == len(ref) and dl.dataset is ds
        for epoch in range(2):
            want = [y for _, y in ref]
            got = list(dl.index_batches())
            assert len(got) == len(want) and all(torch.equal(g, w) for g, w in zip(got, want)), (rank, epoch)
        assert dl.epoch == ref.epoch == 2
        dl.set_epoch(0)
        assert torch.equal(next(iter(dl.index_batches())), next(iter(TensorLoader(labels.float().view(n, 1), labels, bs, shuffle=shuffle, rank=rank,
                                                                                   world_size=world, seed=5, drop_last=drop_last)))[1])


def test_dataset_layouts_and_npz(tmp_path):
    from vit_som_amd.data import DeviceDataset
    g = torch.Generator().manual_seed(0)
    x = torch.randint(0, 256, (5, 3, 8, 8), dtype=torch.uint8, generator=g)
    assert torch.equal(DeviceDataset(x.permute(0, 2, 3, 1), torch.arange(5), "cpu").images, x)
    assert tuple(DeviceDataset(x[:, 0], torch.arange(5), "cpu").images.shape) == (5, 1, 8, 8)
    with pytest.raises(ValueError):
        DeviceDataset(x.float(), torch.arange(5), "cpu")
    np.savez(tmp_path / "d.npz", images=x.permute(0, 2, 3, 1).numpy(), labels=np.arange(5, dtype=np.uint8))
    ds = DeviceDataset.from_npz(str(tmp_path / "d.npz"), device="cpu")
    assert torch.equal(ds.images, x) and ds.labels.dtype == torch.int64 and ds.labels.tolist() == [0, 1, 2, 3, 4]


def test_augment_entries_reject_bad_calls_without_gpu():
    from vit_som_amd._lib import last_error, lib
    ok = dict(src=16, N=10, C=3, H=32, W=32, index=16, params=16, B=4, S=32, R=32, off=0, mean=16, std=16, seed=1, epoch=0, out=16,
              out_u8=None, stream=None)

    def batch(**kw):
        return lib.vsom_augment_batch(*{**ok, **kw}.values())
    for name in ("src", "index", "mean", "std", "out"):
        assert batch(**{name: None}) == -1 and "null" in last_error()
    assert batch(C=2) == -3 and "channels" in last_error()
    assert batch(H=65, W=65) == -3
    assert batch(H=32, W=28) == -3
    assert batch(S=0) == -1
    assert batch(S=65, R=65) == -3
    assert batch(R=31) == -1 and batch(R=74) == -1 and batch(R=36, off=5) == -1
    assert batch(H=64, W=64, S=8, R=8) == -3                                # shrinks by more than 4
    assert batch(out=24) == -2 and batch(params=8) == -2
    assert batch(B=0) == -1 and batch(epoch=-1) == -1

    okp = dict(index=16, N=10, B=4, H=32, S=32, s0=0.08, s1=1.0, l0=-0.3, l1=0.3, two=1, t0=0.08, t1=1.0, m0=-0.3, m1=0.3, flip=0.5,
               erase=0.25, seed=1, epoch=0, params=16, stream=None)

    def plan(**kw):
        return lib.vsom_augment_plan(*{**okp, **kw}.values())
    assert plan(index=None) == -1 and plan(params=None) == -1
    assert plan(H=65) == -3 and plan(S=0) == -1 and plan(B=0) == -1 and plan(N=0) == -1 and plan(N=1 << 31) == -3
    assert plan(s0=0.0) == -1 and plan(s0=1.0, s1=0.5) == -1 and plan(t0=0.0) == -1
    assert plan(flip=1.5) == -1 and plan(erase=-0.1) == -1
    assert plan(params=8) == -2
