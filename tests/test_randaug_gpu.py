"""RandAugment / rand-m9 in the device data pipeline on the MI355X: vsom_augment_batch_ra against PIL's bytes
(tests/golden/pil_randaug_ops.npz), normalisation bitwise against torch, the empty record against vsom_augment_batch, the two
flips, vsom_randaug_plan against its numpy restatement, the whole two-stage transform against the restatement fed the device's
own records, independence of an image from batch size / position / rank count, the loader and the train driver, and records
no plan would write."""
import copy
import math
import signal
import warnings

import numpy as np
import pytest
import torch

import data_ref as R
import randaug_ref as RA
from helpers import load_golden
from test_randaug_cpu import golden_groups, record_with

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CIFAR_MEAN, CIFAR_STD = (0.4914, 0.4822, 0.4465), (0.2023, 0.1994, 0.2010)


@pytest.fixture(autouse=True)
def time_limit(request):
    """A limit of its own (seconds) for every test here: a SIGALRM handler, which ends a test whose host side is slow or
    loops; a test stuck inside a device call is bounded by the `timeout` the suite runs under, as in test_data_gpu.py."""
    limit = 300 if "driver" in request.node.name else 120

    def expired(signum, frame):
        raise TimeoutError(f"{request.node.name}: no result after {limit} s")
    old = signal.signal(signal.SIGALRM, expired)
    signal.alarm(limit)
    yield
    signal.alarm(0)
    signal.signal(signal.SIGALRM, old)


def stats(C):
    return (CIFAR_MEAN, CIFAR_STD) if C == 3 else ((0.5,), (0.5,))


def whole_image_plan(n, H, S, second=False):
    p = np.zeros((n, R.PARAMS), np.int32)
    p[:, 2:4] = H
    if second:
        p[:, 6:8] = S
    return p


def run_ra(src, index, params, rec, S, seed=0, epoch=0):
    """(fp32 output, 8-bit image) of one vsom_augment_batch_ra launch; numpy in, torch (device) out."""
    from vit_som_amd import ops
    src = torch.as_tensor(src).to(DEV)
    C, B = src.shape[1], len(index)
    mean, std = (torch.tensor(v, dtype=torch.float32, device=DEV) for v in stats(C))
    out = torch.full((B, C, S, S), float("nan"), device=DEV)
    out8 = torch.full((B, C, S, S), 77, dtype=torch.uint8, device=DEV)
    ops.augment_batch_ra(src, torch.as_tensor(index).to(DEV), torch.as_tensor(params).to(DEV).contiguous(),
                         torch.as_tensor(rec).to(DEV).contiguous(), out, S, mean, std, seed, epoch, out_u8=out8)
    torch.cuda.synchronize()
    return out, out8


def run_plain(src, index, params, S, seed=0, epoch=0):
    from vit_som_amd import ops
    src = torch.as_tensor(src).to(DEV)
    C, B = src.shape[1], len(index)
    mean, std = (torch.tensor(v, dtype=torch.float32, device=DEV) for v in stats(C))
    out = torch.full((B, C, S, S), float("nan"), device=DEV)
    out8 = torch.full((B, C, S, S), 77, dtype=torch.uint8, device=DEV)
    ops.augment_batch(src, torch.as_tensor(index).to(DEV), torch.as_tensor(params).to(DEV).contiguous(), out, S, S, 0, mean, std, seed, epoch,
                      out_u8=out8)
    torch.cuda.synchronize()
    return out, out8


def torch_normalise(u8, mean, std):
    C = u8.shape[1]
    m = torch.tensor(mean, dtype=torch.float32, device=u8.device).view(1, C, 1, 1)
    s = torch.tensor(std, dtype=torch.float32, device=u8.device).view(1, C, 1, 1)
    return (u8.float() / torch.tensor(255.0, device=u8.device) - m) / s


# ------------------------------------------------------------------ every primitive is PIL's, byte for byte
GROUPS = golden_groups()


@pytest.mark.parametrize("second_crop", [False, True])
@pytest.mark.parametrize("k", range(len(GROUPS)))
def test_primitives_equal_pil_bytes(k, second_crop):
    """One active slot per sample -- case b in slot b mod 4, so every primitive runs in both stages and from every buffer --
    and identity crops (H = S: every coefficient row is a single 1); with `second_crop` an identity second crop as well."""
    src, index, slot, want = GROUPS[k]
    C, S = src.shape[1], src.shape[2]
    rec = np.stack([record_with(slot[b], b % 4) for b in range(len(index))])
    out, out8 = run_ra(src, index, whole_image_plan(len(index), S, S, second_crop), rec, S)
    got = out8.cpu().numpy()
    bad = [b for b in range(len(index)) if not np.array_equal(got[b], want[b])]
    print(f"group {k}: C={C} S={S}: {len(index)} cases, {int((got != want).sum())} of {want.size} bytes differ; cases {bad[:8]}")
    assert not bad, [(b, RA.get_slot(rec[b], b % 4)) for b in bad[:3]]
    assert torch.equal(out, torch_normalise(out8, *stats(C)))                           # the fp32 output, bit for bit


def test_two_primitives_in_one_stage_compose():
    """Slots 0 and 1 (and 2 and 3) both active: the second acts on the result of the first."""
    src, index, slot, want = GROUPS[0]
    S = src.shape[2]
    pairs = [(b, (b + 17) % len(index)) for b in range(0, len(index), 3)]
    for first in (0, 2):
        rec = RA.empty_record(len(pairs))
        for n, (b, c) in enumerate(pairs):
            rec[n] = record_with(slot[b], first)
            rec[n, RA.SLOT0 + (first + 1) * RA.SLOT_WORDS:RA.SLOT0 + (first + 2) * RA.SLOT_WORDS] = slot[c]
        idx = index[[b for b, _ in pairs]]
        _, out8 = run_ra(src, idx, whole_image_plan(len(pairs), S, S), rec, S)
        ref = np.stack([RA.apply_slot(want[b], RA.get_slot(record_with(slot[c], 0), 0)) for b, c in pairs])
        assert np.array_equal(out8.cpu().numpy(), ref)


# ------------------------------------------------------------------ the empty record is vsom_augment_batch
@pytest.mark.parametrize("C,H,S", [(3, 32, 32), (3, 64, 32), (1, 28, 28), (3, 32, 30)])
def test_empty_record_equals_augment_batch_and_the_flips(C, H, S):
    rng = np.random.default_rng(5)
    src = rng.integers(0, 256, (16, C, H, H), dtype=np.uint8)
    index = rng.integers(0, 16, 48).astype(np.int64)
    params, _ = R.plan(index, 2, 13, H=H, S=S, scale=(0.08, 1.0), ratio=(0.75, 1.3333), two_stage=True, flip_p=0.5, erase_p=0.5)
    params[::5, 4:8] = 0                                                                # some samples with one crop only
    assert (params[:, 11] > 0).any() and (params[:, 8] == 1).any()
    rec = RA.empty_record(len(index))
    plain = params.copy()
    plain[:, 8] = 0
    want, want8 = run_plain(src, index, plain, S, seed=13, epoch=2)
    out, out8 = run_ra(src, index, params, rec, S, seed=13, epoch=2)                    # the merged flip p[8] is not read
    assert torch.equal(out8, want8) and torch.equal(out, want)
    plain[:, 8] = 1
    want, want8 = run_plain(src, index, plain, S, seed=13, epoch=2)
    rec[:, 1] = 1                                                                       # flip 2 alone
    out, out8 = run_ra(src, index, params, rec, S, seed=13, epoch=2)
    assert torch.equal(out8, want8) and torch.equal(out, want)
    rec[:, 0] = 1                                                                       # both flips
    _, out8 = run_ra(src, index, params, rec, S, seed=13, epoch=2)
    both = np.stack([RA.transform_u8(src[i], p, r, S) for i, p, r in zip(index, params, rec)])
    assert np.array_equal(out8.cpu().numpy(), both)
    rec[:, 1] = 0                                                                       # flip 1 alone: before the second crop
    _, out8 = run_ra(src, index, params, rec, S, seed=13, epoch=2)
    first = np.stack([RA.transform_u8(src[i], p, r, S) for i, p, r in zip(index, params, rec)])
    assert np.array_equal(out8.cpu().numpy(), first)
    one = params[:, 6] == 0
    assert np.array_equal(first[one], want8.cpu().numpy()[one]) and not np.array_equal(first[~one], want8.cpu().numpy()[~one])


# ------------------------------------------------------------------ the plan
def device_plan(index, N, S, n_tv, timm, flip1_p, fill, seed, epoch):
    from vit_som_amd import ops
    rec = torch.full((len(index), ops.RANDAUG_PARAMS), -7, dtype=torch.int32, device=DEV)
    ops.randaug_plan(torch.as_tensor(index).to(DEV), rec, N, S, n_tv, timm, flip1_p, (0,) * len(fill), fill, seed, epoch)
    torch.cuda.synchronize()
    return rec.cpu().numpy()


PLAN_CASES = [dict(index=np.arange(8192), S=32, n_tv=2, timm=True, flip1_p=0.5, fill=(125, 123, 114), seed=0, epoch=0),
              dict(index=np.arange(50000 - 1024, 50000), S=64, n_tv=1, timm=True, flip1_p=0.2, fill=(124, 116, 104), seed=(7 << 32) | 5, epoch=41),
              dict(index=np.arange(0, 512 * 3, 3), S=28, n_tv=2, timm=False, flip1_p=0.5, fill=(128,), seed=99, epoch=3)]


@pytest.mark.parametrize("case", range(len(PLAN_CASES)))
def test_plan_equals_restatement(case):
    """Integers identical; affine coefficients within 1e-12 (the device's sin / cos / tan / log are not Python's, and
    Image.rotate's round(., 15) is Python's decimal rounding); the fp32 factor within one fp32 step at 2 (2.4e-7): it is
    the rounding of a double the two sides know to 1e-12."""
    kw = PLAN_CASES[case]
    index = kw["index"]
    got = device_plan(index, int(index.max()) + 1, kw["S"], kw["n_tv"], kw["timm"], kw["flip1_p"], kw["fill"], kw["seed"], kw["epoch"])
    want = RA.plan(index, kw["epoch"], kw["seed"], kw["S"], kw["n_tv"], kw["timm"], kw["flip1_p"], kw["fill"])
    bad = np.flatnonzero((RA.integer_words(got) != RA.integer_words(want)).any(1))
    dc = float(np.abs(RA.coefficients(got) - RA.coefficients(want)).max())
    df = float(np.abs(RA.factors(got).astype(np.float64) - RA.factors(want)).max())
    print(f"case {case}: {len(bad)} of {len(index)} records differ in an integer; coefficients max |diff| {dc:.3g}, factors {df:.3g}")
    assert len(bad) == 0, (bad[:5], RA.integer_words(got)[bad[:2]], RA.integer_words(want)[bad[:2]])
    assert dc <= 1e-12 and df <= 2.4e-7
    if case == 0:
        n = len(index)
        band = lambda p, m: 5 * math.sqrt(m * p * (1 - p))                              # noqa: E731
        for cols, ops_n in (((2, 3), 14), ((4, 5), 15)):
            for c in cols:
                counts = np.bincount(got[:, c], minlength=ops_n)
                print(f"word {c}: counts {counts.tolist()} (expected {n / ops_n:.0f} +- {band(1 / ops_n, n):.0f})")
                assert len(counts) == ops_n and (np.abs(counts - n / ops_n) <= band(1 / ops_n, n)).all()
        for t in (0, 1):
            applied = int(((got[:, 6] >> t) & 1).sum())
            assert abs(applied - n / 2) <= band(0.5, n), (t, applied)
        for c in (0, 1):
            assert abs(int(got[:, c].sum()) - n / 2) <= band(0.5, n)


def test_plan_does_not_move_the_crop_plan():
    """The record has a Philox stream of its own: vsom_augment_plan writes what its restatement (data_ref.plan) says, before
    and after vsom_randaug_plan has run on the same indices."""
    from vit_som_amd import ops
    index = torch.arange(512, device=DEV)
    lr, lr2 = (math.log(0.75), math.log(1.3333)), (math.log(R.TIMM_RATIO[0]), math.log(R.TIMM_RATIO[1]))
    want, margin = R.plan(np.arange(512), 1, 3, **R.CIFAR_PLAN)
    assert margin.min() > 1e-9
    rec = torch.zeros(512, ops.RANDAUG_PARAMS, dtype=torch.int32, device=DEV)
    for _ in range(2):
        a = torch.zeros(512, ops.AUGMENT_PARAMS, dtype=torch.int32, device=DEV)
        ops.augment_plan(index, a, 512, 32, 32, (0.08, 1.0), lr, R.TIMM_SCALE, lr2, 0.5, 0.25, 3, 1)
        assert np.array_equal(a.cpu().numpy(), want)
        ops.randaug_plan(index, rec, 512, 32, 2, True, 0.5, (0, 0, 0), (125, 123, 114), 3, 1)


# ------------------------------------------------------------------ end to end
@pytest.mark.parametrize("H,S", [(32, 32), (64, 32)])
def test_two_stage_training_transform_equals_restatement(H, S):
    """Device plan, device record, device batch kernel; the restatement is fed the device's own two records."""
    from vit_som_amd import ops
    n, C, seed, epoch = 64, 3, 21, 5
    rng = np.random.default_rng(H)
    src = rng.integers(0, 256, (n, C, H, H), dtype=np.uint8)
    yy, xx = np.mgrid[0:H, 0:H]
    src[::2] = (127.5 + 127.5 * np.sin(xx * 0.21 + np.arange(n // 2)[:, None, None, None]) * np.cos(yy * 0.17 + np.arange(C)[None, :, None, None])).astype(np.uint8)
    index = torch.randperm(n, generator=torch.Generator().manual_seed(1)).to(DEV)
    params = torch.zeros(n, ops.AUGMENT_PARAMS, dtype=torch.int32, device=DEV)
    rec = torch.zeros(n, ops.RANDAUG_PARAMS, dtype=torch.int32, device=DEV)
    lr = (math.log(0.75), math.log(1.3333))
    ops.augment_plan(index, params, n, H, S, (0.08, 1.0), lr, R.TIMM_SCALE, (math.log(0.75), math.log(4 / 3)), 0.5, 0.0, seed, epoch)
    ops.randaug_plan(index, rec, n, S, 2, True, 0.5, (0, 0, 0), RA.timm_fill(CIFAR_MEAN), seed, epoch)
    mean, std = (torch.tensor(v, dtype=torch.float32, device=DEV) for v in stats(C))
    out = torch.empty(n, C, S, S, device=DEV)
    out8 = torch.empty(n, C, S, S, dtype=torch.uint8, device=DEV)
    ops.augment_batch_ra(torch.as_tensor(src).to(DEV), index, params, rec, out, S, mean, std, seed, epoch, out_u8=out8)
    torch.cuda.synchronize()
    p, r, idx, got = params.cpu().numpy(), rec.cpu().numpy(), index.cpu().numpy(), out8.cpu().numpy()
    used = sorted({RA.get_slot(r[b], s)["op"] for b in range(n) for s in range(4)})
    want = np.stack([RA.transform_u8(src[idx[b]], p[b], r[b], S) for b in range(n)])
    bad = [b for b in range(n) if not np.array_equal(got[b], want[b])]
    print(f"{H} -> {S}: {len(bad)} of {n} images differ ({int((got != want).sum())} bytes); primitives met: {used}")
    assert not bad, [(b, [RA.get_slot(r[b], s)["op"] for s in range(4)], r[b, :2].tolist()) for b in bad[:4]]
    assert len(used) >= 10 and torch.equal(out, torch_normalise(out8, *stats(C)))


# ------------------------------------------------------------------ independence from batching
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
    n = 512
    g = torch.Generator().manual_seed(2)
    ds = DeviceDataset(torch.randint(0, 256, (n, 3, 32, 32), dtype=torch.uint8, generator=g), torch.arange(n), DEV)   # label = index
    tr = DeviceTransform(True, 3, 32, CIFAR_MEAN, CIFAR_STD, auto_augment=True, randaug_n=2, autoaugment=True)
    plain = DeviceTransform(True, 3, 32, CIFAR_MEAN, CIFAR_STD)
    a = _epoch_images(ds, tr, 64, 0, 1, 0)
    b = _epoch_images(ds, tr, 256, 0, 1, 0)
    assert sorted(a) == sorted(b) == list(range(n)) and all(torch.equal(a[k], b[k]) for k in a)     # batch size 64 and 256
    r0, r1 = _epoch_images(ds, tr, 64, 0, 2, 0), _epoch_images(ds, tr, 64, 1, 2, 0)
    assert not set(r0) & set(r1) and sorted(set(r0) | set(r1)) == list(range(n))
    assert all(torch.equal(a[k], v) for k, v in {**r0, **r1}.items())                               # two ranks
    nxt = _epoch_images(ds, tr, 64, 0, 1, 1)
    assert sum(not torch.equal(nxt[k], a[k]) for k in a) > n * 0.99                                 # another epoch
    off = _epoch_images(ds, plain, 64, 0, 1, 0)
    assert sum(not torch.equal(off[k], a[k]) for k in a) > n * 0.9                                  # the policies do something


# ------------------------------------------------------------------ the loader and the driver
def test_loader_runs_an_epoch_with_auto_augment():
    from vit_som_amd import ops
    from vit_som_amd.data import DeviceLoader
    from vit_som_amd.train import device_loaders
    _, cfg = load_golden("ref_cls_tiny")
    cfg = copy.deepcopy(cfg)
    cfg["hyperparameters"]["batch_size"] = 32
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        train, val, test = device_loaders(cfg, n_train=256, n_val=64, n_test=64, auto_augment=True, strict=True)
    assert isinstance(train, DeviceLoader) and train.transform.auto_augment and not val.transform.auto_augment
    C, S = cfg["data"]["num_channels"], cfg["data"]["input_size"]
    seen = 0
    for x, y in train:
        assert tuple(x.shape) == (32, C, S, S) and bool(torch.isfinite(x).all()) and y.dtype == torch.int64
        seen += len(y)
    assert seen == 256 and len(train) == 8
    assert all(tuple(slot[2].shape) == (32, ops.RANDAUG_PARAMS) for slot in train._ring)           # the ring holds the record
    assert all(slot[2] is None for slot in val._buffers())
    picks = torch.cat([slot[2][:, 2:6] for slot in train._ring]).cpu().numpy()
    assert picks.min() >= 0 and picks[:, :2].max() <= 13 and picks[:, 2:].max() <= 14              # both stages drawn


def test_driver_takes_three_steps_with_auto_augment(tmp_path):
    from vit_som_amd.train import device_loaders, main
    _, cfg = load_golden("ref_cls_tiny")
    cfg = copy.deepcopy(cfg)
    cfg["hyperparameters"]["batch_size"] = 32
    logs, made = [], []

    def loaders(c, r, w):
        made.append(device_loaders(c, r, w, n_train=96, n_val=64, n_test=64, auto_augment=True))
        return made[-1]
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        main(cfg, n_runs=1, max_epochs=1, make_loaders=loaders, model_states_dir=str(tmp_path / "states"), log=logs.append)
    assert not [w for w in caught if "RandAugment" in str(w.message)]
    assert len(made[0][0]) == 3 and made[0][0].transform.auto_augment and made[0][0].epoch >= 1
    losses = [float(l.split("train/total_loss=")[1].split()[0]) for l in logs if "train/total_loss=" in l]
    assert len(losses) == 1 and math.isfinite(losses[0])


# ------------------------------------------------------------------ records no plan would write
def test_malformed_records_are_made_safe():
    """An unknown primitive does nothing; NaN / infinite / huge coefficients and factors, parameters out of range and
    garbage flips are clamped: every launch returns success (ops.* raises on any other status) and writes valid images."""
    src, index, slot, want = GROUPS[0]
    S = src.shape[2]
    n = 16
    idx = np.zeros(n, np.int64)
    params = whole_image_plan(n, S, S, True)
    base = RA.empty_record(n)
    _, clean = run_ra(src, idx, params, base, S)
    rec = base.copy()
    for b, op in enumerate((13, 99, -1, -2 ** 31, 2 ** 31 - 1, 1 << 16)):                # primitive codes out of range
        for s in range(4):
            RA.put_slot(rec[b], s, 0, 5, 1.5, (1, 2, 3), (1, 0.1, 2, 0.1, 1, 2))
            rec[b, RA.SLOT0 + s * RA.SLOT_WORDS] = op
    out, out8 = run_ra(src, idx, params, rec, S)
    assert torch.equal(out8, clean) and bool(torch.isfinite(out).all())
    bad = [float("nan"), float("inf"), -float("inf"), 1e300, -1e300, 1e-320]
    badf = [float("nan"), float("inf"), -float("inf"), 3e38, -3e38, 1e-40]
    rec = base.copy()
    for b in range(n):
        a = [bad[(b + i) % len(bad)] for i in range(6)]
        RA.put_slot(rec[b], 0, RA.AFFINE_NEAREST, 0, 1.0, (9, 9, 9), a)
        RA.put_slot(rec[b], 1, RA.SHARPNESS if b % 2 else RA.CONTRAST, 0, badf[b % len(badf)], (0, 0, 0))
        RA.put_slot(rec[b], 2, RA.AFFINE_BICUBIC, 0, 1.0, (9, 9, 9), a[::-1])
        RA.put_slot(rec[b], 3, (RA.POSTERIZE, RA.SOLARIZE, RA.SOLARIZE_ADD)[b % 3], (-5, 1 << 30, -2 ** 31, 300)[b % 4])
        rec[b, :2] = (b * 1000003, -b)
        rec[b, 2:8] = 2 ** 31 - 1
    out, out8 = run_ra(src, idx, params, rec, S)
    assert bool(torch.isfinite(out).all()) and torch.equal(out, torch_normalise(out8, *stats(3)))
    # a NaN factor is 1 and NaN coefficients are 0: the first of these is the identity, the second pixel (0, 0) everywhere
    rec = base.copy()
    RA.put_slot(rec[0], 0, RA.BRIGHTNESS, 0, float("nan"))
    RA.put_slot(rec[1], 0, RA.AFFINE_NEAREST, 0, 1.0, (0, 0, 0), (float("nan"),) * 6)
    _, out8 = run_ra(src, idx, params, rec, S)
    assert torch.equal(out8[0], clean[0]) and torch.equal(out8[1], clean[1][:, :1, :1].expand_as(clean[1]))
