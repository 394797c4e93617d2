"""The variable-size data pipeline without a GPU: the restatement against the committed PIL cases, ragged packing and its
validation, the variable-size transform of the flowers configs, the offline packer, and the new entries' argument checks."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

import ragged_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NEW_ENTRIES = ("vsom_augment_plan_ragged", "vsom_augment_batch_ragged", "vsom_augment_ragged_scratch_bytes")


def test_restatement_equals_every_pil_case():
    cases = G.golden_cases()
    assert len(cases) >= 40
    for row, out in cases:
        got = G.case_u8(row)
        assert np.array_equal(got, out), f"case {row.tolist()}: {(got != out).sum()} bytes differ from PIL"


def test_golden_file_covers_the_edges():
    t = np.array([row for row, _ in G.golden_cases()])
    c = {name: t[:, k] for k, name in enumerate(G.COLS)}
    train, ev = c["mode"] != G.EVAL, c["mode"] == G.EVAL
    assert (c["h"] > c["w"]).any() and (c["h"] < c["w"]).any()
    assert (c["h"] == 1).any() and (c["w"] == 1).any()
    assert (train & (c["h1"] == 1)).any() and (train & (c["w1"] == 1)).any()
    assert (train & (c["h1"] == c["h"]) & (c["w1"] == c["w"])).any()
    assert (train & (c["h1"] == 8 * c["S"])).any() and (train & (c["w1"] == 8 * c["S"])).any()          # 33 taps
    assert (train & (c["h1"] < 4 * c["S"]) & (c["h1"] > 3.9 * c["S"])).any()
    assert (train & (c["h1"] < 4) & (c["S"] >= 16)).any()                                                 # upsampling
    assert (c["c"] == 1).any() and (c["c"] == 3).any()
    assert (c["mode"] == G.TWO_CROPS).sum() >= 5
    assert (train & (c["S"] == 40) & (c["h1"] > 273)).any()             # more source rows than the ring of a 40-wide band holds
    assert (ev & (c["h"] > c["w"])).any() and (ev & (c["h"] < c["w"])).any() and (ev & (c["h"] == c["w"])).any()
    assert (ev & ((c["OH"] - c["S"]) % 2 == 1)).any() and (ev & ((c["OW"] - c["S"]) % 2 == 1)).any()     # half-integer offsets
    assert ((c["S"] == 224) & (c["mode"] == G.TWO_CROPS)).sum() == 1 and ((c["S"] == 224) & ev).sum() == 1
    assert set(c["S"][c["S"] != 224]) <= {16, 24, 40}
    for row in t[ev]:
        d = dict(zip(G.COLS, (int(v) for v in row)))
        assert G.eval_geometry(d["h"], d["w"], d["R"], d["S"]) == (d["OH"], d["OW"], d["top"], d["left"])
    assert os.path.getsize(G.GOLDEN_FILE) < 525414


def images_of_many_shapes():
    return [G.formula_image(5, 7, 3, 0), G.formula_image(1, 9, 3, 1), G.formula_image(16, 16, 3, 2), G.formula_image(33, 2, 3, 3)]


def test_packing_round_trips(tmp_path):
    from vit_som_amd.data import DeviceDataset, RaggedDeviceDataset
    imgs = images_of_many_shapes()
    labels = [3, 1, 4, 1]
    # [C, H, W], [H, W, C] and (one channel) [H, W] give the same planes
    ds = RaggedDeviceDataset.from_arrays(imgs, labels, "cpu", layout="CHW")
    hwc = RaggedDeviceDataset.from_arrays([im.transpose(1, 2, 0) for im in imgs], labels, "cpu")
    assert torch.equal(ds.data, hwc.data) and torch.equal(ds.offsets, hwc.offsets) and torch.equal(ds.shapes, hwc.shapes)
    gray = RaggedDeviceDataset.from_arrays([im[0] for im in imgs], labels, "cpu")
    assert gray.C == 1 and torch.equal(gray.image(3), torch.from_numpy(imgs[3][:1]))
    assert len(ds) == 4 and ds.C == 3 and (ds.max_h, ds.max_w) == (33, 16) and ds.device == torch.device("cpu")
    assert ds.offsets.dtype == torch.int64 and ds.shapes.dtype == torch.int32 and ds.labels.dtype == torch.int64
    assert ds.offsets.tolist() == [0, 112, 144, 912] and ds.shapes.tolist() == [[5, 7], [1, 9], [16, 16], [33, 2]]
    assert ds.data.numel() == 912 + 208 and ds.labels.tolist() == labels
    for n, im in enumerate(imgs):
        assert torch.equal(ds.image(n), torch.from_numpy(im))
    np.savez(tmp_path / "r.npz", **ds.to_npz_arrays())
    back = RaggedDeviceDataset.from_npz(str(tmp_path / "r.npz"), "cpu")
    for name in ("data", "offsets", "shapes", "labels"):
        assert torch.equal(getattr(back, name), getattr(ds, name)), name
    assert (back.C, back.max_h, back.max_w) == (3, 33, 16)
    # the common property of the two data set classes
    assert DeviceDataset(torch.zeros(2, 3, 4, 4, dtype=torch.uint8), torch.arange(2), "cpu").device == torch.device("cpu")


def test_each_validation_failure_has_its_own_message():
    from vit_som_amd.data import RaggedDeviceDataset
    ds = RaggedDeviceDataset.from_arrays(images_of_many_shapes(), [0, 1, 2, 3], "cpu", layout="CHW")
    ok = dict(data=ds.data, offsets=ds.offsets, shapes=ds.shapes, labels=ds.labels, channels=3, device="cpu")

    def build(**kw):
        return RaggedDeviceDataset(**{**ok, **kw})
    assert len(build()) == 4
    with pytest.raises(ValueError, match="multiples of 16"):
        build(offsets=torch.tensor([0, 112, 150, 912]))
    with pytest.raises(ValueError, match="increasing"):
        build(offsets=torch.tensor([0, 144, 112, 912]))
    with pytest.raises(ValueError, match="ends past the data buffer"):
        build(data=ds.data[:-16])
    with pytest.raises(ValueError, match="ends past the data buffer"):
        build(shapes=torch.tensor([[5, 7], [1, 9], [16, 16], [33, 3]], dtype=torch.int32))
    with pytest.raises(ValueError, match="at least 1"):
        build(shapes=torch.tensor([[5, 7], [0, 9], [16, 16], [33, 2]], dtype=torch.int32))
    with pytest.raises(ValueError, match="one label per image"):
        build(labels=torch.arange(3))
    with pytest.raises(ValueError, match="uint8"):
        build(data=ds.data.float())
    with pytest.raises(ValueError, match="channels"):
        build(channels=2)
    with pytest.raises(ValueError, match="channels"):
        RaggedDeviceDataset.from_arrays([G.formula_image(4, 5, 3, 0), G.formula_image(4, 5, 1, 0)], [0, 1], "cpu", layout="CHW")


FLOWERS = sorted(glob.glob(os.path.join(GOLDEN, "config_vit*flowers*.yaml")))


def test_flowers_configs_present():
    assert len(FLOWERS) == 4


@pytest.mark.parametrize("path", FLOWERS, ids=[os.path.basename(p)[7:-5] for p in FLOWERS])
def test_variable_size_transform_of_the_flowers_configs(path):
    from vit_som_amd.data import IMAGENET_DEFAULT_MEAN, IMAGENET_DEFAULT_STD, DeviceTransform
    with open(path) as fh:
        cfg = yaml.safe_load(fh)
    with pytest.raises(ValueError, match="fixed-size"):
        DeviceTransform.from_config(cfg, True)
    with pytest.raises(ValueError, match="fixed-size"):
        DeviceTransform.from_config(cfg, False)
    with pytest.warns(UserWarning, match="RandAugment"):
        tr = DeviceTransform.from_config(cfg, True, variable_size=True)
    ev = DeviceTransform.from_config(cfg, False, variable_size=True)
    for t in (tr, ev):
        assert (t.C, t.S, t.variable_size) == (3, 224, True) and t.mean == IMAGENET_DEFAULT_MEAN and t.std == IMAGENET_DEFAULT_STD
    assert (tr.R, tr.off, tr.augment, tr.two_stage) == (224, 0, True, True)
    assert (ev.R, ev.off, ev.augment) == (256, None, False)             # the window's offsets depend on the sample's shape
    a = cfg["data"]["augment"]
    assert tr.scale == tuple(a["resize_scale"]) and tr.ratio == tuple(a["resize_ratio"]) and tr.erase_p == a["reprob"]
    with pytest.raises(NotImplementedError, match="LDS"):
        DeviceTransform.from_config(cfg, True, auto_augment=True, variable_size=True)


def test_reuters_is_refused_either_way_and_other_sets_are_accepted():
    from vit_som_amd.data import DeviceTransform
    with open(os.path.join(GOLDEN, "config_vit_som_cifar-10.yaml")) as fh:
        cfg = yaml.safe_load(fh)
    t = DeviceTransform.from_config(cfg, False, variable_size=True)
    assert t.variable_size and (t.S, t.R) == (32, 36) and t.mean == (0.4914, 0.4822, 0.4465)
    assert not DeviceTransform.from_config(cfg, False).variable_size
    cfg["data"]["dataset"] = "reuters"
    with pytest.raises(ValueError, match="fixed-size"):
        DeviceTransform.from_config(cfg, False)
    with pytest.raises(ValueError, match="not an image set"):
        DeviceTransform.from_config(cfg, False, variable_size=True)


def test_loader_refuses_auto_augment_and_mismatched_transforms():
    from vit_som_amd.data import DeviceLoader, DeviceTransform, RaggedDeviceDataset
    ds = RaggedDeviceDataset.from_arrays(images_of_many_shapes(), [0, 1, 2, 3], "cpu", layout="CHW")
    with pytest.raises(NotImplementedError, match="LDS"):
        DeviceTransform(True, 3, 32, (0.5,) * 3, (0.5,) * 3, auto_augment=True, variable_size=True)
    fixed = DeviceTransform(True, 3, 32, (0.5,) * 3, (0.5,) * 3, auto_augment=True, randaug_n=2)
    with pytest.raises(NotImplementedError, match="LDS"):
        DeviceLoader(ds, 2, fixed)
    dl = DeviceLoader(ds, 2, DeviceTransform(False, 3, 32, (0.5,) * 3, (0.5,) * 3, variable_size=True))
    assert len(dl) == 2 and [j.tolist() for j in dl.index_batches()] == [[0, 1], [2, 3]]
    with pytest.raises(ValueError, match="variable_size"):
        DeviceTransform(False, 3, 32, (0.5,) * 3, (0.5,) * 3).apply(ds, None, None, None, 0, 0)


def test_pack_images_reproduces_pil(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    from vit_som_amd.data import RaggedDeviceDataset
    tree = tmp_path / "tree"
    files = {"rose": [("b.png", 31, 20), ("a.jpg", 18, 45)], "daisy": [("x.jpeg", 40, 40), ("m.png", 7, 64)], "tulip": [("t.png", 25, 9)]}
    k = 0
    for cls, items in files.items():
        (tree / cls).mkdir(parents=True)
        for name, h, w in items:
            im = Image.fromarray(np.ascontiguousarray(G.formula_image(h, w, 3, 2 * k + 1).transpose(1, 2, 0)))
            im.save(str(tree / cls / name), **({"quality": 90} if name.endswith(("jpg", "jpeg")) else {}))
            k += 1
    (tree / "rose" / "notes.txt").write_text("not an image")
    out = tmp_path / "flowers.npz"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "pack_images.py"), str(tree), str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    ds = RaggedDeviceDataset.from_npz(str(out), "cpu")
    order = [("daisy", "m.png"), ("daisy", "x.jpeg"), ("rose", "a.jpg"), ("rose", "b.png"), ("tulip", "t.png")]    # sorted classes, sorted files
    assert len(ds) == 5 and ds.C == 3 and ds.labels.tolist() == [0, 0, 1, 1, 2]
    for n, (cls, name) in enumerate(order):
        want = np.asarray(Image.open(str(tree / cls / name)).convert("RGB"))
        assert np.array_equal(ds.image(n).numpy(), want.transpose(2, 0, 1)), name
    with np.load(str(out)) as z:
        assert z["classes"].tolist() == ["daisy", "rose", "tulip"] and "test_data" not in z
    # one channel and a held-out part
    import importlib.util
    spec = importlib.util.spec_from_file_location("pack_images", os.path.join(ROOT, "tools", "pack_images.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    arrays = mod.pack(str(tree), str(tmp_path / "gray.npz"), gray=True, test_fraction=0.4, seed=1)
    assert len(arrays["labels"]) == 3 and len(arrays["test_labels"]) == 2
    tr, te = RaggedDeviceDataset.from_npz(str(tmp_path / "gray.npz"), "cpu"), RaggedDeviceDataset.from_npz(str(tmp_path / "gray.npz"), "cpu", "test_")
    assert tr.C == te.C == 1 and sorted(tr.labels.tolist() + te.labels.tolist()) == [0, 0, 1, 1, 2]
    want = {tuple(np.asarray(Image.open(str(tree / c / f)).convert("L")).reshape(-1).tolist()) for c, f in order}
    got = {tuple(d.image(n).reshape(-1).tolist()) for d in (tr, te) for n in range(len(d))}
    assert got == want
    src = open(os.path.join(ROOT, "tools", "pack_images.py")).read()
    assert "urllib" not in src and "requests" not in src and "http" not in src             # it decodes, it fetches nothing


def test_new_entries_are_exported_and_declared():
    import ctypes
    import re
    from vit_som_amd._lib import LIB_PATH, SIGNATURES
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vitsom_hip.h")).read(), flags=re.S)
    raw = ctypes.CDLL(LIB_PATH)
    for name in NEW_ENTRIES:
        assert hasattr(raw, name) and name in SIGNATURES and re.search(rf"\b{name}\s*\(", header), name
    from vit_som_amd import ops
    assert ops.augment_plan_ragged and ops.augment_batch_ragged and ops.augment_ragged_scratch_bytes


def test_new_entries_reject_bad_calls_without_gpu():
    from vit_som_amd._lib import last_error, lib
    assert lib.vsom_augment_ragged_scratch_bytes(128, 3, 224) >= 128 * 3 * 224 * 224
    assert lib.vsom_augment_ragged_scratch_bytes(128, 3, 224) % 16 == 0 and lib.vsom_augment_ragged_scratch_bytes(0, 3, 224) == 0
    ok = dict(data=16, data_bytes=1 << 20, offsets=16, shapes=16, N=10, C=3, max_h=500, max_w=667, index=16, params=16, B=4, S=224, R=224,
              mean=16, std=16, seed=1, epoch=0, scratch=16, scratch_bytes=4 * 3 * 224 * 224, out=16, out_u8=None, stream=None)

    def batch(**kw):
        return lib.vsom_augment_batch_ragged(*{**ok, **kw}.values())
    ev = dict(params=None, scratch=None, scratch_bytes=0, R=256)
    for name in ("data", "offsets", "shapes", "index", "mean", "std", "out"):
        assert batch(**{name: None}) == -1 and "null" in last_error(), name
    assert batch(C=2) == -3 and "channels" in last_error()
    assert batch(S=225, R=225) == -3 and "at most 224" in last_error()
    assert batch(S=0) == -1 and batch(B=0) == -1 and batch(epoch=-1) == -1 and batch(N=0) == -1 and batch(data_bytes=0) == -1
    assert batch(N=1 << 31) == -3
    assert batch(max_h=2049) == -3 and batch(max_w=2049) == -3 and "2048" in last_error()
    assert batch(max_w=8 * 224 + 1) == -3 and "more than 8" in last_error()         # a bound above 8 S
    assert batch(S=32, R=32, max_h=257, max_w=100) == -3 and batch(S=32, R=32, max_h=256, max_w=100, out=24) == -2
    assert batch(R=256) == -1                                                       # training resizes to S
    assert batch(scratch=None) == -4 and batch(scratch_bytes=100) == -4
    assert batch(data=24) == -2 and batch(out=24) == -2 and batch(params=8) == -2 and batch(scratch=8) == -2 and batch(out_u8=2) == -2
    assert batch(**ev, S=225) == -3
    assert batch(**{**ev, "R": 257}) == -3 and batch(**{**ev, "R": 200}) == -1
    assert batch(**{**ev, "R": 36}, S=32, max_h=8 * 36 + 1) == -3 and "more than 8" in last_error()   # a bound above 8 R

    okp = dict(index=16, shapes=16, N=10, B=4, S=224, s0=0.08, s1=1.0, l0=-0.3, l1=0.3, two=1, t0=0.08, t1=1.0, m0=-0.3, m1=0.3,
               flip=0.5, erase=0.25, seed=1, epoch=0, params=16, stream=None)

    def plan(**kw):
        return lib.vsom_augment_plan_ragged(*{**okp, **kw}.values())
    assert plan(index=None) == -1 and plan(shapes=None) == -1 and plan(params=None) == -1 and "null" in last_error()
    assert plan(S=225) == -3 and plan(S=0) == -1 and plan(B=0) == -1 and plan(N=0) == -1 and plan(N=1 << 31) == -3
    assert plan(s0=0.0) == -1 and plan(s0=1.0, s1=0.5) == -1 and plan(t0=0.0) == -1
    assert plan(flip=1.5) == -1 and plan(erase=-0.1) == -1
    assert plan(params=8) == -2
