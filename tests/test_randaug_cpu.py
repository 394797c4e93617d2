"""RandAugment / rand-m9 in the device data pipeline, without a GPU: the numpy restatement of the PIL primitives against
PIL's own bytes (tests/golden/pil_randaug_ops.npz, made by tools/gen_pil_randaug.py), the tables of the plan restatement,
DeviceTransform.from_config(auto_augment=True) on the reference's configs, and the argument checks of the two C entries."""
import glob
import math
import os
import warnings

import numpy as np
import pytest
import yaml

import randaug_ref as RA

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def golden_groups():
    """[(src [n_src, C, S, S], index [n], slot [n, 16], out [n, C, S, S])]"""
    z = np.load(os.path.join(GOLDEN, "pil_randaug_ops.npz"))
    groups, k = [], 0
    while f"g{k}_src" in z:
        groups.append(tuple(z[f"g{k}_{n}"] for n in ("src", "index", "slot", "out")))
        k += 1
    return groups


def record_with(slot_words, s):
    """One record row with the 16 words of a golden case in slot s, the others empty."""
    row = RA.empty_record()[0]
    row[RA.SLOT0 + s * RA.SLOT_WORDS:RA.SLOT0 + (s + 1) * RA.SLOT_WORDS] = slot_words
    return row


def test_restatement_equals_pil_bytes():
    cases = 0
    for k, (src, index, slot, out) in enumerate(golden_groups()):
        for b in range(len(index)):
            s = RA.get_slot(record_with(slot[b], 0), 0)
            got = RA.apply_slot(src[index[b]], s)
            assert np.array_equal(got, out[b]), f"group {k} case {b} ({s}): {(got != out[b]).sum()} bytes differ from PIL"
            cases += 1
    assert cases >= 140


def test_golden_file_covers_the_primitives_and_the_edges():
    groups = golden_groups()
    assert [(g[0].shape[1], g[0].shape[2]) for g in groups] == [(3, 32), (1, 16), (3, 64)]
    assert os.path.getsize(os.path.join(GOLDEN, "pil_randaug_ops.npz")) < os.path.getsize(os.path.join(GOLDEN, "pil_bicubic_crops.npz"))
    for src, index, slot, out in groups[:2]:
        S = src.shape[2]
        slots = [RA.get_slot(record_with(w, 0), 0) for w in slot]
        assert {s["op"] for s in slots} == set(range(1, RA.N_OPS))                       # every primitive
        for op in (RA.AFFINE_NEAREST, RA.AFFINE_BICUBIC):
            a = np.array([s["a"] for s in slots if s["op"] == op])
            assert (a[:, 1] > 0).any() and (a[:, 1] < 0).any() and (a[:, 3] > 0).any() and (a[:, 3] < 0).any()      # both signs
            assert (np.abs(a[:, 2]) > S).any() or (np.abs(a[:, 5]) > S).any()          # the whole image pushed out
        for op in (RA.BRIGHTNESS, RA.COLOR, RA.CONTRAST, RA.SHARPNESS):
            f = [s["f"] for s in slots if s["op"] == op]
            assert min(f) < 1.0 < max(f)                                                # both sides of 1
        assert {0, 8} <= {s["ip"] for s in slots if s["op"] == RA.POSTERIZE}
        for b, s in enumerate(slots):                   # a constant channel and equalize's step == 0 come out unchanged
            if s["op"] in (RA.AUTOCONTRAST, RA.EQUALIZE) and index[b] == 2:
                c = src.shape[1] // 2
                assert np.array_equal(out[b][c], src[2][c]) and len(np.unique(src[2][c])) == 1
            if s["op"] == RA.EQUALIZE and index[b] == 3:
                assert np.array_equal(out[b], src[3])
    assert any(np.array_equal(o, np.zeros_like(o)) for o in groups[0][3])              # NEAREST, fill 0, everything outside
    sources64 = set(groups[2][1].tolist())
    assert {0, 1} <= sources64                                                          # noise and smooth at 64 x 64


def test_restatement_equals_pil_on_fresh_cases():
    """Random parameters the golden file does not hold (skipped without PIL)."""
    Image = pytest.importorskip("PIL.Image")
    from PIL import ImageEnhance, ImageOps
    rng = np.random.default_rng(11)
    for t in range(24):
        C, S = ((3, 32), (1, 16), (3, 48))[t % 3]
        src = rng.integers(0, 256, (C, S, S), dtype=np.uint8)
        im = Image.fromarray(src[0]) if C == 1 else Image.fromarray(np.ascontiguousarray(src.transpose(1, 2, 0)))
        fill = tuple(int(v) for v in rng.integers(0, 256, C))
        angle = float(np.float32(rng.uniform(-30, 30)))
        f = float(np.float32(rng.uniform(0.1, 1.9)))
        a = tuple(float(np.float32(v)) for v in (1, rng.uniform(-0.3, 0.3), rng.uniform(-5, 5), rng.uniform(-0.3, 0.3), 1, rng.uniform(-5, 5)))
        pf = fill[0] if C == 1 else fill
        want = [(dict(op=RA.AFFINE_NEAREST, a=RA.rotate_matrix(angle, S), fill=fill), im.rotate(angle, resample=Image.NEAREST, fillcolor=pf)),
                (dict(op=RA.AFFINE_BICUBIC, a=RA.rotate_matrix(angle, S), fill=fill), im.rotate(angle, resample=Image.BICUBIC, fillcolor=pf)),
                (dict(op=RA.AFFINE_NEAREST, a=a, fill=fill), im.transform((S, S), Image.AFFINE, a, resample=Image.NEAREST, fillcolor=pf)),
                (dict(op=RA.AFFINE_BICUBIC, a=a, fill=fill), im.transform((S, S), Image.AFFINE, a, resample=Image.BICUBIC, fillcolor=pf)),
                (dict(op=RA.CONTRAST, f=f), ImageEnhance.Contrast(im).enhance(f)),
                (dict(op=RA.SHARPNESS, f=f), ImageEnhance.Sharpness(im).enhance(f)),
                (dict(op=RA.COLOR, f=f), ImageEnhance.Color(im).enhance(f)),
                (dict(op=RA.EQUALIZE, ip=0), ImageOps.equalize(im)),
                (dict(op=RA.AUTOCONTRAST, ip=0), ImageOps.autocontrast(im))]
        for slot, pil in want:
            w = np.asarray(pil)
            w = w[None] if C == 1 else w.transpose(2, 0, 1)
            assert np.array_equal(RA.apply_slot(src, slot), w), (t, slot)


def test_plan_tables_are_the_two_policies_numbers():
    """torchvision RandAugment(magnitude=9, num_magnitude_bins=31) and timm rand-m9-mstd0.5-inc1, as include/vitsom_hip.h lists them."""
    assert len(RA.TV_OPS) == 14 and len(RA.TIMM_OPS) == 15
    assert RA.TV_SHEAR == pytest.approx(0.09, abs=1e-15) and RA.TV_ROTATE == pytest.approx(9.0, abs=1e-13)
    assert RA.TV_ENHANCE == pytest.approx(0.27, abs=1e-15) and RA.TV_POSTERIZE == 7 and RA.TV_SOLARIZE == 178.5
    assert [RA.tv_translate(S) for S in (28, 32, 64)] == [int(150 / 331 * S * 0.3) for S in (28, 32, 64)] == [3, 4, 8]
    S = 32
    ident = (0.0,) * 6
    for neg, sg in ((False, 1.0), (True, -1.0)):
        m = math.tan(math.radians(math.degrees(math.atan(0.09))))
        want = {"Identity": (RA.NONE, 0, 1.0, ident), "ShearX": (RA.AFFINE_NEAREST, 0, 1.0, (1, sg * m, 0, 0, 1, 0)),
                "ShearY": (RA.AFFINE_NEAREST, 0, 1.0, (1, 0, 0, sg * m, 1, 0)), "TranslateX": (RA.AFFINE_NEAREST, 0, 1.0, (1, 0, -sg * 4, 0, 1, 0)),
                "TranslateY": (RA.AFFINE_NEAREST, 0, 1.0, (1, 0, 0, 0, 1, -sg * 4)), "Rotate": (RA.AFFINE_NEAREST, 0, 1.0, RA.rotate_matrix(sg * 9.0, S)),
                "Brightness": (RA.BRIGHTNESS, 0, 1 + sg * 0.27, ident), "Color": (RA.COLOR, 0, 1 + sg * 0.27, ident),
                "Contrast": (RA.CONTRAST, 0, 1 + sg * 0.27, ident), "Sharpness": (RA.SHARPNESS, 0, 1 + sg * 0.27, ident),
                "Posterize": (RA.POSTERIZE, 7, 1.0, ident), "Solarize": (RA.SOLARIZE, 179, 1.0, ident),
                "AutoContrast": (RA.AUTOCONTRAST, 0, 1.0, ident), "Equalize": (RA.EQUALIZE, 0, 1.0, ident)}
        for k, name in enumerate(RA.TV_OPS):
            op, ip, f, a = RA.tv_slot(k, neg, S)
            assert (op, ip) == want[name][:2] and f == pytest.approx(want[name][2], abs=1e-15) and a == pytest.approx(want[name][3], abs=1e-13), name
        for mag in (0.0, 2.6, 9.0, 10.0):
            want = {"AutoContrast": (RA.AUTOCONTRAST, 0, 1.0), "Equalize": (RA.EQUALIZE, 0, 1.0), "Invert": (RA.INVERT, 0, 1.0),
                    "PosterizeIncreasing": (RA.POSTERIZE, 4 - int(0.4 * mag), 1.0), "SolarizeIncreasing": (RA.SOLARIZE, 256 - int(25.6 * mag), 1.0),
                    "SolarizeAdd": (RA.SOLARIZE_ADD, min(128, int(11 * mag)), 1.0)}
            for name in ("Color", "Contrast", "Brightness", "Sharpness"):
                want[name + "Increasing"] = (getattr(RA, name.upper()), 0, max(0.1, 1 + sg * 0.09 * mag))
            coef = {"Rotate": RA.rotate_matrix(sg * 3 * mag, S), "ShearX": (1, sg * 0.03 * mag, 0, 0, 1, 0), "ShearY": (1, 0, 0, sg * 0.03 * mag, 1, 0),
                    "TranslateXRel": (1, 0, sg * 0.045 * mag * S, 0, 1, 0), "TranslateYRel": (1, 0, 0, 0, 1, sg * 0.045 * mag * S)}
            for k, name in enumerate(RA.TIMM_OPS):
                op, ip, f, a = RA.timm_slot(k, neg, mag, S)
                if name in coef:
                    assert op == RA.AFFINE_BICUBIC and a == pytest.approx(coef[name], abs=1e-12), name
                else:
                    assert (op, ip) == want[name][:2] and f == pytest.approx(want[name][2], abs=1e-14), (name, mag)
    assert RA.timm_fill((0.4914, 0.4822, 0.4465)) == (125, 123, 114) and RA.timm_fill((0.5,)) == (128,)
    # Image.rotate's recipe: 9 degrees about (16, 16)
    c, s = math.cos(math.radians(9)), math.sin(math.radians(9))
    assert RA.rotate_matrix(9.0, 32) == pytest.approx((c, -s, 16 - 16 * c + 16 * s, s, c, 16 - 16 * s - 16 * c), abs=1e-12)


def test_plan_restatement_frequencies_and_independence():
    n, epoch, seed = 6000, 1, 77
    index = np.arange(n)
    rec = RA.plan(index, epoch, seed, 32, 2, True, 0.3, (125, 123, 114))
    band = lambda p, m: 5 * math.sqrt(m * p * (1 - p))                                  # noqa: E731
    assert abs(int(rec[:, 0].sum()) - n * 0.3) <= band(0.3, n) and abs(int(rec[:, 1].sum()) - n * 0.5) <= band(0.5, n)
    for cols, ops in (((2, 3), 14), ((4, 5), 15)):
        picks = rec[:, cols].ravel()
        assert picks.min() == 0 and picks.max() == ops - 1
        for k in range(ops):
            assert abs(int((picks == k).sum()) - 2 * n / ops) <= band(1 / ops, 2 * n), (ops, k)
    applied = np.array([(rec[:, 6] >> t) & 1 for t in (0, 1)]).ravel()
    assert abs(int(applied.sum()) - n) <= band(0.5, 2 * n)
    for t in (0, 1):                                    # a timm slot that is not applied is empty; an applied one is not
        op = rec[:, RA.SLOT0 + (2 + t) * RA.SLOT_WORDS]
        assert (op[((rec[:, 6] >> t) & 1) == 0] == RA.NONE).all() and (op[((rec[:, 6] >> t) & 1) == 1] != RA.NONE).all()
    fills = rec[:, RA.SLOT0 + 2 * RA.SLOT_WORDS + 3]
    assert set(fills[rec[:, RA.SLOT0 + 2 * RA.SLOT_WORDS] == RA.AFFINE_BICUBIC].tolist()) == {125 | 123 << 8 | 114 << 16}
    # a record depends on (seed, epoch, index) and on nothing else; empty stages leave their slots empty
    again = RA.plan(index[100:110][::-1].copy(), epoch, seed, 32, 2, True, 0.3, (125, 123, 114))
    assert np.array_equal(again[::-1], rec[100:110])
    assert not np.array_equal(RA.plan(index[:64], epoch + 1, seed, 32, 2, True, 0.3, (125, 123, 114)), rec[:64])
    none = RA.plan(index[:64], epoch, seed, 32, 0, False, 0.3, (125, 123, 114))
    assert (none[:, 2:] == np.array([-1] * 4 + [0] * (RA.WORDS - 6))).all() and np.array_equal(none[:, :2], rec[:64, :2])
    one = RA.plan(index[:64], epoch, seed, 32, 1, False, 0.3, (125, 123, 114))
    assert np.array_equal(one[:, :RA.SLOT0 + RA.SLOT_WORDS][:, [0, 1, 2] + list(range(RA.SLOT0, RA.SLOT0 + RA.SLOT_WORDS))],
                          rec[:64][:, [0, 1, 2] + list(range(RA.SLOT0, RA.SLOT0 + RA.SLOT_WORDS))])


CONFIGS = [p for p in sorted(glob.glob(os.path.join(GOLDEN, "config_vit*.yaml"))) if "flowers" not in p]


@pytest.mark.parametrize("path", CONFIGS, ids=[os.path.basename(p)[7:-5] for p in CONFIGS])
def test_transform_from_config_with_auto_augment(path):
    from vit_som_amd.data import PLAIN_SETS, DeviceTransform
    with open(path) as fh:
        cfg = yaml.safe_load(fh)
    d = cfg["data"]
    a = d["augment"]
    with warnings.catch_warnings():
        warnings.simplefilter("error")                                                  # no warning, and strict does not refuse
        tr = DeviceTransform.from_config(cfg, True, auto_augment=True, strict=True)
        ev = DeviceTransform.from_config(cfg, False, auto_augment=True, strict=True)
    assert not ev.auto_augment
    if d["dataset"] in PLAIN_SETS:
        assert not tr.auto_augment and not tr.augment
        return
    assert tr.auto_augment and tr.augment and tr.two_stage
    assert tr.randaug_n == a["randaug_n"] == 2 and tr.autoaugment is True and tr.flip1_p == a["horizontal_flip"]
    assert tr.fill_tv == (0,) * d["num_channels"] and tr.fill_timm == RA.timm_fill(tr.mean) and len(tr.fill_timm) == d["num_channels"]
    assert tr.erase_p == a["reprob"] and tr.scale == tuple(a["resize_scale"])
    cfg["data"]["augment"].update(randaug_n=0, autoaugment=False)
    off = DeviceTransform.from_config(cfg, True, auto_augment=True, strict=True)
    assert off.auto_augment and off.randaug_n == 0 and off.autoaugment is False      # empty stages, the two flips still apart
    cfg["data"]["augment"].update(randaug_n=3)
    with pytest.raises(ValueError, match="randaug_n"):
        DeviceTransform.from_config(cfg, True, auto_augment=True)


def test_config_fixtures_counted():
    assert len(CONFIGS) == 13 and sum("som" in os.path.basename(p) for p in CONFIGS) == 8


def test_default_call_still_warns_and_refuses_word_for_word():
    from vit_som_amd.data import DeviceTransform
    with open(os.path.join(GOLDEN, "config_vit_som_cifar-10.yaml")) as fh:
        cfg = yaml.safe_load(fh)
    msg = ("DeviceTransform: RandAugment / auto-augment (randaug_n, autoaugment) are not applied by the device pipeline: crops, "
           "flip and random erasing only")
    with pytest.warns(UserWarning) as rec:
        tr = DeviceTransform.from_config(cfg, True)
    assert str(rec[0].message) == msg and not tr.auto_augment
    with pytest.raises(NotImplementedError) as exc:
        DeviceTransform.from_config(cfg, True, strict=True)
    assert str(exc.value) == msg


def test_randaug_entries_reject_bad_calls_without_gpu():
    from vit_som_amd._lib import last_error, lib
    ok = dict(src=16, N=10, C=3, H=32, W=32, index=16, params=16, ra=16, B=4, S=32, mean=16, std=16, seed=1, epoch=0, out=16, out_u8=None,
              stream=None)

    def batch(**kw):
        return lib.vsom_augment_batch_ra(*{**ok, **kw}.values())
    for name in ("src", "index", "params", "ra", "mean", "std", "out"):
        assert batch(**{name: None}) == -1 and "null" in last_error()
    assert batch(C=2) == -3 and "channels" in last_error()
    assert batch(H=65, W=65) == -3 and batch(H=32, W=28) == -3
    assert batch(S=0) == -1 and batch(S=65) == -3 and batch(H=64, W=64, S=8) == -3
    assert batch(out=24) == -2 and batch(params=8) == -2 and batch(ra=8) == -2 and batch(out_u8=2) == -2
    assert batch(B=0) == -1 and batch(epoch=-1) == -1 and batch(N=1 << 31) == -3

    okp = dict(index=16, N=10, B=4, S=32, n=2, auto=1, flip=0.5, fill_tv=0, fill_timm=125 | 123 << 8 | 114 << 16, seed=1, epoch=0, ra=16,
               stream=None)

    def plan(**kw):
        return lib.vsom_randaug_plan(*{**okp, **kw}.values())
    assert plan(index=None) == -1 and plan(ra=None) == -1
    assert plan(S=65) == -3 and plan(S=0) == -1 and plan(B=0) == -1 and plan(N=0) == -1 and plan(N=1 << 31) == -3
    assert plan(n=3) == -3 and "randaug_n" in last_error() and plan(n=-1) == -3
    assert plan(flip=1.5) == -1 and plan(fill_timm=1 << 24) == -1 and plan(epoch=-1) == -1
    assert plan(ra=8) == -2
