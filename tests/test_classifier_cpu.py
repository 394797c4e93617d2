"""ViTClassifier host surface (models/vit.py:243-340), without a GPU: state_dict layout against the reference's golden
key list, arena views, optimizer groups, learning rate and LambdaLR multipliers; a CPU input is refused."""
import copy
import json
import math
import os

import numpy as np
import pytest
import torch

from helpers import GOLDEN

CASES = ["ref_vitcls_hd8", "ref_vitcls_hd32"]


def _golden(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
    return z, json.loads(str(z["config"]))


@pytest.mark.parametrize("name", CASES)
def test_state_dict_keys_and_shapes_match_reference(name):
    import vit_som_amd
    z, cfg = _golden(name)
    m = vit_som_amd.ViTClassifier(copy.deepcopy(cfg), device="cpu")
    sd = m.state_dict()
    assert list(sd.keys()) == [str(k) for k in z["state_keys"]]
    for k, v in sd.items():
        assert tuple(v.shape) == z["param/" + k].shape, k
    assert "iteration" not in sd
    # the reference's parameters load as they are
    m.load_state_dict({k: torch.from_numpy(z["param/" + k]) for k in sd})
    assert torch.equal(m.cls_head.weight.detach(), torch.from_numpy(z["param/cls_head.weight"]))


def test_parameters_are_arena_views():
    import vit_som_amd
    _, cfg = _golden("ref_vitcls_hd8")
    m = vit_som_amd.ViTClassifier(copy.deepcopy(cfg), device="cpu")
    base = m.arena.params.data_ptr()
    end = base + m.arena.params.numel() * 4
    for n, p in m.named_parameters():
        if p.requires_grad:
            assert base <= p.data_ptr() < end, n
            assert p.data_ptr() == m.arena.p(n).data_ptr(), n
    assert m.model.decoder_embed.weight.requires_grad                     # the decoder is built, never run
    assert m._decoder_param_names()[0] == "model.decoder_embed.weight"


def test_init_distributions():
    import vit_som_amd
    _, cfg = _golden("ref_vitcls_hd32")
    cfg = copy.deepcopy(cfg)
    cfg["data"]["num_classes"] = 400
    m = vit_som_amd.ViTClassifier(cfg, device="cpu")
    w, b = m.cls_head.weight.detach(), m.cls_head.bias.detach()
    assert abs(float(w.std()) - 0.02) < 0.002
    bound = 1.0 / math.sqrt(w.shape[1])
    assert float(b.abs().max()) <= bound and float(b.abs().max()) > 0.5 * bound


@pytest.mark.parametrize("name", CASES)
def test_optimizer_groups_lr_and_schedule_match_reference(name):
    import vit_som_amd
    from vit_som_amd.optim import param_groups_lrd
    z, cfg = _golden(name)
    m = vit_som_amd.ViTClassifier(copy.deepcopy(cfg), device="cpu")
    (opt,), (sched,) = m.configure_optimizers()
    hp = cfg["hyperparameters"]
    opt_hp = hp["optimizer"]
    ref = param_groups_lrd(m.model, weight_decay=opt_hp["weight_decay"], layer_decay=opt_hp["layer_decay"])
    assert len(opt.param_groups) == len(ref) + 1
    for g, r in zip(opt.param_groups, ref):
        assert g["weight_decay"] == r["weight_decay"] and g["lr_scale"] == r["lr_scale"]
        assert [p.data_ptr() for p in g["params"]] == [p.data_ptr() for p in r["params"]]
    head = opt.param_groups[-1]
    assert head["weight_decay"] == 0.01 and "lr_scale" not in head
    assert [p.data_ptr() for p in head["params"]] == [m.cls_head.weight.data_ptr(), m.cls_head.bias.data_ptr()]
    assert opt.param_groups[0]["lr"] == pytest.approx(float(z["lr0"]), rel=1e-15)
    base = opt.param_groups[0]["initial_lr"]                             # LambdaLR already applied epoch 0's multiplier
    assert base == pytest.approx(opt_hp["lr"] * hp["batch_size"] / 256, rel=1e-15)
    for epoch in range(6):
        mult = max(opt_hp["min_lr"], min((epoch + 1) / (opt_hp["warmup_epochs"] + 1e-8),
                                         0.5 * (math.cos(epoch / hp["total_epochs"] * math.pi) + 1)))
        assert opt.param_groups[0]["lr"] == pytest.approx(base * mult, rel=1e-12)
        sched.step()
    # the decoder never gets a gradient in the reference: no weight decay on its arena slices either
    for n in m._decoder_param_names():
        assert m.arena.wd_by_name[n] == 0.0


def test_cpu_input_is_refused():
    import vit_som_amd
    _, cfg = _golden("ref_vitcls_hd8")
    m = vit_som_amd.ViTClassifier(copy.deepcopy(cfg), device="cpu")
    d = cfg["data"]
    x = torch.zeros(2, d["num_channels"], d["input_size"], d["input_size"])
    with pytest.raises(ValueError):
        m(x)
    with pytest.raises(ValueError):
        m.predict(x)


def test_loss_has_no_label_smoothing_although_the_config_sets_it():
    import vit_som_amd
    _, cfg = _golden("ref_vitcls_hd8")
    assert cfg["hyperparameters"]["optimizer"]["smoothing"] == 0.1
    m = vit_som_amd.ViTClassifier(copy.deepcopy(cfg), device="cpu")
    assert m.smoothing == 0.0


def test_set_distributed_without_som_layer():
    import vit_som_amd
    _, cfg = _golden("ref_vitcls_hd8")
    m = vit_som_amd.ViTClassifier(copy.deepcopy(cfg), device="cpu")
    m.set_distributed(1, 0, backend="torch")
    assert m.world_size == 1 and not hasattr(m, "som_layer")


def test_train_driver_dispatches_on_model_arch(monkeypatch):
    from vit_som_amd import train
    _, cfg = _golden("ref_vitcls_hd8")
    seen = {}
    monkeypatch.setattr(train, "main_vit", lambda config, **kw: seen.setdefault("vit", kw) or {})
    train.main(copy.deepcopy(cfg), n_runs=1, max_epochs=1)
    assert "vit" in seen
    assert seen["vit"]["model_states_dir"] == "experiments/states/vit"
