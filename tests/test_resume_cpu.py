"""What a load writes on the host, without a kernel: the step counters, the weight decay the AdamW kernel reads, and a
checkpoint's round trip.  The runs themselves are tests/test_resume_gpu.py's; tests/resume.py is the shared part."""
import copy

import pytest
import torch

import resume as R


def _perturbed_moments(model, opt, step):
    """An optimizer that looks as if it had run: random moments for every parameter, a step count."""
    g = torch.Generator().manual_seed(1)
    a = model.arena
    for n, _ in model._named_trainable():
        a.view(a.exp_avg, n).copy_(torch.randn(a.offsets[n][2], generator=g))
        a.view(a.exp_avg_sq, n).copy_(torch.rand(a.offsets[n][2], generator=g))
    opt._step = step


@pytest.mark.parametrize("kind", ["cluster", "cls", "desom"])
def test_host_counter_follows_the_loaded_iteration_buffer(kind):
    """`_it` drives gamma_t and the SOM temperature; the reference reads the `iteration` buffer itself.  After
    load_state_dict both must hold the loaded value, in every model that has the buffer."""
    c = R.case(kind)
    model, _, _ = R.fresh(c, "cpu")
    want = int(c.state["iteration"])
    assert want > 0 and int(model.iteration) == want and model._it == want
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    sd["iteration"] = torch.tensor(37)
    other = c.cls(copy.deepcopy(c.cfg), device="cpu")
    assert other._it == 0
    other.load_state_dict(sd)
    assert int(other.iteration) == 37 and other._it == 37
    # and the schedule reads it: the temperature of the next step is the one of iteration 37, not Tmax
    other.set_schedule(*c.schedule)
    other.som_layer.update_temperature(other._it)
    assert other.som_layer.current_temperature < other.som_layer.Tmax


@pytest.mark.parametrize("kind", ["cluster", "cls", "vit"])
def test_weight_decay_chunks_follow_a_loaded_state_and_a_group_edit(kind):
    """The kernel reads arena.wd_chunk, the groups are where weight decay is set: after load_state_dict of a state with
    other values, and after an edit of param_groups (torch allows it), every parameter's chunks carry its group's value --
    the decoder's stay 0 in classification mode."""
    c = R.case(kind)
    model, opt, _ = R.fresh(c, "cpu")

    def check():
        want = R.expected_wd(model, opt)
        assert set(want) == {n for n, _ in model._named_trainable()}
        for n, wd in want.items():
            got = R.wd_chunks_of(model, n)
            assert got.numel() > 0 and bool((got == torch.tensor(wd, dtype=torch.float32)).all()), (n, wd, got.unique().tolist())
        if model.classification:
            assert model._decoder_param_names() and all(want[n] == 0.0 for n in model._decoder_param_names())

    check()                                                       # as constructed: {0, 0.01, 0.05}
    assert sorted(set(R.expected_wd(model, opt).values())) == [0.0, 0.01, 0.05]
    opt.load_state_dict(R.foreign_edit(opt.state_dict()))
    assert [g["weight_decay"] for g in opt.param_groups] == [0.10 + 0.05 * i for i in range(len(opt.param_groups))]
    check()
    for g in opt.param_groups:                                    # a live edit; the step is where the kernel would read it
        g["weight_decay"] = 0.5
    opt._sync_weight_decay()
    check()
    before = model.arena.wd_chunk.clone()
    seen = opt._wd_seen
    opt._sync_weight_decay()                                      # nothing changed: nothing is written
    assert opt._wd_seen is seen and torch.equal(model.arena.wd_chunk, before)


def test_classifier_checkpoint_restores_its_step_count(tmp_path):
    """ViTClassifier has no `iteration` buffer: its step count travels as the checkpoint's global_step."""
    c = R.case("vit")
    model, opt, sched = R.fresh(c, "cpu")
    model._it = 11
    path = model.save_checkpoint(str(tmp_path / "vit.ckpt"), opt, sched, epoch=2)
    assert torch.load(path, weights_only=True)["global_step"] == 11
    again = c.cls.load_from_checkpoint(path, device="cpu")
    assert again._it == 11
    assert torch.load(again.save_checkpoint(str(tmp_path / "vit2.ckpt")), weights_only=True)["global_step"] == 11


def _same_tree(a, b):
    if torch.is_tensor(a) or torch.is_tensor(b):
        return torch.is_tensor(a) and torch.is_tensor(b) and a.dtype == b.dtype and torch.equal(a, b)
    if isinstance(a, dict):
        return isinstance(b, dict) and set(a) == set(b) and all(_same_tree(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(_same_tree(u, v) for u, v in zip(a, b))
    return a == b


@pytest.mark.filterwarnings("ignore:Detected call of `lr_scheduler.step")      # no kernel here: the optimizer never steps
@pytest.mark.parametrize("kind", ["cluster", "cls", "vit"])
def test_save_load_save_writes_the_same_file_twice(kind, tmp_path):
    c = R.case(kind)
    model, opt, sched = R.fresh(c, "cpu")
    _perturbed_moments(model, opt, step=5)
    if "iteration" in model._buffers:
        model.iteration.fill_(11)
    model._it = 11
    sched.step(); sched.step()
    assert opt.param_groups[0]["lr"] != opt.param_groups[0]["initial_lr"]
    first = R.save_snapshot(model, opt, sched, str(tmp_path / "a.ckpt"))
    m2, o2, s2 = R.resume(c, first, "cpu")
    second = R.save_snapshot(m2, o2, s2, str(tmp_path / "b.ckpt"))
    ca, cb = torch.load(first, weights_only=True), torch.load(second, weights_only=True)
    assert ca["epoch"] == cb["epoch"] == 2 and ca["global_step"] == cb["global_step"] == 11
    for key in ("state_dict", "optimizer_states", "lr_schedulers", "hyper_parameters"):
        assert _same_tree(ca[key], cb[key]), key
    assert len(ca["optimizer_states"][0]["state"]) == len(list(model._named_trainable()))


def test_a_torch_written_classification_state_loads_without_decoder_entries():
    """torch's AdamW keeps no state for a parameter that never had a gradient: in a classification run, the decoder.  Such
    a state loads with zero moments there and the others' step count."""
    c = R.case("cls")
    model, opt, _ = R.fresh(c, "cpu")
    ref, names, leaves = R.torch_adamw_over(opt)
    decoder = set(model._decoder_param_names())
    assert decoder
    g = torch.Generator().manual_seed(2)
    for n, leaf in zip(names, leaves):
        leaf.grad = None if n in decoder else torch.randn(leaf.shape, generator=g)
    ref.step(); ref.step()
    sd = ref.state_dict()
    assert len(sd["state"]) == len(names) - len(decoder)
    _perturbed_moments(model, opt, step=9)                          # whatever was there before is gone after the load
    opt.load_state_dict(sd)
    assert opt._step == 2
    a = model.arena
    for i, n in enumerate(names):
        m, v = a.view(a.exp_avg, n), a.view(a.exp_avg_sq, n)
        if n in decoder:
            assert not m.any() and not v.any(), n
        else:
            assert torch.equal(m, sd["state"][i]["exp_avg"]) and torch.equal(v, sd["state"][i]["exp_avg_sq"]), n
    # the padding between tensors is not state, and holds none
    for buf in (a.exp_avg.clone(), a.exp_avg_sq.clone()):
        for n in names:
            a.view(buf, n).zero_()
        assert not buf.any()
