"""Stopping a run and starting it again, as data and two functions: tests/test_resume_cpu.py checks what a load writes on
the host, tests/test_resume_gpu.py that a resumed run IS the uninterrupted one.

The oracle of a resumed run is the uninterrupted run of the same model on the same inputs: the steps are deterministic
(test_model_gpu.py::test_steps_are_deterministic, and the launch-tape tests bit for bit), so every comparison made through
`differences` is bit equality and there is no tolerance to choose.  The one tolerance of these modules is `adamw_close`,
the rule of tests/test_ops_gpu.py::test_adamw_step, for the optimizer against torch.optim.AdamW.

What a training step rests on besides the parameters, and who has to put it back after a load:
  _it / iteration      the host counter behind gamma_t and the SOM temperature, and its device twin (load_state_dict;
                       ViTClassifier has no buffer: load_from_checkpoint takes the file's global_step)
  opt._step, wd_chunk  FusedAdamW.load_state_dict; the moments live in the arena, compared per parameter through arena.view
                       (the padding between tensors is not state)
  plane image, stamp   SOMLayer.load_state_dict marks the prototypes' image stale; the next step splits them again
  W^T copies           rewritten by every backward pass
  launch tape          one per batch size; a load into a live model writes the arena in place, so the tape stays valid
  loss ring            where a step's loss terms land; only their values are compared
  LR scheduler         sched.load_state_dict; the lr itself travels in the optimizer's groups

`run_steps` is the one driver: steps first..last over a fixed list of inputs, sched.step() after every EPOCH_STEPS-th step
(the "epoch" boundary falls inside both halves of an interrupted run, so the lr changes before and after the stop), one
snapshot per step.  `save_snapshot` / `resume` stop and continue through the public surface only: save_checkpoint and
load_from_checkpoint where the model has them, state_dict / load_state_dict for DESOM and for a live model,
configure_optimizers, opt.load_state_dict, sched.load_state_dict, set_schedule."""
import copy
from collections import namedtuple

import torch

from helpers import golden_params, load_golden

EPOCH_STEPS = 3           # run_steps: sched.step() after steps 3, 6, ...
LOSS_SEED = 0.5           # mode "bridge": (LOSS_SEED * training_step(...)).backward(), the tape's segment 2
NOT_COMPARED = ("tape_id",)     # kept per step to assert which launch path ran; an id says nothing about the arithmetic

Case = namedtuple("Case", "kind cls cfg state schedule batch")


def vit_config_of(som_cfg):
    """The configs/vit/*.yaml-shaped config of the same shapes, as tests/test_fullsize_fp64_gpu.py::_vit_config_of makes it."""
    cfg = copy.deepcopy(som_cfg)
    cfg["hyperparameters"]["model_arch"] = "vit"
    del cfg["hyperparameters"]["gamma"], cfg["hyperparameters"]["som"]
    return cfg


def case(kind):
    """The models of these tests at their smallest shapes: `cluster` / `cls` = ViTSOM on ref_cluster_tiny / ref_cls_tiny,
    `vit` = ViTClassifier on ref_cls_tiny's ViT and cls_head, `desom` = DESOM on ref_desom_tiny, `planes` = the depth-3
    B = 192 ViTSOM whose BMU pass takes the planes form (state None: seeded init, started at iteration 40 -- at 0 the gamma
    ramp gives the SOM term no weight)."""
    import vit_som_amd
    if kind == "planes":
        from oracle.gen_golden import make_config
        cfg = make_config(3, 32, 4, 192, 3, 3, 96, 2, (8, 8), 0, 192)
        return Case(kind, vit_som_amd.ViTSOM, cfg, None, (4000, 400), 192)
    z, cfg = load_golden({"cluster": "ref_cluster_tiny", "cls": "ref_cls_tiny", "vit": "ref_cls_tiny", "desom": "ref_desom_tiny"}[kind])
    state = golden_params(z)
    B = int(z["x"].shape[0])
    if kind == "desom":
        return Case(kind, vit_som_amd.DESOM, cfg, state, (int(z["n_train"]),), B)
    if kind == "vit":
        state = {("model." + k[4:] if k.startswith("vit.") else k): v for k, v in state.items()
                 if k.startswith(("vit.", "cls_head."))}
        return Case(kind, vit_som_amd.ViTClassifier, vit_config_of(cfg), state, (int(z["n_train"]), int(z["est_steps"])), B)
    return Case(kind, vit_som_amd.ViTSOM, cfg, state, (int(z["n_train"]), int(z["est_steps"])), B)


def optimizers(model):
    """configure_optimizers() in either of its return shapes -> (optimizer, scheduler or None)."""
    out = model.configure_optimizers()
    if isinstance(out, tuple):
        (opt,), (sched,) = out
        return opt, sched
    return out, None


def fresh(c, device):
    """A new model in the case's initial state, scheduled, with its optimizer and scheduler."""
    if c.state is None:
        torch.manual_seed(0)
    model = c.cls(copy.deepcopy(c.cfg), device=device)
    if c.state is not None:
        model.load_state_dict(c.state)
    else:
        sd = model.state_dict()
        sd["iteration"] = torch.tensor(40)
        model.load_state_dict(sd)
    model.set_schedule(*c.schedule)
    return (model,) + optimizers(model)


def inputs_of(c, sizes, seed=3):
    """One (x, y) host batch per entry of `sizes`, fixed by the seed."""
    d = c.cfg["data"]
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(B, d["num_channels"], d["input_size"], d["input_size"], generator=g),
             torch.randint(0, max(int(d["num_classes"]), 1), (B,), generator=g)) for B in sizes]


def _host(v):
    return v.detach().cpu().clone() if torch.is_tensor(v) else v


def tape_id(model, B):
    """The id of the launch tape of batch size B (0: none); only ViTSOM records one."""
    vit = getattr(model, "vit", None)
    acts = getattr(vit, "_acts", {}).get(B) if vit is not None else None
    tape = acts.__dict__.get("tape") if acts is not None else None
    return tape.id if tape is not None else 0


def step_snapshot(model, opt, loss, B):
    """What one step leaves behind, on the host: loss and logged terms, the counters, the lr it ran with, the temperature and
    gamma_t and the BMUs where the model has them."""
    snap = {"loss": _host(loss), "_it": model._it, "opt_step": opt._step, "lr": opt.param_groups[0]["lr"]}
    for k, v in model._last.items():
        snap["last/" + k] = _host(v)
    if "iteration" in model._buffers:
        snap["iteration"] = int(model.iteration)
    som = getattr(model, "som_layer", None)
    if som is not None:
        snap["T"] = float(som.current_temperature)
        snap["bmu"] = _host(model._ctx[2].bmu)
    snap["tape_id"] = tape_id(model, B)
    return snap


def final_state(model, val_batch=None):
    """Clones of the parameter, gradient and moment arenas, per parameter; with `val_batch` also the validation loss (taken
    after training steps: SOMLayer.current_temperature is a plain attribute that only a training step sets)."""
    a = model.arena
    out = {}
    for n, _ in model._named_trainable():
        for key, buf in (("p", a.params), ("g", a.grads), ("m", a.exp_avg), ("v", a.exp_avg_sq)):
            out[f"{key}/{n}"] = _host(a.view(buf, n))
    if val_batch is not None:
        x, y = (t.to(a.device) for t in val_batch)
        out["val"] = _host(model.validation_step((x, y), 0))
    return out


def run_steps(model, opt, sched, inputs, first, last, mode="fused", trace=None):
    """Steps first..last (counted from 1) over inputs[first - 1:last]; mode "fused" = train_step_fused, "bridge" =
    training_step(...) and a backward with LOSS_SEED.  -> trace: step -> step_snapshot."""
    trace = {} if trace is None else trace
    dev = model.arena.device
    for i in range(first, last + 1):
        x, y = (t.to(dev) for t in inputs[i - 1])
        if mode == "fused":
            loss = model.train_step_fused(x, y)
        else:
            loss = model.training_step((x, y), i - 1)
            (LOSS_SEED * loss).backward()
        opt.step()
        trace[i] = step_snapshot(model, opt, loss, x.shape[0])
        if sched is not None and i % EPOCH_STEPS == 0:
            sched.step()
    return trace


def save_snapshot(model, opt, sched, path):
    """The run's state as a file: save_checkpoint where the model has it, the same layout from state_dict for DESOM."""
    if hasattr(model, "save_checkpoint"):
        return model.save_checkpoint(path, opt, sched, epoch=sched.last_epoch)
    torch.save({"state_dict": {k: v.detach().cpu().clone() for k, v in model.state_dict().items()},
                "optimizer_states": [opt.state_dict()], "lr_schedulers": [] if sched is None else [sched.state_dict()]}, path)
    return path


def resume(c, path, device, live=None):
    """Continue from the file: in a fresh model (load_from_checkpoint where the class has it, else construct and
    load_state_dict), or in `live` = (model, opt, sched), whose buffers, tapes and optimizer stay the ones they are.
    -> (model, opt, sched)."""
    ckpt = torch.load(path, map_location="cpu", weights_only=True)
    if live is not None:
        model, opt, sched = live
        model.load_state_dict(ckpt["state_dict"])
    else:
        if hasattr(c.cls, "load_from_checkpoint"):
            model = c.cls.load_from_checkpoint(path, device=device)
        else:
            model = c.cls(copy.deepcopy(c.cfg), device=device)
            model.load_state_dict(ckpt["state_dict"])
        model.set_schedule(*c.schedule)
        opt, sched = optimizers(model)
    opt.load_state_dict(ckpt["optimizer_states"][0])
    if sched is not None:
        sched.load_state_dict(ckpt["lr_schedulers"][0])
    return model, opt, sched


def differences(a, b):
    """Keys of two snapshots (step_snapshot or final_state) whose values are not bit-equal, or that only one of them has."""
    bad = [k for k in set(a) ^ set(b) if k not in NOT_COMPARED]
    for k in set(a) & set(b):
        if k in NOT_COMPARED:
            continue
        u, v = a[k], b[k]
        if torch.is_tensor(u) or torch.is_tensor(v):
            same = torch.is_tensor(u) and torch.is_tensor(v) and u.dtype == v.dtype and torch.equal(u, v)
        else:
            same = type(u) is type(v) and u == v
        if not same:
            bad.append(k)
    return sorted(bad)


# ------------------------------------------------------------------------------------ the optimizer against torch
def adamw_close(got, ref):
    """The rule of tests/test_ops_gpu.py::test_adamw_step, quoted: torch.allclose(pd.cpu(), ref, atol=2e-7)."""
    return torch.allclose(got.detach().cpu(), ref.detach().cpu(), atol=2e-7)


def torch_adamw_over(opt):
    """torch.optim.AdamW over host clones of FusedAdamW's parameters, group by group in its order (the construction of
    test_train_driver.py::test_checkpoint_layout_roundtrip_cpu).  -> (reference optimizer, names, leaves)."""
    names = opt._param_names_in_group_order()
    leaves = [p.detach().cpu().clone().requires_grad_(True) for g in opt.param_groups for p in g["params"]]
    k, groups = 0, []
    for g in opt.param_groups:
        groups.append({"params": leaves[k:k + len(g["params"])], "weight_decay": g["weight_decay"]})
        k += len(g["params"])
    g0 = opt.param_groups[0]
    return torch.optim.AdamW(groups, lr=g0["lr"], betas=tuple(g0["betas"]), eps=g0["eps"]), names, leaves


def foreign_edit(sd, lr=3e-3, eps=1e-6):
    """An optimizer state as another run would have written it: its own weight decay in every group (0.10, 0.15, ...: none
    of them a value of this project's configs), its own eps and lr."""
    sd = {"state": sd["state"], "param_groups": [dict(g) for g in sd["param_groups"]]}
    for i, g in enumerate(sd["param_groups"]):
        g["weight_decay"], g["eps"], g["lr"] = 0.10 + 0.05 * i, eps, lr
    return sd


def expected_wd(model, opt):
    """name -> the weight decay the kernel must apply: the parameter's group's, 0 for the decoder in classification mode."""
    names = iter(opt._param_names_in_group_order())
    want = {next(names): float(g["weight_decay"]) for g in opt.param_groups for _ in g["params"]}
    if model.classification:
        for n in model._decoder_param_names():
            want[n] = 0.0
    return want


def wd_chunks_of(model, name):
    """The entries of arena.wd_chunk that cover parameter `name`."""
    off, n, _ = model.arena.offsets[name]
    return model.arena.wd_chunk[off // 256:(off + (n + 255) // 256 * 256) // 256].cpu()
