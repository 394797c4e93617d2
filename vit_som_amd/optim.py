"""The reference's layer-decay parameter groups and the fused AdamW step over the flat arena."""
import weakref
from typing import Dict

import torch

from . import ops
from .tuning import hooks


def get_layer_id_for_vit(name: str, num_layers: int) -> int:
    """tools/utils.py:73-84."""
    if name in ("cls_token", "pos_embed") or name.startswith("patch_embed"):
        return 0
    if name.startswith("blocks"):
        return int(name.split(".")[1]) + 1
    return num_layers


def param_groups_lrd(model, weight_decay=0.05, no_weight_decay_list=(), layer_decay=0.75):
    """tools/utils.py:28-71: layer/decay groups carrying an ``lr_scale`` key (inert downstream,
    SURVEY.md 3.3 -- kept so optimizer.param_groups looks like the reference's)."""
    groups: Dict[str, dict] = {}
    num_layers = len(model.blocks) + 1
    scales = [layer_decay ** (num_layers - i) for i in range(num_layers + 1)]
    for n, p in model.named_parameters():
        if not p.requires_grad:
            continue
        if p.ndim == 1 or n in no_weight_decay_list:
            g_decay, this_decay = "no_decay", 0.0
        else:
            g_decay, this_decay = "decay", weight_decay
        layer_id = get_layer_id_for_vit(n, num_layers)
        name = "layer_%d_%s" % (layer_id, g_decay)
        if name not in groups:
            groups[name] = {"lr_scale": scales[layer_id], "weight_decay": this_decay, "params": []}
        groups[name]["params"].append(p)
    return list(groups.values())


# ------------------------------------------------------------------------------------ optimiser
class FusedAdamW(torch.optim.Optimizer):
    """torch.optim.AdamW / Adam semantics (vit_som.py:146-157) as ONE kernel over the flat arena.

    ``param_groups`` mirror the reference's (layer/decay groups with the inert ``lr_scale`` key
    plus the prototypes/cls_head group with AdamW's default weight_decay=0.01).  All groups
    share one lr (the reference's single-lambda LambdaLR scales them equally).  ``step()``
    first sums the gradient arena across ranks (RCCL all-reduce) when world_size > 1."""

    def __init__(self, model: "ViTSOM", param_groups, lr, betas, adamw=True, eps=1e-8):
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=0.01 if adamw else 0.0)
        super().__init__(param_groups, defaults)
        self._model = model
        self._adamw = adamw
        self._step = 0
        self._wd_seen = None
        self._sync_weight_decay()

    def _sync_weight_decay(self):
        """The kernel reads weight decay per 256-float chunk from arena.wd_chunk; the groups are where it is set -- by the
        constructor, by load_state_dict, by whoever edits param_groups (torch allows it).  One host-side comparison of the
        groups' values per call; the chunks are rewritten only when a value (or the arena) has changed."""
        a = self._model.arena
        wds = tuple(float(g["weight_decay"]) for g in self.param_groups)
        if self._wd_seen is not None and self._wd_seen[0]() is a and self._wd_seen[1] == wds:
            return
        name_of = {id(p): n for n, p in self._model._named_trainable()}
        for g, wd in zip(self.param_groups, wds):
            for p in g["params"]:
                a.set_weight_decay(name_of[id(p)], wd)
        if self._model.classification:
            # the reference leaves the decoder without gradients in classification mode, so
            # torch's AdamW never touches it (no decay either) -- SURVEY.md section 5 defect (a)
            for n in self._model._decoder_param_names():
                a.set_weight_decay(n, 0.0)
        self._wd_seen = (weakref.ref(a), wds)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:               # Lightning's automatic optimization passes training_step + backward here
            with torch.enable_grad():
                loss = closure()
        m = self._model
        m.allreduce_gradients()
        self._sync_weight_decay()
        self._step += 1
        g0 = self.param_groups[0]
        lrs = {float(g["lr"]) for g in self.param_groups}
        if len(lrs) != 1:
            raise RuntimeError("FusedAdamW: per-group learning rates differ; the arena kernel uses one lr")
        b1, b2 = g0["betas"]
        som = getattr(m, "som_layer", None)
        planes = None
        if som is not None and hooks.adamw_planes and som._planes_used and som._planes_shape_ok(som._planes_rows):
            # the batch that last took the planes form would take it again: the prototypes' plane image for the next BMU
            # pass leaves the same kernel that updates them
            name = next((n for n, q in m._named_trainable() if q is som.prototypes), None)
            if name is not None:
                planes = (m.arena.offsets[name][0], *som.prototypes.shape, som._w_planes_buffer())
        ops.adamw_step(m.arena.params, m.arena.grads, m.arena.exp_avg, m.arena.exp_avg_sq, m.arena.wd_chunk,
                       float(g0["lr"]), b1, b2, g0["eps"], self._step, grad_scale=1.0 / m.world_size, adamw=self._adamw,
                       planes=planes)
        if som is not None:
            som._raw_updates += 1                                # the kernel writes through raw pointers
            som._wplanes_stamp = som._w_stamp() if planes is not None else None
        return loss

    def zero_grad(self, set_to_none: bool = True):
        # gradients are fully overwritten by every backward pass; nothing to clear
        return None

    # torch.optim.AdamW-compatible state layout (per-parameter 'step' / 'exp_avg' / 'exp_avg_sq' in
    # param_groups order), so optimizer states interchange with reference-written checkpoints
    def _param_names_in_group_order(self):
        name_of = {id(p): n for n, p in self._model._named_trainable()}
        return [name_of[id(p)] for g in self.param_groups for p in g["params"]]

    def state_dict(self):
        a = self._model.arena
        names = self._param_names_in_group_order()
        state = {}
        if self._step > 0:
            for i, n in enumerate(names):
                state[i] = {"step": torch.tensor(float(self._step)), "exp_avg": a.view(a.exp_avg, n).clone(),
                            "exp_avg_sq": a.view(a.exp_avg_sq, n).clone()}
        groups, k = [], 0
        for g in self.param_groups:
            pg = {key: v for key, v in g.items() if key != "params"}
            pg["params"] = list(range(k, k + len(g["params"])))
            k += len(g["params"])
            groups.append(pg)
        return {"state": state, "param_groups": groups}

    def load_state_dict(self, sd):
        a = self._model.arena
        names = self._param_names_in_group_order()
        if len(sd["param_groups"]) != len(self.param_groups):
            raise ValueError("FusedAdamW.load_state_dict: different number of parameter groups")
        for g, sg in zip(self.param_groups, sd["param_groups"]):
            for key, v in sg.items():
                if key != "params":
                    g[key] = v
        steps = set()
        a.exp_avg.zero_(); a.exp_avg_sq.zero_()
        for i, st in sd["state"].items():
            n = names[int(i)]
            a.view(a.exp_avg, n).copy_(st["exp_avg"])
            a.view(a.exp_avg_sq, n).copy_(st["exp_avg_sq"])
            steps.add(int(float(st["step"])))
        if len(steps) > 1:
            raise ValueError("FusedAdamW.load_state_dict: parameters carry different step counts")
        self._step = steps.pop() if steps else 0
        self._sync_weight_decay()
