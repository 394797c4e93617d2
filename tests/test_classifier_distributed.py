"""ViTClassifier data parallel: two ranks sharing the one MI355X (gloo transport) reproduce the single-process step on
the concatenated batch, with the encoder buckets reduced inside the backward pass."""
import copy
import json
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from helpers import GOLDEN, rel_err


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close()
    return p


def _golden():
    z = np.load(os.path.join(GOLDEN, "ref_vitcls_hd32.npz"), allow_pickle=False)
    P = {str(k): torch.from_numpy(z["param/" + str(k)]) for k in z["state_keys"]}
    x = torch.cat([torch.from_numpy(z["x0"]), torch.from_numpy(z["x1"])])     # global batch of 12
    y = torch.cat([torch.from_numpy(z["y0"]), torch.from_numpy(z["y1"])])
    return json.loads(str(z["config"])), P, x, y


def _gpu_worker(rank, world, port, out):
    import vit_som_amd
    from vit_som_amd.tuning import hooks
    os.environ["VSOM_DIST_BACKEND"] = "gloo"
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    hooks.set(bucket_blocks=1)                              # one early piece per encoder block (the model has two)
    cfg, P, x, y = _golden()
    cfg = copy.deepcopy(cfg)
    per = x.shape[0] // world
    cfg["hyperparameters"]["batch_size"] = per
    m = vit_som_amd.ViTClassifier(cfg, device="cuda:0")
    m.load_state_dict(P)
    m.set_distributed(world, rank)
    (opt,), _ = m.configure_optimizers()
    xs, ys = x[rank * per:(rank + 1) * per].cuda(), y[rank * per:(rank + 1) * per].cuda()
    grads, overlapped = None, 0
    for s in range(2):
        if s == 0:
            loss = m.training_step((xs, ys), 0)
            loss.backward()
            overlapped = len(m._works)
            m.allreduce_gradients()
            grads = (m.arena.grads / world).cpu()
        else:
            m.train_step_fused(xs, ys)
        opt.step()
    torch.cuda.synchronize()
    assert overlapped >= 2, "the early (overlapped) all-reduce pieces were not issued"
    if rank == 0:
        torch.save({"params": m.arena.params.cpu(), "grads": grads, "lr": opt.param_groups[0]["lr"]}, out)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.gpu
def test_two_ranks_equal_single_process_on_concatenated_batch(tmp_path):
    import vit_som_amd
    out = str(tmp_path / "dp.pt")
    mp.spawn(_gpu_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    dp = torch.load(out)
    cfg, P, x, y = _golden()
    cfg = copy.deepcopy(cfg)
    cfg["hyperparameters"]["batch_size"] = x.shape[0]
    m = vit_som_amd.ViTClassifier(cfg, device="cuda:0")
    m.load_state_dict(P)
    (opt,), _ = m.configure_optimizers()
    for g in opt.param_groups:                              # the 2-rank run's lr (it scales with the per-rank batch)
        g["lr"] = g["lr"] / 2
    ref_grads = None
    for s in range(2):
        m.train_step_fused(x.cuda(), y.cuda())
        if s == 0:
            ref_grads = m.arena.grads.cpu()
        opt.step()
    torch.cuda.synchronize()
    ref = m.arena.params.cpu()
    assert abs(opt.param_groups[0]["lr"] - dp["lr"]) < 1e-15
    assert rel_err(dp["grads"], ref_grads) < 1e-6
    init = vit_som_amd.ViTClassifier(copy.deepcopy(cfg), device="cuda:0")
    init.load_state_dict(P)
    p0 = init.arena.params.cpu()
    moved = (ref - p0).abs() > 0
    assert rel_err((dp["params"] - p0)[moved], (ref - p0)[moved]) < 2e-3
    assert torch.allclose(dp["params"], ref, atol=0.25 * dp["lr"])
