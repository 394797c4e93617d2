"""ViTClassifier on the MI355X: the single-query attention kernels against an fp64 restatement, the model against the
reference's own goldens (tests/golden/ref_vitcls_*, tools/gen_golden_vitcls.py) and an fp64 oracle composition at the
real head size, the pruned last block against the full one, evaluation, checkpoints, the driver and the full-size
vit_cifar-10 / vit_cifar-100 steps."""
import copy
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import GOLDEN, f32_close, rel_err

pytestmark = pytest.mark.gpu

GOLDENS = ["ref_vitcls_hd8", "ref_vitcls_hd32"]


def _golden(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
    return z, json.loads(str(z["config"]))


def _model(name):
    import vit_som_amd
    z, cfg = _golden(name)
    m = vit_som_amd.ViTClassifier(copy.deepcopy(cfg), device="cuda:0")
    m.load_state_dict({k: torch.from_numpy(z["param/" + k]) for k in (str(s) for s in z["state_keys"])})
    return z, cfg, m


def vit_config(C, img, p, E, depth, heads, num_classes, batch_size, DE=16, ddepth=1):
    """A configs/vit/*.yaml-shaped config."""
    from oracle.gen_golden import make_config
    cfg = make_config(C, img, p, E, depth, heads, DE, ddepth, (1, 1), num_classes, batch_size)
    cfg["hyperparameters"]["model_arch"] = "vit"
    del cfg["hyperparameters"]["gamma"], cfg["hyperparameters"]["som"]
    return cfg


# ------------------------------------------------------------------------------------ kernel
def _q1_ref(q, kv, do, B, N, H, hd):
    E = H * hd
    q = q.double().view(B, H, hd)
    k = kv.double().view(B, N, 2, H, hd)[:, :, 0].permute(0, 2, 1, 3)          # [B, H, N, hd]
    v = kv.double().view(B, N, 2, H, hd)[:, :, 1].permute(0, 2, 1, 3)
    q.requires_grad_(True); k.requires_grad_(True); v.requires_grad_(True)
    s = torch.einsum("bhd,bhnd->bhn", q, k) * hd ** -0.5
    lse = torch.logsumexp(s, dim=-1)
    o = torch.einsum("bhn,bhnd->bhd", torch.softmax(s, dim=-1), v)
    o.backward(do.double().view(B, H, hd))
    dkv = torch.stack([k.grad.permute(0, 2, 1, 3), v.grad.permute(0, 2, 1, 3)], dim=2).reshape(B * N, 2 * E)
    return o.detach().reshape(B, E), lse.detach(), q.grad.reshape(B, E), dkv


@pytest.mark.parametrize("B,N,H,hd", [(3, 5, 3, 8), (7, 37, 2, 8), (5, 17, 2, 32), (16, 65, 3, 64), (8, 197, 3, 64),
                                      (4, 257, 3, 64)])
def test_attention_q1_against_fp64(B, N, H, hd):
    from vit_som_amd import ops
    E = H * hd
    g = torch.Generator().manual_seed(B * 1000 + N)
    q, kv, do = (torch.randn(B, E, generator=g), torch.randn(B * N, 2 * E, generator=g), torch.randn(B, E, generator=g))
    ro, rlse, rdq, rdkv = _q1_ref(q, kv, do, B, N, H, hd)
    qd, kvd, dod = q.cuda(), kv.cuda(), do.cuda()
    runs = []
    for _ in range(2):
        o, lse = torch.full((B, E), float("nan"), device="cuda"), torch.full((B, H), float("nan"), device="cuda")
        dq, dkv = torch.full((B, E), float("nan"), device="cuda"), torch.full((B * N, 2 * E), float("nan"), device="cuda")
        ops.attention_q1_fwd(qd, kvd, o, lse, B, N, H, hd)
        ops.attention_q1_bwd(dod, o, lse, qd, kvd, dq, dkv, B, N, H, hd)
        torch.cuda.synchronize()
        runs.append([t.cpu() for t in (o, lse, dq, dkv)])
    for got, ref in zip(runs[0], (ro, rlse, rdq, rdkv)):
        assert torch.isfinite(got).all()
        assert rel_err(got, ref) <= 1e-5, rel_err(got, ref)
    for a, b in zip(*runs):
        assert torch.equal(a, b), "two launches differ"


def test_attention_q1_rejects_bad_shapes():
    from vit_som_amd._lib import lib, ptr, stream
    B, N, H = 2, 5, 2
    buf = torch.zeros(B * N * 2 * H * 64, device="cuda")
    p = ptr(buf)
    for hd in (4, 12, 128):
        assert lib.vsom_attention_q1_fwd(p, p, p, p, B, N, H, hd, stream()) == -1
        assert lib.vsom_attention_q1_bwd(p, p, p, p, p, p, p, B, N, H, hd, stream()) == -1
    for b, n, h in ((0, N, H), (B, 0, H), (B, N, 0)):
        assert lib.vsom_attention_q1_fwd(p, p, p, p, b, n, h, 8, stream()) == -1
        assert lib.vsom_attention_q1_bwd(p, p, p, p, p, p, p, b, n, h, 8, stream()) == -1
    assert lib.vsom_attention_q1_fwd(None, p, p, p, B, N, H, 8, stream()) == -1


# ------------------------------------------------------------------------------------ reference goldens
@pytest.mark.parametrize("name", GOLDENS)
def test_forward_and_validation_match_reference_golden(name):
    z, cfg, m = _model(name)
    logits = m(torch.from_numpy(z["x0"]).cuda())
    assert float((logits.cpu() - torch.from_numpy(z["logits"])).abs().max()) < 2e-5
    x1, y1 = torch.from_numpy(z["x1"]).cuda(), torch.from_numpy(z["y1"]).cuda()
    vloss = m.validation_step((x1, y1), 0)
    assert abs(float(vloss) - float(z["val_loss"])) < 5e-5
    assert float(m._last["acc"]) == float(z["val_acc"])
    _, pl = m.predict(x1)
    assert torch.equal(pl, m(x1))


@pytest.mark.parametrize("name", GOLDENS)
def test_training_step_grads_match_reference_golden(name):
    z, cfg, m = _model(name)
    loss = m.training_step((torch.from_numpy(z["x0"]).cuda(), torch.from_numpy(z["y0"]).cuda()), 0)
    loss.backward()
    torch.cuda.synchronize()
    assert abs(float(loss) - float(z["loss"])) < 2e-5
    none = {str(s) for s in z["grad_none"]}
    assert none and all(n.startswith("model.decoder_") for n in none)
    for n, p in m.named_parameters():
        if not p.requires_grad:
            continue
        g = p.grad.cpu()
        if n in none:
            assert not g.any(), n
        else:
            ref = torch.from_numpy(z["grad/" + n])
            assert rel_err(g, ref) < 1e-4 or float((g - ref).abs().max()) < 1e-9, (n, rel_err(g, ref))


@pytest.mark.parametrize("name", GOLDENS)
def test_three_optimizer_steps_match_reference_golden(name):
    z, cfg, m = _model(name)
    dec0 = {n: p.detach().clone() for n, p in m.named_parameters() if n.startswith("model.decoder_")}
    (opt,), _ = m.configure_optimizers()
    for step in range(3):
        x, y = torch.from_numpy(z[f"x{step}"]).cuda(), torch.from_numpy(z[f"y{step}"]).cuda()
        if step == 1:
            m.train_step_fused(x, y)
        else:
            m.training_step((x, y), step).backward()
        opt.step()
        if step in (0, 2):
            torch.cuda.synchronize()
            for n, p in m.named_parameters():
                if p.requires_grad:
                    assert f32_close(p.detach().cpu().numpy(), z[f"step{step + 1}/" + n], 1e-5), (step, n)
    for n, p in m.named_parameters():
        if n in dec0:
            assert torch.equal(p.detach(), dec0[n]), n


# ------------------------------------------------------------------------------------ oracle at the real head size
@pytest.mark.parametrize("img,p", [(32, 4), (32, 2)])
def test_real_head_size_against_fp64_oracle(img, p):
    import vit_som_amd
    from oracle import vitsom_oracle as O
    from oracle.gen_golden import make_config
    som_cfg = make_config(3, img, p, 192, 3, 3, 96, 1, (2, 2), 10, 8)
    d = O.Dims(som_cfg)
    P = O.init_params(som_cfg, seed=5)
    g = torch.Generator().manual_seed(6)
    with torch.no_grad():
        for k, v in P.items():
            if k.endswith("bias") or "norm" in k:
                v.add_(0.1 * torch.randn(v.shape, generator=g))
    x, y = torch.randn(8, 3, img, img, generator=g), torch.randint(0, 10, (8,), generator=g)
    cfg = vit_config(3, img, p, 192, 3, 3, 10, 8, DE=96)
    m = vit_som_amd.ViTClassifier(cfg, device="cuda:0")
    sd = {("model." + k[4:] if k.startswith("vit.") else k): v for k, v in P.items() if k.startswith(("vit.", "cls_head."))}
    m.load_state_dict(sd)
    P64 = {k: v.double().requires_grad_(v.is_floating_point()) for k, v in P.items()}
    feats, _ = O.vit_forward_features(P64, x.double(), d)
    ref_loss = F.cross_entropy(F.linear(feats, P64["cls_head.weight"], P64["cls_head.bias"]), y)
    ref_loss.backward()
    loss = m.training_step((x.cuda(), y.cuda()), 0)
    loss.backward()
    torch.cuda.synchronize()
    assert abs(float(loss) - float(ref_loss)) / abs(float(ref_loss)) < 1e-4
    for n, q in m.named_parameters():
        if not q.requires_grad or n.startswith("model.decoder_"):
            continue
        ref = P64[("vit." + n[6:]) if n.startswith("model.") else n].grad
        assert rel_err(q.grad.cpu(), ref) < 1e-4, (n, rel_err(q.grad.cpu(), ref))


# ------------------------------------------------------------------------------------ pruned against full
def _run(m, x, y, steps=1):
    """-> (first loss, first step's gradient arena, parameters after `steps` steps)."""
    (opt,), _ = m.configure_optimizers()
    first = None
    for _ in range(steps):
        loss = m.train_step_fused(x, y)
        if first is None:
            first = (float(loss), m.arena.grads.cpu())
        opt.step()
    torch.cuda.synchronize()
    return first[0], first[1], m.arena.params.cpu()


@pytest.mark.parametrize("img,p,E,H,B", [(8, 4, 24, 3, 5), (32, 4, 192, 3, 64)])
def test_pruned_last_block_equals_full_block(img, p, E, H, B):
    import vit_som_amd
    from vit_som_amd.tuning import hooks
    cfg = vit_config(3, img, p, E, 3, H, 10, B)
    g = torch.Generator().manual_seed(1)
    x, y = torch.randn(B, 3, img, img, generator=g).cuda(), torch.randint(0, 10, (B,), generator=g).cuda()
    torch.manual_seed(0)
    m0 = vit_som_amd.ViTClassifier(copy.deepcopy(cfg), device="cuda:0")
    sd = {k: v.clone() for k, v in m0.state_dict().items()}
    out = {}
    try:
        for prune in (True, False, True):
            hooks.set(cls_prune=prune)
            m = vit_som_amd.ViTClassifier(copy.deepcopy(cfg), device="cuda:0")
            m.load_state_dict(sd)
            out.setdefault(prune, []).append(_run(m, x, y, steps=3))
            m.load_state_dict(sd)
            logits = m(x)
            out.setdefault(("logits", prune), logits.cpu())
    finally:
        hooks.reset()
    (lp, gp, pp), (lf, gf, pf) = out[True][0], out[False][0]
    assert abs(lp - lf) / abs(lf) < 1e-5
    assert rel_err(out[("logits", True)], out[("logits", False)]) < 1e-5
    # per-parameter gradients of the first step
    m = vit_som_amd.ViTClassifier(copy.deepcopy(cfg), device="cuda:0")
    for n, _ in m._named_trainable():
        lo, k, _ = m.arena.offsets[n]
        a, b = gp[lo:lo + k], gf[lo:lo + k]
        assert rel_err(a, b) < 1e-5 or float((a - b).abs().max()) < 1e-9, (n, rel_err(a, b))
    # three steps repeated from the same state: the same bits
    assert torch.equal(out[True][0][2], out[True][1][2])
    assert torch.equal(out[True][0][1], out[True][1][1])


# ------------------------------------------------------------------------------------ evaluation, checkpoints, driver
def test_evaluate_classification_equals_sklearn_on_argmax():
    from sklearn.metrics import accuracy_score, precision_recall_fscore_support
    from vit_som_amd.evaluation import evaluate_classification
    from vit_som_amd.train import TensorLoader
    z, cfg, m = _model("ref_vitcls_hd32")
    g = torch.Generator().manual_seed(3)
    d = cfg["data"]
    x = torch.randn(60, d["num_channels"], d["input_size"], d["input_size"], generator=g)
    y = torch.randint(0, d["num_classes"], (60,), generator=g)
    loader = TensorLoader(x, y, 12)
    acc, prec, rec, f1, _ = evaluate_classification(m, cfg, loader)
    pred = torch.cat([m(xb.cuda()).argmax(-1).cpu() for xb, _ in loader]).numpy()
    yt = y.numpy()
    assert acc == pytest.approx(accuracy_score(yt, pred), abs=1e-12)
    # the reference's evaluation.py: macro averages, zero_division=nan (a class never predicted is left out)
    p_, r_, f_, _ = precision_recall_fscore_support(yt, pred, average="macro", zero_division=np.nan)
    assert prec == pytest.approx(p_, abs=1e-12)
    assert rec == pytest.approx(r_, abs=1e-12)
    assert f1 == pytest.approx(f_, abs=1e-12)


def test_checkpoint_roundtrip_gives_identical_logits(tmp_path):
    import vit_som_amd
    z, cfg, m = _model("ref_vitcls_hd8")
    (opt,), (sched,) = m.configure_optimizers()
    x, y = torch.from_numpy(z["x0"]).cuda(), torch.from_numpy(z["y0"]).cuda()
    m.train_step_fused(x, y)
    opt.step()
    path = m.save_checkpoint(str(tmp_path / "vit.ckpt"), opt, sched, epoch=0)
    ck = torch.load(path, weights_only=True)
    assert set(ck["state_dict"]) == {str(s) for s in z["state_keys"]}
    m2 = vit_som_amd.ViTClassifier.load_from_checkpoint(path, config=cfg)
    assert torch.equal(m(x), m2(x))


def test_driver_trains_the_vit_baseline(tmp_path):
    from vit_som_amd import train
    cfg = vit_config(3, 32, 4, 48, 2, 3, 10, 32)
    cfg["data"]["dataset"] = "synthetic"
    metrics = train.main(cfg, n_runs=1, max_epochs=2, model_states_dir=str(tmp_path / "states"),
                         make_loaders=lambda c, r, w: train.synthetic_loaders(c, r, w, n_train=256, n_val=64, n_test=64))
    for k in ("accuracy", "precision", "recall", "f1", "run_duration", "inference_time"):
        assert len(metrics[k]) == 1 and np.isfinite(metrics[k][0]), k
    assert os.path.exists(tmp_path / "states" / "vit_synthetic_best.ckpt")


# ------------------------------------------------------------------------------------ full size
@pytest.mark.parametrize("p,B,classes", [(4, 128, 10), (2, 512, 100)])
def test_full_size_vit_configs_step_and_learn(p, B, classes):
    import vit_som_amd
    cfg = vit_config(3, 32, p, 192, 12, 3, classes, B, DE=96, ddepth=2)
    torch.manual_seed(0)
    m = vit_som_amd.ViTClassifier(cfg, device="cuda:0")
    (opt,), _ = m.configure_optimizers()
    for grp in opt.param_groups:
        grp["lr"] = 1e-4
    g = torch.Generator().manual_seed(2)
    x, y = torch.randn(B, 3, 32, 32, generator=g).cuda(), torch.randint(0, classes, (B,), generator=g).cuda()
    losses = []
    for _ in range(20):
        losses.append(m.train_step_fused(x, y).clone())
        opt.step()
    losses = [float(v) for v in losses]
    assert all(np.isfinite(losses)), losses
    assert losses[-1] < 0.99 * losses[0], losses
