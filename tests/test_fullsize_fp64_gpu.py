"""Full-size training steps against an fp64 reference on the device.

The shipped workloads at their real size -- c3 exactly as bench.py runs it, c1, c2, c4, c5 and the ViTClassifier -- one
training step replayed from the launch tape (the product path), compared with the oracle (oracle/vitsom_oracle.py)
evaluated in float64 on the GPU from the same parameters, input, iteration and BMUs.  At these sizes the product takes the
paths the small oracle tests stay below: the LayerNorm backward fused into the input-gradient GEMM (>= 32 row tiles), the
BMU pass on plane images (B >= 192), the forward as two half-batch chains (B >= 64), the weight-gradient split plans of
the real M, the launch tape at batch 512.  Every gradient is checked with rel_err AND tile_rel_err (helpers.py), so an
error confined to one 64 x 64 output tile -- a wrong edge tile, split count or epilogue -- is not diluted by the rest.

The parameters are O.init_params with N(0, 0.1) added to every bias, every LayerNorm weight and bias and the CLS token
(init_params leaves them at 1 / 0, where an epilogue reading the wrong column gives the same numbers), then moved by
three optimizer steps.

Bars: at most 4x the worst value measured on an MI355X for the case, never above the 1e-4 model bar; the measured values
are listed at BARS.  The whole file runs in about 15 s (13 s for the eight cases).
"""
import copy
import gc

import pytest
import torch
import torch.nn.functional as F

from helpers import rel_err, tile_rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
N_TRAIN, EST, IT = 50000, 9700, 1000        # bench.py's schedule: gamma_t > 0 (mid-ramp)
WARM = 3                                     # host-driven, host-driven, recorded: the measured step is a tape replay


def _som_cfg(C, img, p, E, depth, heads, DE, ddepth, map_size, classes, B):
    from oracle.gen_golden import make_config
    return make_config(C, img, p, E, depth, heads, DE, ddepth, map_size, classes, B, gamma=0.01, Tmax=4.0, Tmin=0.1,
                       total_epochs=500)


def _c3():
    import bench
    return bench.c3_config(512)


# name -> (model kind, config factory, batch, GEMM mode, expected product paths)
#   ln:     every block LayerNorm backward fused into its input-gradient GEMM
#   planes: the cosine BMU pass on plane images
CASES = {
    "c3": ("som", _c3, 512, "default", dict(ln=True, planes=True)),
    "c3_f32": ("som", _c3, 512, "f32", dict(ln=False, planes=False)),
    "c2": ("som", lambda: _som_cfg(3, 32, 4, 192, 12, 3, 96, 2, (24, 24), 0, 512), 512, "default", dict(ln=True, planes=True)),
    "c1": ("som", lambda: _som_cfg(1, 28, 2, 16, 4, 2, 4, 2, (24, 24), 0, 128), 128, "default", dict(ln=False, planes=False)),
    "c4": ("som", lambda: _som_cfg(3, 32, 4, 192, 12, 3, 96, 2, (4, 4), 100, 128), 128, "default", dict(ln=True, planes=False)),
    "c5": ("som", lambda: _som_cfg(3, 64, 4, 192, 12, 3, 96, 2, (40, 40), 200, 256), 256, "default", dict(ln=True, planes=True)),
    "vit_p2": ("cls", lambda: _som_cfg(3, 32, 2, 192, 12, 3, 96, 2, (2, 2), 100, 512), 512, "default", dict(ln=True)),
    "vit_p4": ("cls", lambda: _som_cfg(3, 32, 4, 192, 12, 3, 96, 2, (2, 2), 10, 128), 128, "default", dict(ln=True)),
}

# Bars, one family per case: at most 4x the worst value measured on an MI355X, never above the 1e-4 model bar.
#   rel / tile: rel_err / tile_rel_err of every gradient; out: max |out - ref| of the loss and of each output.
# Measured (worst gradient rel_err / tile_rel_err, and the parameter it was on):
#   c3      1.05e-5 / 1.44e-5  (blocks.10.norm1.weight / blocks.0.mlp.0.bias)     loss 4.6e-8  dist 2.0e-7  cls 2.2e-6  recon 2.3e-6
#   c3_f32  6.3e-7  / 7.7e-7   (cls_token / prototypes)                           loss 6.7e-8  dist 7.9e-8  cls 2.5e-6  recon 2.8e-6
#   c2      9.2e-6  / 1.11e-5  (decoder_blocks.1.norm1.weight / blocks.11.norm2.weight)  loss 4.0e-8  dist 1.9e-7  cls 1.2e-6  recon 1.5e-6
#   c1      8.4e-6  / 8.4e-6   (decoder_blocks.0.attn.qkv.bias)                  loss 1.4e-7  dist 3.5e-7  cls 8.4e-7  recon 1.87e-5
#   c4      8.7e-6  / 1.15e-5  (patch_embed.proj.weight / blocks.4.mlp.0.weight)  loss 4.9e-7  dist 1.5e-7  cls 1.7e-6  logits 4.9e-7
#   c5      2.63e-5 / 3.20e-5  (blocks.11.attn.qkv.bias / .weight)                loss 1.4e-7  dist 1.0e-7  cls 1.5e-6  logits 7.6e-7
#   vit_p2  9.3e-6  / 1.26e-5  (blocks.0.norm2.weight / blocks.1.norm1.weight)    loss 2.3e-7  cls 1.4e-6  logits 5.9e-7
#   vit_p4  8.8e-6  / 1.08e-5  (patch_embed.proj.weight / blocks.0.attn.qkv.weight)  loss 2.5e-8  cls 1.6e-6  logits 5.2e-7
# Every case runs the BMU policy on all rows with an fp64 gap above SURE_GAP (510 / 512 rows at c3, 254 / 256 at c5):
# no mismatch.
BARS = {
    "c3": dict(rel=4e-5, tile=5.5e-5, out=dict(loss=1.8e-7, dist=7.8e-7, cls=8.8e-6, recon=9.3e-6)),
    "c3_f32": dict(rel=2.5e-6, tile=3e-6, out=dict(loss=2.6e-7, dist=3.1e-7, cls=9.9e-6, recon=1.1e-5)),
    "c2": dict(rel=3.6e-5, tile=4.4e-5, out=dict(loss=1.5e-7, dist=7.6e-7, cls=4.9e-6, recon=5.9e-6)),
    "c1": dict(rel=3.3e-5, tile=3.3e-5, out=dict(loss=5.4e-7, dist=1.4e-6, cls=3.3e-6, recon=7.4e-5)),
    "c4": dict(rel=3.4e-5, tile=4.6e-5, out=dict(loss=1.9e-6, dist=5.9e-7, cls=6.8e-6, logits=1.9e-6)),
    "c5": dict(rel=1e-4, tile=1e-4, out=dict(loss=5.6e-7, dist=4.1e-7, cls=5.9e-6, logits=3e-6)),
    "vit_p2": dict(rel=3.7e-5, tile=5e-5, out=dict(loss=9.1e-7, cls=5.4e-6, logits=2.3e-6)),
    "vit_p4": dict(rel=3.5e-5, tile=4.3e-5, out=dict(loss=1e-7, cls=6.4e-6, logits=2e-6)),
}
SURE_GAP = 4e-6          # rows whose fp64 BMU is unambiguous in fp32: the step's BMU must be it


def _perturbed_params(cfg, seed):
    from oracle import vitsom_oracle as O
    P = O.init_params(cfg, seed=seed)
    g = torch.Generator().manual_seed(seed + 100)
    for k in O.trainable_keys(P):
        if k.endswith("bias") or "norm" in k or k == "vit.cls_token":
            P[k] = P[k] + 0.1 * torch.randn(P[k].shape, generator=g)
    return P


def _vit_config_of(som_cfg):
    """The configs/vit/*.yaml-shaped config of the same shapes (ViTClassifier)."""
    cfg = copy.deepcopy(som_cfg)
    cfg["hyperparameters"]["model_arch"] = "vit"
    del cfg["hyperparameters"]["gamma"], cfg["hyperparameters"]["som"]
    return cfg


def _free():
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _run_case(name):
    import vit_som_amd
    from oracle import vitsom_oracle as O
    from vit_som_amd import ops
    kind, make, B, _, expect = CASES[name]
    som_cfg = make()
    d = O.Dims(som_cfg)
    P = _perturbed_params(som_cfg, seed=7)
    if kind == "som":
        m = vit_som_amd.ViTSOM(copy.deepcopy(som_cfg), device=DEV)
        m.load_state_dict(P)
        m._it = IT
        to_oracle = {n: n for n, _ in m._named_trainable()}
    else:
        m = vit_som_amd.ViTClassifier(_vit_config_of(som_cfg), device=DEV)
        m.load_state_dict({("model." + k[4:] if k.startswith("vit.") else k): v for k, v in P.items()
                           if k.startswith(("vit.", "cls_head."))})
        to_oracle = {n: ("vit." + n[6:] if n.startswith("model.") else n) for n, _ in m._named_trainable()}
    m.set_schedule(N_TRAIN, EST)
    (opt,), _ = m.configure_optimizers()
    g = torch.Generator().manual_seed(11)
    xs = [torch.randn(B, d.C, d.img, d.img, generator=g).to(DEV) for _ in range(WARM + 1)]
    ys = [torch.randint(0, max(d.num_classes, 1), (B,), generator=g).to(DEV) for _ in range(WARM + 1)]
    vit = m._vit
    for i in range(WARM):
        m.train_step_fused(xs[i], ys[i])
        opt.step()
    torch.cuda.synchronize()
    a = vit._acts[B]
    tape0 = a.__dict__.get("tape")
    tape0 = tape0.id if tape0 is not None else 0
    it = m._it
    P64 = {}
    for k, v in m.state_dict().items():
        k = ("vit." + k[6:]) if k.startswith("model.") else k
        P64[k] = v.detach().to(DEV).double() if v.is_floating_point() else v.to(DEV)

    # ---- the measured step
    x, y = xs[WARM], ys[WARM]
    loss = float(m.train_step_fused(x, y))
    torch.cuda.synchronize()
    a = vit._acts[B]
    got = {n: m._grad_views[n].clone() for n in to_oracle}
    jobs = a.__dict__.get("ln_jobs")
    tape = a.__dict__.get("tape")
    paths = dict(tape=(tape.id if tape is not None else 0, tape0), fwd_split=vit._fwd_side is not None,
                 jobs=(jobs.n, jobs.flushed, sum(1 for k in jobs.keys[:jobs.n] if k[-1] == "fused")) if jobs else None,
                 ln_supported=[ops.linear_bwd_input_ln_supported(a.T, 3 * d.E, d.E), ops.linear_bwd_input_ln_supported(a.T, d.hidden, d.E)])
    if kind == "som":
        s = m._ctx[2]
        out = dict(dist=s.dist.clone(), cls=m._cls_view(a.xe, a).clone())
        bmu = s.bmu.clone()
        if m.classification:
            out["logits"] = a.logits.clone()
        else:
            out["recon"] = torch.empty_like(x)
            ops.l1_unpatchify(a.pred, x, torch.empty(1, device=DEV), recon=out["recon"], p=d.p)
            paths["ln_supported"] += [ops.linear_bwd_input_ln_supported(a.T, 3 * d.DE, d.DE),
                                      ops.linear_bwd_input_ln_supported(a.T, d.dhidden, d.DE)]
        paths["planes"] = m.som_layer._planes_used
        decoder = m._decoder_param_names() if m.classification else []
    else:
        c = m._ctx[2]
        out = dict(cls=c.xe.clone(), logits=c.logits.clone())
        decoder = m._decoder_param_names()
    del m, opt, a, vit
    _free()

    # ---- the fp64 reference on the device
    x64 = x.double()
    if kind == "som":
        total, parts, G = O.loss_and_grads(P64, x64, y, d, it, N_TRAIN, EST, bmu=bmu)
        ref = dict(dist=parts["dist"], cls=parts["cls"])
        ref.update({"logits": parts["logits"]} if d.classification else {"recon": parts["recon"]})
    else:
        keys = sorted(set(to_oracle.values()))
        leaves = {k: P64[k].clone().requires_grad_(True) for k in keys}
        Q = dict(P64)
        Q.update(leaves)
        feats, _ = O.vit_forward_features(Q, x64, d)
        logits = F.linear(feats, Q["cls_head.weight"], Q["cls_head.bias"])
        total = F.cross_entropy(logits, y)
        grads = torch.autograd.grad(total, [leaves[k] for k in keys], allow_unused=True)
        G = {k: (gr if gr is not None else torch.zeros_like(leaves[k])) for k, gr in zip(keys, grads)}
        ref = dict(cls=feats.detach(), logits=logits.detach())
        total = total.detach()
        parts = None
    errs = {"loss": abs(loss - float(total))}
    errs.update({k: float((out[k].double() - ref[k]).abs().max()) for k in out})
    sure_rows = None
    if kind == "som":
        top2 = parts["dist"].topk(2, dim=1, largest=False).values
        sure = (top2[:, 1] - top2[:, 0]) > SURE_GAP
        sure_rows = (int(sure.sum()), int((bmu[sure] != parts["bmu"][sure]).sum()), int((bmu != parts["bmu"]).sum()))
    gerr = {}
    for n, k in to_oracle.items():
        if n in decoder:
            gerr[n] = (float(got[n].abs().max()), None)
        else:
            gerr[n] = (rel_err(got[n], G[k]), tile_rel_err(got[n], G[k]))
    del G, parts, P64, ref, out, got
    _free()
    return dict(paths=paths, errs=errs, gerr=gerr, sure=sure_rows, decoder=decoder, expect=expect, kind=kind, B=B,
                d=d)


@pytest.mark.parametrize("name", list(CASES))
def test_full_size_step_against_fp64(name):
    from vit_som_amd import ops
    mode = CASES[name][3]
    prev = ops.get_gemm_mode()
    if mode == "f32":
        ops.set_gemm_mode(ops.GEMM_F32)
    try:
        r = _run_case(name)
    finally:
        ops.set_gemm_mode(prev)
        _free()
    bars, paths, expect, d = BARS[name], r["paths"], r["expect"], r["d"]
    trained = {n: e for n, e in r["gerr"].items() if e[1] is not None}
    worst_rel = max(trained.items(), key=lambda kv: kv[1][0])
    worst_tile = max(trained.items(), key=lambda kv: kv[1][1])
    print(f"\n[{name}] outputs {r['errs']} sure/mismatch/flipped {r['sure']} paths {paths}")
    print(f"[{name}] worst rel_err {worst_rel[1][0]:.3e} ({worst_rel[0]}), worst tile_rel_err {worst_tile[1][1]:.3e} ({worst_tile[0]})")
    for n, (e, t) in r["gerr"].items():
        print(f"[{name}]   {n:45s} rel {e:.3e} tile {t if t is None else format(t, '.3e')}")

    # the product paths ran
    tape, tape0 = paths["tape"]
    if r["kind"] == "som":
        assert tape == tape0 > 0, "the measured step was not a tape replay"
        assert paths["planes"] is expect["planes"]
    assert paths["fwd_split"]
    assert all(paths["ln_supported"]) is expect["ln"] and any(paths["ln_supported"]) is expect["ln"], paths["ln_supported"]
    n_jobs, flushed, fused = paths["jobs"]
    full_blocks = d.depth - 1 if r["kind"] == "cls" else d.depth + (0 if d.classification else d.ddepth)
    assert n_jobs == flushed > 0
    assert fused == (2 * full_blocks if expect["ln"] else 0), (fused, full_blocks)
    # loss, distances, BMU policy and outputs against fp64
    assert set(r["errs"]) == set(bars["out"])
    for k, e in r["errs"].items():
        assert e < bars["out"][k], (k, e)
    if r["sure"] is not None:
        n_sure, mismatched, _ = r["sure"]
        assert n_sure > 0.75 * r["B"] and mismatched == 0, r["sure"]
    # every gradient against fp64; the decoder of a classification step gets exactly zero
    for n, (e, t) in r["gerr"].items():
        if t is None:
            assert e == 0.0, n
        else:
            assert e < bars["rel"] and t < bars["tile"], (n, e, t)
    assert bool(r["decoder"]) == (r["kind"] == "cls" or d.classification)
