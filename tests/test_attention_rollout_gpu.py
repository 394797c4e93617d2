"""Attention rollout on the GPU: the step and the chain against the fp64 restatement under the project's accuracy rule,
numeric edges, determinism, no alignment requirement, the memory contract, no N x N matrix, the model methods and
evaluate_attention with its figures.

The accuracy rule (numeric_edges.py): with e = max_b max_j |got - ref64| / max_j ref64, require e <= max(FLOOR, 4 e32), e32
the same metric of the plain fp32 torch restatement on the CPU and FLOOR = 3e-6, the bound vsom_attention_probs is held to.
Every case prints `rollout-figures` lines with the largest e and e32 it saw."""
import copy
import functools

import numpy as np
import pytest
import torch

import attention_rollout_ref as R
import memcheck
import numeric_edges as NE

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

STEP_SHAPES = [(3, 5, 2, 8), (2, 64, 1, 16), (2, 65, 3, 64), (1, 130, 1, 16), (2, 197, 2, 8), (2, 257, 3, 64), (2, 1, 2, 64)]
ALPHAS = (0.5, 1.0)
QUERY_KINDS = ("cls", "patches", "random")


def _qkv(B, N, H, hd, seed=0, scale=1.0):
    return torch.randn(B * N, 3 * H * hd, generator=torch.Generator().manual_seed(seed)) * scale


@functools.lru_cache(maxsize=None)
def _probs(shape, seed, scale):
    """(qkv, P64, P32) of one block on the CPU, computed once per shape."""
    qkv = _qkv(*shape, seed=seed, scale=scale)
    return qkv, R.probabilities(qkv, *shape, torch.float64), R.probabilities(qkv, *shape, torch.float32)


def _report(what, shape, e, e32):
    print(f"rollout-figures {what} {'x'.join(map(str, shape))}: e {e:.3e} e32 {e32:.3e} bound {R.bound(e32):.3e}")


def _check(got, ref, y32, N, total=None):
    """The rule, and every row's sum within N x the bound of the query's weight (the bound in the rule's own unit: the
    row's largest reference value)."""
    assert bool(torch.isfinite(got).all())
    e, e32 = R.row_scaled_error(got, ref), R.row_scaled_error(y32, ref)
    assert e <= R.bound(e32), (e, e32)
    if total is not None:
        peak = ref.double().max(dim=1).values
        assert bool(((got.double().cpu().sum(1) - total.double()).abs() <= N * R.bound(e32) * peak).all())
    return e, e32


# ---------------------------------------------------------------- one step against fp64
@pytest.mark.parametrize("shape", STEP_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_one_step_against_fp64(shape):
    from vit_som_amd import ops
    B, N, H, hd = shape
    qkv, P64, P32 = _probs(shape, 1, 1.0)
    dq = qkv.to(DEV)
    worst = (0.0, 0.0)
    for kind in QUERY_KINDS:
        w = R.query(kind, B, N, seed=2)
        dw = w.to(DEV)
        for fusion in R.FUSIONS:
            for alpha in ALPHAS:
                out = torch.full((B, N), float("nan"), device=DEV)
                got = ops.attention_rollout_step(dq, dw, out, B, N, H, hd, fusion, alpha).cpu()
                ref = R.step_from_probs(P64, w, fusion, alpha)
                y32 = R.step_from_probs(P32, w, fusion, alpha)
                worst = max(worst, _check(got, ref, y32, N, w.sum(1)))
    _report("step", shape, *worst)


def test_fusion_codes_and_one_head():
    from vit_som_amd import ops
    B, N, H, hd = 2, 65, 1, 16
    dq, dw = _qkv(B, N, H, hd, 3).to(DEV), R.query("random", B, N, 4).to(DEV)
    outs = [ops.attention_rollout_step(dq, dw, torch.empty(B, N, device=DEV), B, N, H, hd, f, 0.5) for f in ("mean", "max", "min", 0, 1, 2)]
    assert torch.equal(outs[1], outs[0])                     # one head: the three fusions are the same matrix
    assert R.row_scaled_error(outs[2], outs[0]) <= R.FLOOR   # the minimum goes through logarithms: the same to rounding
    for name, code in ((0, 3), (1, 4), (2, 5)):
        assert torch.equal(outs[name], outs[code])           # a name and its code are one call
    with pytest.raises(ValueError, match="fusion: expected one of"):
        ops.attention_rollout_step(dq, dw, torch.empty(B, N, device=DEV), B, N, H, hd, "median", 0.5)
    with pytest.raises(ValueError, match="v_out: expected"):
        ops.attention_rollout_step(dq, dw, torch.empty(B, N + 1, device=DEV), B, N, H, hd, "mean", 0.5)


# ---------------------------------------------------------------- a chain of blocks
@pytest.mark.parametrize("shape", [(2, 65, 3, 64), (2, 197, 2, 8)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("scale", [1.0, 3.0])
def test_chain_of_blocks(shape, scale):
    from vit_som_amd import ops
    B, N, H, hd = shape
    blocks = [_probs(shape, 20 + i, scale) for i in range(12)]
    dev = [b[0].to(DEV) for b in blocks]
    w = R.query("cls", B, N)
    dw = w.to(DEV)
    worst = (0.0, 0.0)
    for depth in (1, 2, 12):
        for fusion, alpha in (("mean", 0.5), ("max", 0.5), ("min", 1.0)):
            got = ops.attention_rollout(dev[:depth], dw, H, hd, fusion, alpha)
            assert got.data_ptr() != dw.data_ptr() and torch.equal(dw.cpu(), w)          # a fresh tensor; w is not written
            ref, y32 = w.double(), w.float()
            for _, P64, P32 in reversed(blocks[:depth]):
                ref, y32 = R.step_from_probs(P64, ref, fusion, alpha), R.step_from_probs(P32, y32, fusion, alpha)
            worst = max(worst, _check(got.cpu(), ref, y32, N, w.sum(1)))
    _report(f"chain-scale{scale:g}", shape, *worst)


# ---------------------------------------------------------------- numeric edges
EDGE_CASES = [(s, k) for s, k in NE.attention_ids([(2, 65, 2, 64), (2, 197, 2, 64), (2, 17, 2, 8)])]


@pytest.mark.parametrize("shape,kind", EDGE_CASES, ids=[f"{'x'.join(map(str, s))}-{k}" for s, k in EDGE_CASES])
def test_numeric_edges(shape, kind):
    from vit_som_amd import ops
    B, N, H, hd = shape
    case = NE.attention_case(shape, kind)
    qkv = case.inp["qkv"].reshape(B * N, 3 * H * hd)
    P64, P32 = R.probabilities(qkv, *shape, torch.float64), R.probabilities(qkv, *shape, torch.float32)
    assert float((P64 - case.ref["probs"]).abs().max()) < 1e-12             # the restatement's softmax is numeric_edges' own
    dq = qkv.to(DEV)
    w = R.query("patches", B, N)
    worst = (0.0, 0.0)
    for fusion in R.FUSIONS:
        for alpha in ALPHAS:
            got = ops.attention_rollout_step(dq, w.to(DEV), torch.empty(B, N, device=DEV), B, N, H, hd, fusion, alpha).cpu()
            ref, y32 = R.step_from_probs(P64, w, fusion, alpha), R.step_from_probs(P32, w, fusion, alpha)
            e, e32 = _check(got, ref, y32, N, w.sum(1))
            worst = max(worst, (e, e32))
            if kind in ("sat_first", "sat_last"):
                # the concentration the fp64 reference itself shows: the dominant key's column holds the share it holds there,
                # and where the reference's largest column leads its runner-up clearly it is the kernel's largest too
                dom = 0 if kind == "sat_first" else N - 1
                share, want = got.double()[:, dom] / got.double().sum(1), ref[:, dom] / ref.sum(1)
                assert bool(((share - want).abs() <= N * R.bound(e32)).all()), (share, want)
                top = ref.topk(2, dim=1)
                clear = (top.values[:, 0] - top.values[:, 1]) > 2 * R.bound(e32) * top.values[:, 0]
                assert bool((got.argmax(1)[clear] == top.indices[clear, 0]).all())
                if fusion == "mean":
                    assert bool((top.indices[:, 0] == dom).all()) and bool(clear.all())        # the reference does concentrate there
    _report(f"edge-{kind}", shape, *worst)


# ---------------------------------------------------------------- determinism
def test_bits_do_not_depend_on_the_batch():
    from vit_som_amd import ops
    B, N, H, hd = 5, 65, 3, 64
    qkv, w = _qkv(B, N, H, hd, 7).to(DEV), R.query("random", B, N, 8).to(DEV)
    run = lambda q, v: ops.attention_rollout_step(q.contiguous(), v.contiguous(), torch.empty_like(v), v.shape[0], N, H, hd, "max", 0.5)   # noqa: E731
    first = run(qkv, w)
    assert torch.equal(run(qkv, w), first)                                   # the same call twice
    q3 = qkv.view(B, N, -1)
    for b in range(B):                                                       # a sample alone is its row of the batch
        assert torch.equal(run(q3[b].reshape(N, -1), w[b:b + 1]), first[b:b + 1]), b
    perm = torch.tensor([3, 0, 4, 1, 2], device=DEV)
    assert torch.equal(run(q3[perm].reshape(B * N, -1), w[perm]), first[perm])
    chain = [_qkv(B, N, H, hd, 30 + i).to(DEV) for i in range(3)]
    assert torch.equal(ops.attention_rollout(chain, w, H, hd), ops.attention_rollout(chain, w, H, hd))


def test_no_alignment_requirement():
    from vit_som_amd import ops
    for shape in [(2, 65, 3, 64), (2, 17, 2, 8)]:
        B, N, H, hd = shape
        qkv, w = _qkv(*shape, seed=9).to(DEV), R.query("random", B, N, 10).to(DEV)
        store = torch.empty(qkv.numel() + 1, device=DEV)
        off = store[1:].view_as(qkv)
        off.copy_(qkv)
        assert qkv.data_ptr() % 16 == 0 and off.data_ptr() % 16 == 4
        for fusion in R.FUSIONS:
            a = ops.attention_rollout_step(qkv, w, torch.empty_like(w), B, N, H, hd, fusion, 0.5)
            b = ops.attention_rollout_step(off, w, torch.empty_like(w), B, N, H, hd, fusion, 0.5)
            assert torch.equal(a, b), (shape, fusion)


# ---------------------------------------------------------------- memory
@pytest.mark.parametrize("shape", [(3, 5, 2, 8), (2, 65, 3, 64), (2, 257, 3, 64)], ids=lambda s: "x".join(map(str, s)))
def test_memory_contract(shape, monkeypatch):
    from vit_som_amd import ops
    B, N, H, hd = shape
    qkv, w = _qkv(*shape, seed=11).to(DEV), R.query("random", B, N, 12).to(DEV)
    want = ops.attention_rollout_step(qkv, w, torch.empty_like(w), B, N, H, hd, "mean", 0.5)
    scratch = memcheck.ExactScratch(memcheck.FILL_FF)
    monkeypatch.setattr(ops, "scratch", scratch)
    gq, hq = memcheck.guarded_copy(qkv)                    # what surrounds the inputs reads as NaN
    gw, hw = memcheck.guarded_copy(w)
    out, h = memcheck.guarded((B, N), torch.float32, DEV)
    ops.attention_rollout_step(gq, gw, out, B, N, H, hd, "mean", 0.5)
    torch.cuda.synchronize()
    assert scratch.calls == 1 and [k[2] for k in scratch.arenas] == [ops.attention_rollout_ws_size(B, N, H, hd)]
    scratch.check()
    for handle, what in ((h, "v_out"), (hq, "qkv"), (hw, "v_in")):
        handle.check(what)
    h.all_written("v_out")
    assert torch.equal(out, want)


def test_no_n_by_n_matrix_is_allocated():
    from vit_som_amd import ops
    B, N, H, hd = 64, 257, 3, 64
    g = torch.Generator(device=DEV).manual_seed(0)
    qkvs = [torch.randn(B * N, 3 * H * hd, device=DEV, generator=g) for _ in range(2)]
    w = R.query("cls", B, N).to(DEV)
    warm = ops.attention_rollout(qkvs, w, H, hd)
    torch.cuda.synchronize()
    del warm
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = ops.attention_rollout(qkvs, w, H, hd)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    assert rise < B * H * N * N * 4, rise
    assert rise <= 4 * B * N * 4                            # two [B, N] buffers (the allocator rounds each up)
    assert float((out.sum(1) - 1).abs().max()) < 1e-4


# ---------------------------------------------------------------- the models
def _som_config(use_reduced=False, classes=5):
    from oracle.gen_golden import make_config
    cfg = make_config(3, 16, 4, 48, 3, 3, 24, 1, (3, 4), classes, 8)
    cfg["hyperparameters"]["som"]["use_reduced"] = use_reduced
    return cfg


def _sharpen(vit):
    """Fresh xavier weights give nearly uniform attention; larger q / k projections give every row a shape of its own."""
    with torch.no_grad():
        for blk in vit.blocks:
            blk.attn.qkv.weight.mul_(6.0)


@pytest.fixture(scope="module")
def tiny():
    import vit_som_amd
    torch.manual_seed(0)
    cfg = _som_config()
    m = vit_som_amd.ViTSOM(copy.deepcopy(cfg), device=DEV)
    _sharpen(m.vit)
    x = torch.randn(6, 3, 16, 16, generator=torch.Generator().manual_seed(1)).to(DEV)
    with torch.no_grad():
        attns = [a.cpu() for a in m.vit.forward(x, return_attns=True)[3]]
    return m, cfg, x, attns


def test_model_rollout_against_the_chain_over_the_attention_maps(tiny):
    m, cfg, x, attns = tiny
    vit = m.vit
    B, N, L = x.shape[0], 17, len(vit.blocks)
    assert len(attns) == L == 3 and attns[0].shape == (B, 3, N, N)
    assert float(attns[0].max()) > 0.2                                       # not the uniform 1 / 17
    tq = torch.rand(N, generator=torch.Generator().manual_seed(2))
    tq2 = torch.rand(B, N, generator=torch.Generator().manual_seed(3))
    worst = (0.0, 0.0)
    for query, w in (("cls", R.query("cls", B, N)), ("patches", R.query("patches", B, N)), (5, torch.eye(N)[5].expand(B, N)),
                     (tq, tq.expand(B, N)), (tq2.to(DEV), tq2)):
        for fusion, residual, start in (("mean", 0.5, 0), ("max", 0.5, 1), ("min", 0.25, 0), ("mean", 0.0, 2)):
            got = vit.attention_rollout(x, query, fusion, residual, start)
            assert got.shape == (B, N) and got.dtype == torch.float32
            ref = R.rollout_from_maps(attns, w, fusion, 1 - residual, start, torch.float64)
            y32 = R.rollout_from_maps(attns, w, fusion, 1 - residual, start, torch.float32)
            worst = max(worst, _check(got.cpu(), ref, y32, N, w.sum(1)))
    _report("model", (B, N, 3, 16), *worst)
    # alpha = 1 from the last block: the head-mean CLS row of the last map
    got = vit.attention_rollout(x, "cls", "mean", 0.0, L - 1).cpu()
    want = attns[-1].double().mean(1)[:, 0]
    assert R.row_scaled_error(got, want) <= R.FLOOR
    assert vit.patch_map(got).shape == (B, 4, 4) and torch.equal(vit.patch_map(got).reshape(B, -1), got[:, 1:])
    with pytest.raises(ValueError, match="query must be non-negative"):
        vit.attention_rollout(x, -tq)
    with pytest.raises(ValueError, match=r"query must be 'cls', 'patches', a token index in \[0, 17\)"):
        vit.attention_rollout(x, 17)


def test_vitsom_default_query_follows_use_reduced(tiny):
    import vit_som_amd
    m, cfg, x, _ = tiny
    assert torch.equal(m.attention_rollout(x), m.vit.attention_rollout(x, "patches"))
    assert torch.equal(m.attention_rollout(x, query="cls"), m.vit.attention_rollout(x, "cls"))
    red = _som_config(use_reduced=True)
    mr = vit_som_amd.ViTSOM(copy.deepcopy(red), device=DEV)
    _sharpen(mr.vit)
    assert torch.equal(mr.attention_rollout(x), mr.vit.attention_rollout(x, "cls"))
    assert not torch.equal(mr.attention_rollout(x), mr.vit.attention_rollout(x, "patches"))


def _vit_config(classes=5):
    cfg = _som_config(classes=classes)
    cfg["hyperparameters"]["model_arch"] = "vit"
    del cfg["hyperparameters"]["gamma"], cfg["hyperparameters"]["som"]
    return cfg


def test_classifier_rollout_does_not_depend_on_cls_prune(tiny):
    import vit_som_amd
    from vit_som_amd.tuning import hooks
    _, _, x, _ = tiny
    torch.manual_seed(3)
    m = vit_som_amd.ViTClassifier(_vit_config(), device=DEV)
    _sharpen(m.model)
    out = {}
    try:
        for prune in (True, False):
            hooks.set(cls_prune=prune)
            m.predict(x)                                                     # the pruned forward leaves the last qkv stale
            out[prune] = m.attention_rollout(x).clone()
    finally:
        hooks.reset()
    assert torch.equal(out[True], out[False])
    assert torch.equal(out[True], m.model.attention_rollout(x, "cls"))
    assert float((out[True].sum(1) - 1).abs().max()) < 1e-5


# ---------------------------------------------------------------- evaluate_attention and the figures
def _loader(sizes=(6, 6, 3), classes=5):
    g = torch.Generator().manual_seed(4)
    return [(torch.randn(b, 3, 16, 16, generator=g), torch.randint(0, classes, (b,), generator=g)) for b in sizes]


def test_evaluate_attention_folds_are_add_at_bit_for_bit(tiny, tmp_path):
    from vit_som_amd import attention_rollout as AR
    m, cfg, _, _ = tiny
    loader = _loader()
    report = AR.evaluate_attention(m, cfg, loader)
    K, C, n = 12, 5, 16
    csum, usum = np.zeros((C, n)), np.zeros((K, n))
    ccount, ucount = np.zeros(C, dtype=np.int64), np.zeros(K, dtype=np.int64)
    ent, cls = [], []
    for x, y in loader:
        x = x.to(DEV)
        r = m.attention_rollout(x)                                           # the default query: what the SOM is fed
        p, c = AR.patch_distribution(r)
        bmu = m.predict(x)[0].cpu().numpy()
        p = p.cpu().numpy().astype(np.float64)
        np.add.at(csum, y.numpy(), p)
        np.add.at(usum, bmu, p)
        np.add.at(ccount, y.numpy(), 1)
        np.add.at(ucount, bmu, 1)
        ent += list(-(p * np.log(np.where(p > 0, p, 1.0))).sum(1) / np.log(n))
        cls += list(c.cpu().numpy().astype(np.float64))
    assert report.n_samples == 15 and report.query == "patches" and report.head_fusion == "mean" and report.residual == 0.5
    assert report.class_counts.sum() == 15 and report.unit_counts.sum() == 15
    assert np.array_equal(report.class_counts, ccount) and np.array_equal(report.unit_counts, ucount)
    # the sums are np.add.at's, bit for bit; the maps are those sums over the counts, so maps x counts is the sum
    assert report.class_sums.dtype == np.float64 and np.array_equal(report.class_sums.reshape(C, n), csum)
    assert np.array_equal(report.unit_sums.reshape(K, n), usum)
    for maps, sums, counts in ((report.class_maps, csum, ccount), (report.unit_maps, usum, ucount)):
        has = counts > 0
        assert np.array_equal(maps.reshape(len(counts), n)[has], sums[has] / counts[has][:, None])
        assert not maps.reshape(len(counts), n)[~has].any()
        assert np.allclose(maps.reshape(len(counts), n)[has] * counts[has][:, None], sums[has], rtol=4e-16, atol=0)
        assert np.allclose(maps.reshape(len(counts), n)[has].sum(1), 1.0, atol=1e-6)
    assert report.mean_map.shape == (4, 4) and abs(report.mean_map.sum() - 1) < 1e-6
    assert 0.0 < report.entropy <= 1.0 and abs(report.entropy - np.mean(ent)) < 1e-6
    assert 0.0 <= report.cls_mass < 1.0 and abs(report.cls_mass - np.mean(cls)) < 1e-6
    # the two figures
    rep2, path = AR.visualize_attention_map(m, cfg, loader, output_dir=str(tmp_path))
    assert path == str(tmp_path / "vit_som_attention_map.png") and (tmp_path / "vit_som_attention_map.png").stat().st_size > 0
    assert np.array_equal(rep2.unit_sums, report.unit_sums)
    maps, path = AR.visualize_attention_rollout(m, cfg, loader, n_images=8, output_dir=str(tmp_path))
    assert maps.shape == (8, 4, 4) and (tmp_path / "vit_som_attention_rollout.png").stat().st_size > 0
    assert path == str(tmp_path / "vit_som_attention_rollout.png")


def test_evaluate_attention_for_a_classifier_and_label_refusal(tiny):
    import vit_som_amd
    from vit_som_amd import attention_rollout as AR
    m, cfg, _, _ = tiny
    torch.manual_seed(5)
    vc = vit_som_amd.ViTClassifier(_vit_config(), device=DEV)
    _sharpen(vc.model)
    report = AR.evaluate_attention(vc, _vit_config(), _loader(), query="cls", head_fusion="max")
    assert report.unit_maps is None and report.unit_counts is None and report.class_counts.sum() == 15
    assert report.query == "cls" and 0.0 < report.entropy <= 1.0
    with pytest.raises(ValueError, match=r"evaluate_attention: 15 labels fell outside \[0, 5\)"):
        AR.evaluate_attention(m, cfg, [(x, y + 5) for x, y in _loader()])
    with pytest.raises(ValueError, match="evaluate_attention: the loader is empty"):
        AR.evaluate_attention(m, cfg, [])


def test_train_driver_reports_the_rollout(tmp_path, monkeypatch):
    from helpers import load_golden
    from vit_som_amd.train import _parser, main, synthetic_loaders
    assert _parser().parse_args(["--config", "c", "--attention-report"]).attention_report is True
    _, cfg = load_golden("ref_cluster_tiny")
    cfg = copy.deepcopy(cfg)
    cfg["hyperparameters"]["batch_size"] = 32
    monkeypatch.chdir(tmp_path)                                          # the figures go to experiments/plots under the cwd
    logs = []
    loaders = lambda c, r, w: synthetic_loaders(c, r, w, n_train=96, n_val=32, n_test=32)      # noqa: E731
    met = main(cfg, n_runs=1, max_epochs=1, make_loaders=loaders, model_states_dir=str(tmp_path / "states"), log=logs.append,
               attention_report=True)
    assert len(met["rollout_entropy"]) == 1 and 0.0 < met["rollout_entropy"][0] <= 1.0
    assert len(met["rollout_cls_mass"]) == 1 and 0.0 <= met["rollout_cls_mass"][0] < 1.0
    assert any(line.startswith("Attention rollout: rollout_entropy") for line in logs)
    for name in ("vit_som_attention_map.png", "vit_som_attention_rollout.png"):
        assert (tmp_path / "experiments" / "plots" / name).stat().st_size > 0
    off = main(cfg, n_runs=1, max_epochs=1, make_loaders=loaders, model_states_dir=str(tmp_path / "states"), log=logs.append)
    assert "rollout_entropy" not in off                                  # without the flag nothing changes
