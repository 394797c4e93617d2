"""The input-gradient GEMM with the LayerNorm backward in its epilogue (ops.linear_bwd_input_ln) against the two-launch
path it replaces (linear_bwd_input_t into scratch + layernorm_bwd): dX bit for bit, dgamma / dbeta to rounding."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    from vit_som_amd import ops as _ops
    return _ops


def _case(T, n, cols, resid, seed=0):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g).to(DEV)
    dy, Wt, x = r(T, n), r(cols, n) * 0.05, r(T, cols) * 2 + 0.5
    gamma = 1 + 0.1 * r(cols)
    mean = x.mean(1)
    rstd = torch.rsqrt(x.var(1, unbiased=False) + 1e-6)
    res = r(T, cols) if resid else None
    return dy, Wt, x, mean.contiguous(), rstd.contiguous(), gamma, res


def _two_launch(ops, dy, Wt, x, mean, rstd, gamma, res):
    T, cols = x.shape
    da = torch.empty(T, cols, device=DEV)
    ops.linear_bwd_input_t(dy, Wt, da)
    dx, dg, db = torch.empty_like(x), torch.empty(cols, device=DEV), torch.empty(cols, device=DEV)
    ops.layernorm_bwd(da, x, mean, rstd, gamma, res, dx, dg, db)
    return dx, dg, db, da


def _fused(ops, dy, Wt, x, mean, rstd, gamma, res):
    cols = x.shape[1]
    dx, dg, db = torch.empty_like(x), torch.empty(cols, device=DEV), torch.empty(cols, device=DEV)
    ops.linear_bwd_input_ln(dy, Wt, x, mean, rstd, gamma, res, dx, dg, db)
    return dx, dg, db


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


@pytest.mark.parametrize("mode", [1, 2])                      # GEMM_SPLIT_BF16 (six products), GEMM_SPLIT_BF16_GRAD3 (three)
@pytest.mark.parametrize("T", [33280, 6240, 33280 + 17, 4100 + 3])
@pytest.mark.parametrize("n,cols", [(768, 192), (192, 192), (576, 192), (384, 96), (288, 96)])
@pytest.mark.parametrize("resid", [True, False])
def test_fused_matches_two_launch(ops, mode, T, n, cols, resid):
    prev = ops.get_gemm_mode()
    ops.set_gemm_mode(mode)
    try:
        assert ops.linear_bwd_input_ln_supported(T, n, cols)
        case = _case(T, n, cols, resid, seed=T + n + cols)
        dx0, dg0, db0, da = _two_launch(ops, *case)
        dx1, dg1, db1 = _fused(ops, *case)
        torch.cuda.synchronize()
    finally:
        ops.set_gemm_mode(prev)
    assert torch.equal(dx0, dx1)
    assert _rel(dg1, dg0) < 1e-6 and _rel(db1, db0) < 1e-6
    # against fp64 from the same GEMM product
    dy, Wt, x, mean, rstd, gamma, res = case
    xh = (x.double() - mean.double()[:, None]) * rstd.double()[:, None]
    assert _rel(dg1, (da.double() * xh).sum(0)) < 2e-5
    assert _rel(db1, da.double().sum(0)) < 2e-5


@pytest.mark.parametrize("cols,n", [(192, 768), (96, 384)])
def test_partial_and_finish_many_give_the_one_call_bits(ops, cols, n):
    T = 33280 + 17
    case = _case(T, n, cols, True, seed=5)
    dx0, dg0, db0 = _fused(ops, *case)
    jobs = ops.LayerNormJobs(torch.device(DEV))
    jobs.begin()
    dx1, dg1, db1 = torch.empty_like(dx0), torch.empty_like(dg0), torch.empty_like(db0)
    dy, Wt, x, mean, rstd, gamma, res = case
    jobs.bwd_linear_fused(dy, Wt, x, mean, rstd, gamma, res, dx1, dg1, db1)
    jobs.flush()
    torch.cuda.synchronize()
    assert torch.equal(dx0, dx1) and torch.equal(dg0, dg1) and torch.equal(db0, db1)


def test_unsupported_shapes_are_refused(ops):
    assert not ops.linear_bwd_input_ln_supported(33280, 768, 128)
    assert not ops.linear_bwd_input_ln_supported(300, 768, 192)           # too few row tiles: the two-launch path
    assert not ops.linear_bwd_input_ln_supported(300, 384, 96)
    prev = ops.get_gemm_mode()
    ops.set_gemm_mode(0)
    try:
        assert not ops.linear_bwd_input_ln_supported(33280, 768, 192)
    finally:
        ops.set_gemm_mode(prev)


def test_c3_steps_with_and_without_the_fused_layernorm_backward():
    """8 training steps at the c3 architecture (smaller batch): parameters within the default mode's gradient tolerance."""
    import vit_som_amd
    from oracle.gen_golden import make_config
    from vit_som_amd.tuning import hooks
    cfg = make_config(3, 32, 4, 192, 12, 3, 96, 2, (12, 12), 0, 64)
    finals = []
    try:
        for fused in (False, True):
            hooks.set(ln_bwd_fused=fused)
            torch.manual_seed(0)
            m = vit_som_amd.ViTSOM(cfg, device=DEV)
            m.set_schedule(50000, 10000)
            (opt,), _ = m.configure_optimizers()
            g = torch.Generator().manual_seed(1)
            x = torch.rand(64, 3, 32, 32, generator=g).to(DEV)
            y = torch.randint(0, 10, (64,), generator=g).to(DEV)
            for _ in range(8):
                m.train_step_fused(x, y)
                opt.step()
            torch.cuda.synchronize()
            finals.append(torch.cat([p.detach().flatten() for p in m.parameters()]))
    finally:
        hooks.reset()
    assert _rel(finals[1], finals[0]) < 1e-5
