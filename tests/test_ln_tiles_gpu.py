"""The 192 x 192 tiles of the LayerNorm-fused input-gradient GEMM (vsom_set_ln_tiles(1)) against the 64 x 192 tiles they
replace: the per-element k order and MFMA order do not depend on the tile height, and every 64-row group runs the same
epilogue into the same partial slot, so dX, the dgamma / dbeta partials and the finished dgamma / dbeta are bitwise equal.
Row groups wholly past M write nothing: the buffers carry a sentinel tail that must survive."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENTINEL = 12345.0


@pytest.fixture(scope="module")
def ops():
    from vit_som_amd import ops as _ops
    prev = _ops.get_gemm_mode()
    yield _ops
    _ops.set_ln_tiles(1)
    _ops.set_gemm_mode(prev)


def _case(T, n, cols, resid, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g).to(DEV)
    dy, Wt, x = r(T, n), r(cols, n) * 0.05, r(T, cols) * 2 + 0.5
    gamma = 1 + 0.1 * r(cols)
    mean = x.mean(1).contiguous()
    rstd = torch.rsqrt(x.var(1, unbiased=False) + 1e-6).contiguous()
    res = r(T, cols) if resid else None
    return dy, Wt, x, mean, rstd, gamma, res


def _run(ops, mode, dy, Wt, x, mean, rstd, gamma, res):
    """dX and the partials from linear_bwd_input_ln_partial, dgamma / dbeta from linear_bwd_input_ln; every output buffer
    starts as NaN (an element left unwritten fails the comparison) with a sentinel tail past its end."""
    from vit_som_amd._lib import lib
    ops.set_ln_tiles(mode)
    T, cols = x.shape
    pn = lib.vsom_linear_bwd_input_ln_partial_bytes(T, cols) // 4
    part_buf = torch.full((pn + 4 * cols,), float("nan"), device=DEV)
    part_buf[pn:] = SENTINEL
    dx_buf = torch.full((T * cols + 4 * cols,), float("nan"), device=DEV)
    dx_buf[T * cols:] = SENTINEL
    dx = dx_buf[:T * cols].view(T, cols)
    ops.linear_bwd_input_ln_partial(dy, Wt, x, mean, rstd, gamma, res, dx, part_buf[:pn].view(torch.uint8))
    dx2, dg, db = torch.empty_like(x), torch.empty(cols, device=DEV), torch.empty(cols, device=DEV)
    ops.linear_bwd_input_ln(dy, Wt, x, mean, rstd, gamma, res, dx2, dg, db)
    torch.cuda.synchronize()
    assert bool((part_buf[pn:] == SENTINEL).all()) and bool((dx_buf[T * cols:] == SENTINEL).all()), "write past the end"
    assert torch.equal(dx, dx2)
    return dx.clone(), part_buf[:pn].clone(), dg, db


# 33280: 174 workgroups, the last with one live row group; 33297: the last with two (one ragged); 2048: 11, the last with
# two; 2112: every row group live; 4165: the last with one ragged row group
@pytest.mark.parametrize("mode", [2, 1])                      # GEMM_SPLIT_BF16_GRAD3 (the wide tiles), GEMM_SPLIT_BF16
@pytest.mark.parametrize("T", [33280, 33280 + 17, 2048, 2112, 4165])
@pytest.mark.parametrize("n", [768, 576])
@pytest.mark.parametrize("resid", [True, False])
def test_wide_tiles_bitwise(ops, mode, T, n, resid):
    ops.set_gemm_mode(mode)
    assert ops.linear_bwd_input_ln_supported(T, n, 192)
    case = _case(T, n, 192, resid, seed=T + n + int(resid))
    dx0, p0, dg0, db0 = _run(ops, 0, *case)
    dx1, p1, dg1, db1 = _run(ops, 1, *case)
    assert torch.equal(dx0, dx1)
    assert torch.equal(p0, p1)
    assert torch.equal(dg0, dg1) and torch.equal(db0, db1)
    assert bool(torch.isfinite(dx1).all()) and bool(torch.isfinite(p1).all())


def test_training_steps_bitwise_with_wide_tiles(ops):
    """Eight c3 training steps (batch 512: 33 280 tokens) end in bit-identical parameters and gradients with the 64 x 192
    and the 192 x 192 tiles (the launch tape is recorded again when the switch changes)."""
    import bench
    import vit_som_amd
    ops.set_gemm_mode(ops.GEMM_SPLIT_BF16_GRAD3)
    cfg = bench.c3_config(512)
    finals = []
    for mode in (0, 1):
        ops.set_ln_tiles(mode)
        torch.manual_seed(0)
        m = vit_som_amd.ViTSOM(copy.deepcopy(cfg), device=DEV)
        m.set_schedule(50000, 10000)
        m._it = 1000
        (opt,), _ = m.configure_optimizers()
        g = torch.Generator().manual_seed(5)
        for _ in range(8):
            xb = torch.randn(512, 3, 32, 32, generator=g).to(DEV)
            yb = torch.zeros(512, dtype=torch.int64, device=DEV)
            m.train_step_fused(xb, yb)
            opt.step()
        torch.cuda.synchronize()
        finals.append((m.arena.params.clone(), m.arena.grads.clone()))
        del m, opt
    ops.set_ln_tiles(1)
    assert torch.equal(finals[0][0], finals[1][0])
    assert torch.equal(finals[0][1], finals[1][1])
