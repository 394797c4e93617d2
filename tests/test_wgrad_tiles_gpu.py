"""The 192 x 192 weight-gradient tiles (vsom_set_wgrad_tiles) against the 192 x 64 tiles they replace: every output
element sums the same k-tiles in the same MFMA order, so at the same split count the slabs, dW and db are bitwise
equal; with their own split count they stay within the gradient mode's accuracy and are deterministic."""
import copy

import pytest
import torch

from helpers import rel_err

pytestmark = pytest.mark.gpu

DEV = "cuda"
T = 512 * 65
# (name, rows of dW, columns of dW): the encoder's qkv, proj, fc1, fc2 weight gradients
SHAPES = [("qkv", 576, 192), ("proj", 192, 192), ("fc1", 768, 192), ("fc2", 192, 768)]


@pytest.fixture(scope="module")
def ops():
    from vit_som_amd import ops as _ops
    prev = _ops.get_gemm_mode()
    _ops.set_gemm_mode(_ops.GEMM_SPLIT_BF16_GRAD3)
    yield _ops
    _ops.set_wgrad_tiles(2)
    _ops.set_gemm_mode(prev)


def rnd(*shape, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * 0.05).to(DEV)


def bwd_weight(ops, mode, dy, x, bias):
    ops.set_wgrad_tiles(mode)
    dW = torch.empty(dy.shape[1], x.shape[1], device=DEV)
    db = torch.empty(dy.shape[1], device=DEV) if bias else None
    ops.linear_bwd_weight(dy, x, dW, db)
    return dW, db


@pytest.mark.parametrize("name,N,K", SHAPES)
@pytest.mark.parametrize("M", [T, 1000, 1301, 4160])
@pytest.mark.parametrize("bias", [True, False])
def test_wide_tiles_bitwise_at_narrow_split_count(ops, name, N, K, M, bias):
    dy, x = rnd(M, N, seed=1), rnd(M, K, seed=2)
    dW0, db0 = bwd_weight(ops, 0, dy, x, bias)
    dW1, db1 = bwd_weight(ops, 1, dy, x, bias)
    assert torch.equal(dW0, dW1)
    assert not bias or torch.equal(db0, db1)


def test_wide_tiles_bitwise_with_row_map(ops):
    """The patch embedding's weight gradient skips each image's CLS row (row map a_seg = 64 patches, stride 65):
    C * p * p = 192 and E = 192 put it on the wide tiles (its entry always forms the bias gradient)."""
    B, C, S, p, E = 8, 3, 64, 8, 192
    n = (S // p) ** 2
    dt, xp = rnd(B, n + 1, E, seed=5), rnd(B * n, C * p * p, seed=6)
    outs = []
    for mode in (0, 1):
        ops.set_wgrad_tiles(mode)
        dW, dc = torch.empty(E, C * p * p, device=DEV), torch.empty(E, device=DEV)
        db = torch.empty(E, device=DEV)
        ops.patch_embed_bwd(dt, xp, dW, db, dc, B, C, S, p, E)
        outs.append((dW, db))
    assert torch.equal(outs[0][0], outs[1][0])
    assert torch.equal(outs[0][1], outs[1][1])
    ref = (dt[:, 1:].reshape(B * n, E).double().T @ xp.double())
    assert rel_err(outs[1][0].cpu(), ref.cpu()) < 2e-5


@pytest.mark.parametrize("name,N,K", SHAPES)
def test_wide_tiles_tuned_plan_accuracy_and_determinism(ops, name, N, K):
    dy, x = rnd(T, N, seed=3), rnd(T, K, seed=4)
    dW, db = bwd_weight(ops, 2, dy, x, True)
    ref = dy.double().T @ x.double()
    assert rel_err(dW.cpu(), ref.cpu()) < 2e-5, rel_err(dW.cpu(), ref.cpu())
    assert rel_err(db.cpu(), dy.double().sum(0).cpu()) < 1e-6
    dW2, db2 = bwd_weight(ops, 2, dy, x, True)
    assert torch.equal(dW, dW2) and torch.equal(db, db2)


def test_training_steps_bitwise_with_wide_tiles_at_narrow_split_count(ops):
    """Eight training steps at the encoder's widths end in bit-identical parameters with the 192 x 64 tiles and with the
    192 x 192 tiles at the same split counts (the launch tape is recorded again when the switch changes)."""
    import vit_som_amd
    from oracle.gen_golden import make_config
    cfg = make_config(3, 32, 4, 192, 4, 3, 96, 2, (12, 12), 0, 96)
    finals = []
    for mode in (0, 1, 0):
        ops.set_wgrad_tiles(mode)
        torch.manual_seed(0)
        m = vit_som_amd.ViTSOM(copy.deepcopy(cfg), device=DEV)
        m.set_schedule(5000, 500)
        m._it = 100
        (opt,), _ = m.configure_optimizers()
        g = torch.Generator().manual_seed(5)
        for _ in range(8):
            xb = torch.randn(96, 3, 32, 32, generator=g).to(DEV)
            yb = torch.zeros(96, dtype=torch.int64, device=DEV)
            m.train_step_fused(xb, yb)
            opt.step()
        finals.append(m.arena.params.clone())
    ops.set_wgrad_tiles(2)
    assert torch.equal(finals[0], finals[1]) and torch.equal(finals[0], finals[2])
