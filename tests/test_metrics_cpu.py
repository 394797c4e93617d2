"""What helpers.tile_rel_err sees that helpers.rel_err does not: errors confined to one GEMM output tile, one token row's
contribution to a weight gradient, one bias element -- and what it ignores: fp32 rounding of an fp64 reference, and
rows whose reference is negligible (prototypes far from every BMU)."""
import torch

from helpers import rel_err, tile_rel_err

BAR = 1e-4          # the model-level gradient bar


def _rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def test_one_scaled_tile_of_the_prototype_gradient():
    ref = _rnd(1600, 12288, seed=1)                      # c3's prototype gradient: K x L
    for r0, c0 in ((640, 4096), (1536, 12224), (608, 4128)):       # aligned, the last tile, straddling four metric tiles
        got = ref.clone()
        got[r0:r0 + 64, c0:c0 + 64] *= 1 + 1e-3
        assert rel_err(got, ref) < BAR                   # diluted: ~1.4e-5
        assert tile_rel_err(got, ref) > 4e-4, (r0, c0)


def test_one_token_row_missing_from_a_weight_gradient():
    dy, x = _rnd(4160, 768, seed=2), _rnd(4160, 192, seed=3)
    ref = dy.T @ x                                       # 768 x 192, as mlp.0's dW = dY^T X
    got = ref - torch.outer(dy[1234], x[1234])
    assert tile_rel_err(got, ref) > 100 * BAR


def test_one_bias_element_zeroed():
    ref = _rnd(768, seed=4)
    got = ref.clone()
    got[700] = 0.0
    assert tile_rel_err(got, ref) > 100 * BAR
    # a 1-D tensor is one row cut into 64-element tiles; the same in a 4-D patch kernel, viewed as [E, C*p*p]
    w = _rnd(192, 3, 4, 4, seed=5)
    w2 = w.clone()
    w2[17, 2, 3, 1] += 1.0
    assert tile_rel_err(w2, w) > 1.5 * rel_err(w2, w) > 100 * BAR


def test_fp32_rounding_and_negligible_rows_are_ignored():
    ref = _rnd(1600, 3136, seed=6)
    # rows scaled like a neighbourhood exp(-d^2 / 2T^2): most of them fall far below fp32's range
    d2 = torch.arange(1600, dtype=torch.float64) / 8.0
    ref = ref * torch.exp(-d2)[:, None]
    assert float(ref[-1].abs().max()) < 1e-40
    assert tile_rel_err(ref.float(), ref) < 1e-6
    assert tile_rel_err(ref.float(), ref) < tile_rel_err(ref.float() * (1 + 1e-5), ref)
    for shape in ((768, 192), (768,), (1, 1, 192), (100, 12288)):
        r = _rnd(*shape, seed=7)
        assert tile_rel_err(r.float(), r) < 1e-6
        assert tile_rel_err(r, r) == 0.0
