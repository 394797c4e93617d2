"""Host arithmetic and argument checks of the input-gradient GEMM + LayerNorm backward entries (no launch happens)."""


def test_support_predicate_and_partial_size():
    from vit_som_amd._lib import lib
    assert lib.vsom_get_gemm_mode() == 2                                   # default: split-bf16, three gradient products
    assert lib.vsom_linear_bwd_input_ln_supported(33280, 768, 192) == 1
    assert lib.vsom_linear_bwd_input_ln_supported(33280, 384, 96) == 1
    assert lib.vsom_linear_bwd_input_ln_supported(33280, 768, 128) == 0    # widths other than 192 / 96
    assert lib.vsom_linear_bwd_input_ln_supported(300, 768, 192) == 0      # 5 row tiles: too few for the column reducer
    assert lib.vsom_linear_bwd_input_ln_supported(31 * 64, 768, 192) == 0 and lib.vsom_linear_bwd_input_ln_supported(32 * 64, 768, 192) == 1
    assert lib.vsom_linear_bwd_input_ln_supported(31 * 128, 384, 96) == 0 and lib.vsom_linear_bwd_input_ln_supported(32 * 128, 384, 96) == 1
    assert lib.vsom_set_gemm_mode(0) == 0
    try:
        assert lib.vsom_linear_bwd_input_ln_supported(33280, 768, 192) == 0  # VSOM_GEMM_F32
    finally:
        lib.vsom_set_gemm_mode(2)
    # one [2][cols] partial per row tile: 64-row tiles at 192 columns, 128-row tiles at 96
    assert lib.vsom_linear_bwd_input_ln_partial_bytes(33280, 192) == 520 * 2 * 192 * 4
    assert lib.vsom_linear_bwd_input_ln_partial_bytes(33280 + 17, 96) == 261 * 2 * 96 * 4
    assert lib.vsom_linear_bwd_input_ln_partial_bytes(33280, 128) == 0
    assert lib.vsom_linear_bwd_input_ln_partial_bytes(0, 192) == 0


def test_argument_checks():
    from vit_som_amd._lib import last_error, lib
    part = lib.vsom_linear_bwd_input_ln_partial_bytes(33280, 192)
    a = (16, 768, 16, 33280, 768, 192, 16, 16, 16, 16, None, 16)          # dY, lddy, Wt, M, N, K, X, mean, rstd, gamma, resid, dX
    assert lib.vsom_linear_bwd_input_ln_partial(None, *a[1:], 16, part, None) == -1
    assert "null" in last_error()
    assert lib.vsom_linear_bwd_input_ln(*a, None, 16, 16, part, None) == -1                  # no dgamma
    assert lib.vsom_linear_bwd_input_ln_partial(16, 700, *a[2:], 16, part, None) == -1       # lddy < N
    assert lib.vsom_linear_bwd_input_ln_partial(*a[:5], 128, *a[6:], 16, part, None) == -3   # width 128
    assert "unsupported" in last_error()
    assert lib.vsom_linear_bwd_input_ln_partial(*a[:11], 20, 16, part, None) == -2           # dX misaligned
    assert lib.vsom_linear_bwd_input_ln_partial(*a, 16, part - 4, None) == -4                # partial buffer too small
    assert lib.vsom_linear_bwd_input_ln_partial(*a, None, part, None) == -4
    assert lib.vsom_linear_bwd_input_ln(*a, 16, 16, 16, part - 4, None) == -4


def test_hook_is_part_of_the_tape_signature():
    from vit_som_amd.tuning import hooks
    assert hooks.ln_bwd_fused is True
    assert ("ln_bwd_fused", True) in hooks.signature()
    try:
        hooks.set(ln_bwd_fused=False)
        assert ("ln_bwd_fused", False) in hooks.signature()
    finally:
        hooks.reset()
