"""Host arithmetic of the weight-gradient launch plan (gemm_f32.hip, bwd_weight_plan): the workspace query must cover
the slabs the plan writes, in every setting of vsom_set_wgrad_tiles, for every weight-gradient shape the ViT-SOM step
and the classifier step launch.  Pure host code: no GPU needed (the CU count falls back to the MI355X's 256)."""
import pytest

CUS = 256


def cdiv(a, b):
    return -(-a // b)


def splits_for(tiles, ktiles, target):
    s = min(max((target + tiles // 2) // tiles, 1), ktiles)
    return cdiv(ktiles, cdiv(ktiles, s))


def planned_splits(mode, M, N, K):
    """Slabs written by the tile kernels; None where the generic kernel runs (its own split choice)."""
    ktiles = cdiv(M, 32)
    if N % 192 == 0 and K % 64 == 0:
        tiles = (N // 192) * (K // 64)
    elif N % 96 == 0 and K % 96 == 0:
        tiles = (N // 96) * (K // 96)
    else:
        return None
    if mode == 2 and N % 192 == 0 and K % 192 == 0:
        return splits_for((N // 192) * (K // 192), ktiles, 3 * CUS // 4)
    return splits_for(tiles, ktiles, 384)


def pad4(n):
    return (n + 3) & ~3


def step_shapes(B):
    """(M, N, K) of every linear_bwd_weight of the c3 ViT-SOM step and of the classifier step at batch B."""
    T, E, H4, D, n = B * 65, 192, 768, 96, 64
    enc = [(T, 3 * E, E), (T, E, E), (T, H4, E), (T, E, H4)]
    dec = [(T, 3 * D, D), (T, D, D), (T, 4 * D, D), (T, D, 4 * D), (T, D, E), (B * n, 48, D)]
    patch = [(B * n, E, 48)]
    cls = [(B, E, E), (T, 2 * E, E), (B, 10, E), (B, H4, E), (B, E, H4)]
    return enc + dec + patch + cls


@pytest.fixture(scope="module")
def lib():
    from vit_som_amd._lib import lib as _lib
    return _lib


@pytest.mark.parametrize("B", [512, 96, 7])
def test_workspace_covers_the_plan(lib, B):
    from vit_som_amd import ops
    try:
        for mode in (0, 1, 2):
            ops.set_wgrad_tiles(mode)
            for M, N, K in step_shapes(B):
                got = lib.vsom_linear_bwd_weight_workspace_bytes(M, N, K)
                stride = (pad4(N * K) + pad4(N)) * 4
                s = planned_splits(mode, M, N, K)
                if s is None:
                    assert got >= stride, (mode, M, N, K)
                else:
                    assert got == s * stride, (mode, M, N, K, got, s)
    finally:
        ops.set_wgrad_tiles(2)


def test_wide_plan_split_counts(lib):
    """c3 encoder shapes: the 192 x 192 plan puts about 192 workgroups on the chip (three quarters of the CUs), the
    192 x 64 plan about 384; mode 1 keeps the latter's split counts."""
    from vit_som_amd import ops
    T = 512 * 65
    try:
        for (N, K), wgs in (((576, 192), 186), ((192, 192), 174), ((768, 192), 192), ((192, 768), 192)):
            assert planned_splits(2, T, N, K) * (N // 192) * (K // 192) == wgs
            assert planned_splits(1, T, N, K) == planned_splits(0, T, N, K)
        ops.set_wgrad_tiles(1)
        a = lib.vsom_linear_bwd_weight_workspace_bytes(T, 576, 192)
        ops.set_wgrad_tiles(0)
        assert lib.vsom_linear_bwd_weight_workspace_bytes(T, 576, 192) == a
    finally:
        ops.set_wgrad_tiles(2)


def test_described_split_counts_are_the_planned_ones(lib):
    """The same plan read directly (vsom_describe_plan): split count and workgroups of the tile kernels."""
    import ctypes
    import re
    from vit_som_amd import ops
    buf = ctypes.create_string_buffer(160)
    try:
        for mode in (0, 1, 2):
            ops.set_wgrad_tiles(mode)
            for M, N, K in step_shapes(512):
                s = planned_splits(mode, M, N, K)
                if s is None:
                    continue
                assert lib.vsom_describe_plan(8, M, N, K, 1, buf, len(buf)) == 0
                m = re.match(r"engine=x6_tn tile=(\d+)x(\d+) .* splits=(\d+) workgroups=(\d+)$", buf.value.decode())
                assert m, buf.value
                rows, cols, splits, wgs = map(int, m.groups())
                assert splits == s and wgs == (N // rows) * (K // cols) * s, (mode, M, N, K, buf.value)
                assert (rows, cols) == ((192, 192) if mode and N % 192 == 0 and K % 192 == 0 else
                                        (192, 64) if N % 192 == 0 and K % 64 == 0 else (96, 96))
    finally:
        ops.set_wgrad_tiles(2)


def test_set_wgrad_tiles_rejects_unknown_modes(lib):
    assert lib.vsom_set_wgrad_tiles(3) != 0
    assert lib.vsom_set_wgrad_tiles(-1) != 0
    assert lib.vsom_set_wgrad_tiles(2) == 0
