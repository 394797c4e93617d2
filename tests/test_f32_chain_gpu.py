"""The exact-f32 contraction (csrc/gemm_f32.h: F32Stage, F32_KLOOP, mfma_tile) bit for bit against a host emulation of its
summation chain, through every entry whose output is that chain and nothing after it: the three Linear GEMMs under
GEMM_F32 (NT, NN, TN with the column-sum hook) and the two PCA contractions (the centring hook, NT and TN).

The chain of one output element: k-tile by k-tile, 8-group by 8-group, MFMA step s = 0..3, k = kb + s before kb + 4 + s,
every product joined by one fused multiply-add.  The inputs are +-m 2^e with m in [128, 255] and e in [-10, -4]: a product
has 16 bits, a sum of up to 72 of them spans at most 35, so the fp64 expression a * b + c is exact and its one rounding to
float32 is the fma's.  On such inputs the chain and the natural order 0 .. K - 1 differ in a tenth (K = 27) to a third
(K = 72) of the elements, so a kernel that summed in another order would not pass (checked below, on the host).

Shapes: 130 rows (two 128-row tiles, the second ragged), 70 columns (two 64-column tiles), K = 72 (three k-tiles, the last
holding 8) and K = 27 (below a tile and no multiple of 4: element-wise loads); where 70 or 130 make an operand's row pitch
no multiple of four floats, the aligned neighbour (72, 132) is run as well, and every case once more through views that
begin one float later: both the 16-byte buffer loads and the generic staging feed the chain."""
import numpy as np
import pytest
import torch

from vit_som_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
f32, f64 = np.float32, np.float64


def draw(shape, seed):
    rs = np.random.RandomState(seed)
    m = rs.randint(128, 256, size=shape).astype(f64)
    e = rs.randint(-10, -3, size=shape)
    sign = rs.randint(0, 2, size=shape) * 2.0 - 1.0
    return (sign * np.ldexp(m, e)).astype(f32)


def chain_order(K):
    return [k for kb in range(0, -(-K // 32) * 32, 8) for s in range(4) for k in (kb + s, kb + 4 + s) if k < K]


def contract(a, b, order):
    """c[m, n] = the fma chain over k in `order` of a[m, k] b[n, k]."""
    a, b = a.astype(f64), b.astype(f64)
    c = np.zeros((a.shape[0], b.shape[0]), f32)
    for k in order:
        c = (a[:, k, None] * b[None, :, k] + c.astype(f64)).astype(f32)
    return c


def chain(a, b):
    return contract(a, b, chain_order(a.shape[1]))


def place(a, off):
    """`a` on the device, contiguous, beginning `off` floats after a 16-byte boundary."""
    buf = torch.empty(a.size + off, dtype=torch.float32, device=DEV)
    t = buf[off:].view(*a.shape)
    t.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    return t


def host(t):
    return t.detach().cpu().numpy()


def same(got, want, what):
    got = host(got)
    bad = got != want                     # on the values: -0 equals +0
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} elements differ, first at {np.argwhere(bad)[0]}"


@pytest.fixture
def gemm_f32():
    mode = ops.get_gemm_mode()
    try:
        ops.set_gemm_mode(ops.GEMM_F32)
        yield
    finally:
        ops.set_gemm_mode(mode)


@pytest.mark.parametrize("K, least", [(27, 0.05), (72, 0.15)])
def test_the_chain_is_told_apart_from_the_natural_order(K, least):
    a, b = draw((130, K), 1), draw((70, K), 2)
    differ = (chain(a, b) != contract(a, b, range(K))).mean()
    print(f"K = {K}: {differ:.3f} of the elements differ between the two orders")
    assert differ > least


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("K", [72, 27])
def test_linear_fwd_is_the_chain(gemm_f32, K, off):
    x, W = draw((130, K), 10 + K), draw((70, K), 11 + K)
    out = torch.empty(130, 70, device=DEV)
    ops.linear_fwd(place(x, off), place(W, off), torch.zeros(70, device=DEV), out)
    same(out, chain(x, W), "linear_fwd")


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("cols", [70, 72])
@pytest.mark.parametrize("K", [72, 27])
def test_linear_bwd_input_is_the_chain(gemm_f32, K, cols, off):
    dy, W = draw((130, K), 20 + K), draw((K, cols), 21 + K)
    dx = torch.empty(130, cols, device=DEV)
    ops.linear_bwd_input(place(dy, off), place(W, off), dx)
    same(dx, chain(dy, W.T), "linear_bwd_input")


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("N, K", [(130, 70), (132, 72)])
@pytest.mark.parametrize("M", [27, 32])
def test_linear_bwd_weight_is_the_chain_and_its_bias_the_column_sum(gemm_f32, M, N, K, off):
    """One k-tile, one split: dW is the chain, db the column-sum hook -- dY's rows added in ascending order, in float32."""
    dy, x = draw((M, N), 30 + M), draw((M, K), 31 + M)
    dW, db = torch.empty(N, K, device=DEV), torch.empty(N, device=DEV)
    ops.linear_bwd_weight(place(dy, off), place(x, off), dW, db)
    same(dW, chain(dy.T, x.T), "linear_bwd_weight dW")
    s = np.zeros(N, f32)
    for m in range(M):
        s = s + dy[m]
    same(db, s, "linear_bwd_weight db")


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("D", [27, 32])
def test_pca_project_is_the_chain_of_the_centred_rows(D, off):
    X, mean, B = draw((130, D), 40 + D), draw((D,), 41 + D), draw((D, D), 42 + D)
    Y = torch.empty(130, D, device=DEV)
    ops.pca_project(place(X, off), place(mean, off), place(B, off), None, Y)
    same(Y, chain(X - mean, B), "pca_project")


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("l, D", [(130, 134), (132, 136)])
def test_pca_backproject_is_the_chain_of_the_centred_columns(l, D, off):
    Y, X, mean = draw((27, l), 50 + l), draw((27, D), 51 + l), draw((D,), 52 + l)
    Zt = torch.empty(l, D, device=DEV)
    ops.pca_backproject(place(Y, off), place(X, off), place(mean, off), Zt)
    same(Zt, chain(Y.T, (X - mean).T), "pca_backproject")
