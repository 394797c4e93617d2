"""Restatement of attention rollout for the tests: a torch chain over fully materialised matrices, in the dtype the caller
names (fp64: the reference; fp32: the yardstick of the accuracy rule).  Written from the formulas, not from the kernel:

    P_h[i, j] = softmax_j(q_i . k_j / sqrt(hd))                          (numeric_edges.attention_eval's softmax)
    F         = mean / max / min over the heads of P_h, element by element
    A[i, j]   = (alpha F[i, j] + (1 - alpha) [i == j]) / (alpha sum_j F[i, j] + (1 - alpha))
    step      : v_out[b, j] = sum_i v_in[b, i] A_b[i, j]
    rollout   : v = w, then the step of block L - 1, L - 2, ... down to start_layer

Pure torch; runs on the CPU and, for speed in the GPU tests, on the device alike."""
import torch

FUSIONS = ("mean", "max", "min")
FLOOR = 3e-6                                     # the bound vsom_attention_probs is held to; the row-scaled map peaks at 1
FACTOR = 4.0                                     # numeric_edges.FACTOR


def probabilities(qkv, B, N, H, hd, dtype):
    """[B, H, N, N] softmax probabilities of a block from its qkv buffer [B N, 3 H hd] (columns [3][H][hd])."""
    x = qkv.to(dtype).reshape(B, N, 3, H, hd)
    q, k = x[:, :, 0].permute(0, 2, 1, 3), x[:, :, 1].permute(0, 2, 1, 3)
    s = (q @ k.transpose(-2, -1)) * hd ** -0.5
    return s.softmax(-1)


def fuse(P, fusion):
    """[B, N, N] from [B, H, N, N]."""
    if fusion == "mean":
        return P.mean(dim=1)
    if fusion == "max":
        return P.max(dim=1).values
    if fusion == "min":
        return P.min(dim=1).values
    raise ValueError(fusion)


def mixed(P, fusion, alpha):
    """The residual-mixed, row-normalised matrix A [B, N, N] of one block from its probabilities P [B, H, N, N]."""
    F = fuse(P, fusion)
    eye = torch.eye(F.shape[-1], dtype=F.dtype, device=F.device)
    return (alpha * F + (1 - alpha) * eye) / (alpha * F.sum(-1, keepdim=True) + (1 - alpha))


def step_from_probs(P, v, fusion, alpha):
    return torch.einsum("bi,bij->bj", v.to(P.dtype), mixed(P, fusion, alpha))


def step(qkv, v, B, N, H, hd, fusion, alpha, dtype):
    return step_from_probs(probabilities(qkv, B, N, H, hd, dtype), v, fusion, alpha)


def rollout(qkvs, w, B, N, H, hd, fusion, alpha, dtype):
    """qkvs in forward order: the last block's step comes first."""
    v = w.to(dtype)
    for qkv in reversed(list(qkvs)):
        v = step(qkv, v, B, N, H, hd, fusion, alpha, dtype)
    return v


def rollout_from_maps(attns, w, fusion, alpha, start_layer, dtype):
    """The same chain over attention maps [B, H, N, N] per block, as ViTAutoencoder.forward(x, return_attns=True) returns."""
    v = w.to(dtype)
    for P in reversed(list(attns)[start_layer:]):
        v = step_from_probs(P.to(dtype), v, fusion, alpha)
    return v


def query(kind, B, N, seed=0):
    """The three v_in of the one-step tests: e_cls, uniform over the patches, random positive."""
    w = torch.zeros(B, N)
    if kind == "cls":
        w[:, 0] = 1.0
    elif kind == "patches":
        if N > 1:
            w[:, 1:] = 1.0 / (N - 1)
        else:
            w[:, 0] = 1.0
    else:
        w = torch.rand(B, N, generator=torch.Generator().manual_seed(seed)) + 0.05
    return w


def row_scaled_error(got, ref):
    """e = max_b ( max_j |got - ref| / max_j ref ): every sample's map measured against its own largest value."""
    got, ref = got.double().cpu(), ref.double().cpu()
    return float(((got - ref).abs().max(dim=1).values / ref.max(dim=1).values).max())


def bound(e32):
    return max(FLOOR, FACTOR * e32)
