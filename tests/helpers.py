"""Shared test helpers (golden loading, tolerances)."""
import json
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REF_CASES = ["ref_cluster_tiny", "ref_cls_tiny", "ref_mnistlike_tiny", "ref_hexa_euclid_tiny", "ref_manhattan_tiny"]


def load_golden(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
    cfg = json.loads(str(z["config_json"]))
    return z, cfg


def golden_params(z, prefix="param/"):
    return {k[len(prefix):]: torch.from_numpy(z[k]) for k in z.files if k.startswith(prefix)}


def f32_close(a, ref, atol):
    """True when |a - ref| <= max(atol, 4 fp32 ulps of ref) everywhere.  The golden arrays carry one host's fp32 summation
    order; another host's vector width and BLAS kernels move a value by an ulp or two, and at |ref| ~ 240 (Manhattan
    distances) one ulp is already more than 1e-5.  Below |ref| ~ 20 the bound is atol itself."""
    ref = np.asarray(ref, dtype=np.float32)
    tol = np.maximum(atol, 4 * np.spacing(np.abs(ref)).astype(np.float64))
    return bool((np.abs(np.asarray(a, dtype=np.float64) - ref) <= tol).all())


def rel_err(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).norm() / (b.norm() + 1e-30))


def tile_rel_err(got, ref, tile=(64, 64)):
    """Worst relative error over the output tiles of a gradient: max_t |g_t - r_t| / max(|r_t|, 0.1 RMS(r) sqrt(n_t)).

    rel_err is one Frobenius ratio over the whole tensor, so an error confined to one GEMM tile (a wrong edge tile, split
    or epilogue) is diluted by the size of the rest: one 64 x 64 tile of the 1600 x 12288 prototype gradient off by 1e-3
    moves it by 1.4e-5.  Here each tensor is viewed as 2-D [out, in] (a patch kernel [E, C, p, p] as [E, C*p*p]; 1-D
    and 0-D tensors as one row), cut into `tile` blocks (edge blocks are smaller), and each block is measured against
    its own norm.  The floor keeps blocks whose reference is negligible next to the tensor's typical entry -- prototype
    rows far from every BMU, whose gradient is ~1e-40 -- from dividing by nothing."""
    r = torch.as_tensor(ref).double()
    g = torch.as_tensor(got).to(r.device).double()
    assert g.shape == r.shape, (tuple(g.shape), tuple(r.shape))
    g = g.reshape(1, -1) if g.dim() < 2 else g.reshape(g.shape[0], -1)
    r = r.reshape(1, -1) if r.dim() < 2 else r.reshape(r.shape[0], -1)
    rows, cols = r.shape
    tr, tc = min(tile[0], rows), min(tile[1], cols)
    pad = (0, -cols % tc, 0, -rows % tr)
    shape = ((rows + pad[3]) // tr, tr, (cols + pad[1]) // tc, tc)

    def tile_sums(t):
        return torch.nn.functional.pad(t, pad).view(shape).sum((1, 3))

    err = tile_sums((g - r).pow(2)).sqrt()
    norm = tile_sums(r.pow(2)).sqrt()
    count = tile_sums(torch.ones_like(r))
    rms = float(r.pow(2).mean().sqrt())
    floor = (0.1 * rms * count.sqrt()).clamp_min(1e-30)
    return float((err / torch.maximum(norm, floor)).max())
