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
