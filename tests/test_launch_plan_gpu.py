"""Every row of the launch-plan table (launch_plan_rows.PLAN_ROWS) run through its ops wrapper, in every GEMM mode and
every setting of the family's hook, against an fp64 torch reference.  Bounds are the suite's own (test_ops_gpu.py):
GEMM_TOL, GRAD3_TOL where the row runs three products, and the per-entry bounds of test_linear_gelu_fwd, test_bmu_cosine,
test_bmu_cosine_x3_rerank and test_attention.  The rows of the cosine BMU pass run the package's dispatcher
(SOMLayer._distances_into) and hold it, bit for bit, to the wrapper of the form the plan names.  The references are
computed once per row and shared by the modes."""
import functools

import pytest
import torch
import torch.nn.functional as F

import launch_plan_rows as R
from helpers import rel_err
from test_launch_plan_cpu import describe
from test_ops_gpu import GEMM_TOL, GRAD3_TOL

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    from vit_som_amd import ops as _ops
    return _ops


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def padded(rows, cols, pad, seed):
    """[rows, cols] view of a [rows, cols + pad] tensor: (host view, device view)."""
    full = rnd(rows, cols + pad, seed=seed)
    return full[:, :cols], full.to(DEV)[:, :cols]


@functools.lru_cache(maxsize=None)
def case(i):
    """Inputs (host, fp32) and fp64 references of PLAN_ROWS[i]."""
    row = R.PLAN_ROWS[i]
    M, N, K = row.shape
    c = {}
    if row.op in (R.LINEAR_FWD, R.LINEAR_GELU_FWD, R.LINEAR_RELU_FWD, R.LINEAR_RESIDUAL_FWD):
        c["x"], c["xd"] = padded(M, K, row.ld_pad, 1)
        c["W"], c["b"], c["R"] = rnd(N, K, seed=2, scale=0.1), rnd(N, seed=3), rnd(M, N, seed=4)
        c["pre"] = c["x"].double() @ c["W"].double().T + c["b"].double()
        if row.op == R.LINEAR_GELU_FWD:
            pre = c["pre"].clone().requires_grad_(True)
            c["act"] = F.gelu(pre)
            c["act"].sum().backward()
            c["act"], c["grad"] = c["act"].detach(), pre.grad
    elif row.op in (R.BWD_INPUT, R.BWD_INPUT_GELU, R.BWD_INPUT_T, R.BWD_INPUT_T_GELU):
        c["dy"], c["W"], c["gg"] = rnd(M, N, seed=1), rnd(N, K, seed=2, scale=0.1), rnd(M, K, seed=6)
        c["ref"] = c["dy"].double() @ c["W"].double()
        if row.op in (R.BWD_INPUT_GELU, R.BWD_INPUT_T_GELU):
            c["ref"] = c["ref"] * c["gg"].double()
    elif row.op == R.BWD_WEIGHT:
        c["dy"], c["dyd"] = padded(M, N, row.ld_pad, 1)
        c["x"] = rnd(M, K, seed=2)
        c["dW"], c["db"] = c["dy"].double().T @ c["x"].double(), c["dy"].double().sum(0)
    elif row.op == R.BWD_INPUT_LN:
        c["dy"], c["Wt"], c["x"] = rnd(M, N, seed=1), rnd(K, N, seed=2, scale=0.05), rnd(M, K, seed=3) * 2 + 0.5
        c["gamma"] = 1 + 0.1 * rnd(K, seed=4)
        c["mean"], c["rstd"] = c["x"].mean(1), torch.rsqrt(c["x"].var(1, unbiased=False) + 1e-6)
        x = c["x"].double().requires_grad_(True)
        y = (x - x.mean(1, keepdim=True)) * torch.rsqrt(x.var(1, unbiased=False, keepdim=True) + 1e-6) * c["gamma"].double()
        da = c["dy"].double() @ c["Wt"].double().T
        y.backward(da)
        c["dx"], c["dbeta"] = x.grad, da.sum(0)
    elif row.op in (R.SOM_BWD_GW, R.SOM_BWD_GX, R.BMU_COSINE_DOTS, R.BMU_COSINE):
        B, Kp, L = row.shape
        c["x"], c["xd"] = padded(B, L, row.ld_pad, 1)
        c["W"] = F.normalize(torch.rand(Kp, L, generator=torch.Generator().manual_seed(2)), dim=1)
        c["coef"], c["rd"], c["cd"], c["gx0"] = rnd(B, Kp, seed=3), rnd(B, seed=4), rnd(Kp, seed=5), rnd(B, L, seed=6)
        x, W, coef = c["x"].double(), c["W"].double(), c["coef"].double()
        c["gW"] = coef.T @ x + c["cd"].double()[:, None] * W
        c["gX"] = c["gx0"].double() + coef @ W + c["rd"].double()[:, None] * x
        c["d64"] = 1 - F.normalize(x, dim=1) @ F.normalize(W, dim=1).T
    elif row.op == R.ATTENTION_BWD:
        Nt, H, hd, B = M, N, K, 2
        E = H * hd
        c["qkv"], c["dout"] = rnd(B, Nt, 3 * E, seed=1), rnd(B, Nt, E, seed=2)
        q64 = c["qkv"].double().requires_grad_(True)
        q, k, v = q64.reshape(B, Nt, 3, H, hd).permute(2, 0, 3, 1, 4)
        out = (((q @ k.transpose(-2, -1)) * hd ** -0.5).softmax(-1) @ v).transpose(1, 2).reshape(B, Nt, E)
        out.backward(c["dout"].double())
        c["dqkv"] = q64.grad
    return c


def cosine_layer(K, L):
    """A SOMLayer of K cosine prototypes of L elements: the package's dispatcher of the BMU pass."""
    from vit_som_amd import SOMLayer
    cfg = {"hyperparameters": {"model_arch": "desom", "total_epochs": 1, "batch_size": 8, "ae": {"encoder_dims": [L]},
                               "som": {"map_size": [K, 1], "Tmax": 2.0, "Tmin": 0.5, "distance_fcn": "cosine", "topology": "square"}},
           "data": {"dataset": "synthetic"}}
    return SOMLayer(cfg).to(DEV)


def run(ops, row, c, tol):
    """Launch the row's entry point and compare with the fp64 reference."""
    M, N, K = row.shape
    d = lambda name: c[name].to(DEV)
    new = lambda *s: torch.full(s, float("nan"), device=DEV)
    if row.op == R.LINEAR_FWD:
        assert rel_err(ops.linear_fwd(c["xd"], d("W"), d("b"), new(M, N)).cpu(), c["pre"]) < tol
    elif row.op == R.LINEAR_GELU_FWD:
        grad, act = ops.linear_gelu_fwd(c["xd"], d("W"), d("b"), new(M, N), new(M, N))
        assert float(((act.cpu().double() - c["act"]).abs() / (1 + c["act"].abs())).max()) < 5e-6
        assert float((grad.cpu().double() - c["grad"]).abs().max()) < 5e-6
    elif row.op == R.LINEAR_RELU_FWD:
        act = ops.linear_relu_fwd(c["xd"], d("W"), d("b"), new(M, N), new(M, N))
        assert rel_err(act.cpu(), c["pre"].clamp_min(0)) < tol
    elif row.op == R.LINEAR_RESIDUAL_FWD:
        out = ops.linear_residual_fwd(c["xd"], d("W"), d("b"), d("R"), M, new(M, N))
        assert rel_err(out.cpu(), c["pre"] + c["R"].double()) < tol
    elif row.op in (R.BWD_INPUT, R.BWD_INPUT_GELU):
        gg = d("gg") if row.op == R.BWD_INPUT_GELU else None
        assert rel_err(ops.linear_bwd_input(d("dy"), d("W"), new(M, K), gelu_grad=gg).cpu(), c["ref"]) < tol
    elif row.op in (R.BWD_INPUT_T, R.BWD_INPUT_T_GELU):
        gg = d("gg") if row.op == R.BWD_INPUT_T_GELU else None
        Wt = d("W").T.contiguous()
        assert rel_err(ops.linear_bwd_input_t(d("dy"), Wt, new(M, K), gelu_grad=gg).cpu(), c["ref"]) < tol
    elif row.op == R.BWD_WEIGHT:
        dW, db = new(N, K), new(N)
        ops.linear_bwd_weight(c["dyd"], d("x"), dW, db)
        assert rel_err(dW.cpu(), c["dW"]) < tol
        assert rel_err(db.cpu(), c["db"]) < GEMM_TOL             # a plain fp32 column sum in every mode
    elif row.op == R.BWD_INPUT_LN:
        dx, dg, db = new(M, K), new(K), new(K)
        ops.linear_bwd_input_ln(d("dy"), d("Wt"), d("x"), d("mean"), d("rstd"), d("gamma"), None, dx, dg, db)
        assert rel_err(dx.cpu(), c["dx"]) < tol
        assert rel_err(db.cpu(), c["dbeta"]) < tol
    elif row.op in (R.SOM_BWD_GW, R.SOM_BWD_GX):
        gW, gX = new(N, K), d("gx0").clone()
        ops.som_bwd(d("x"), d("W"), d("coef"), d("rd"), d("cd"), gW, gX, accumulate_gx=True)
        got, ref = (gW, c["gW"]) if row.op == R.SOM_BWD_GW else (gX, c["gX"])
        assert rel_err(got.cpu(), ref) < tol
    elif row.op == R.BMU_COSINE_DOTS:
        xd, Wd = d("x"), d("W")
        inx, inw = torch.empty(M, device=DEV), torch.empty(N, device=DEV)
        ops.row_inv_norm(xd, inx); ops.row_inv_norm(Wd, inw)
        dist, bmu = new(M, N), torch.empty(M, dtype=torch.int64, device=DEV)
        ops.bmu_cosine_fwd(xd, Wd, inx, inw, dist, bmu)
        assert float((dist.cpu().double() - c["d64"]).abs().max()) < 2e-6
        assert torch.equal(bmu.cpu(), dist.cpu().argmin(1))
    elif row.op == R.BMU_COSINE:
        from vit_som_amd.tuning import hooks
        engine = describe(ops.lib, row.op, row.shape, row.aligned)[0]
        form = {"f32": ops.BMU_EXACT, "bmu_x3": ops.BMU_X3, "bmu_x3_planes": ops.BMU_X3_PLANES}[engine]
        xd, Wd = c["xd"], d("W")
        # 1. the form the plan names is the form the package's dispatcher runs: its outputs are, bit for bit, those of the
        #    named form's own wrapper (the three forms differ in dist or in the last bits of the norms)
        som = cosine_layer(N, K)
        som.prototypes.data.copy_(Wd)
        som.invalidate_planes()
        s = som._buffers_for(M, xd.device)
        planes_hook = hooks.bmu_planes
        hooks.set(bmu_planes=bool(row.aligned & 2))
        try:
            assert som._bmu_form(M, xd.stride(0), xd.data_ptr() % 16 == 0) == form
            som._distances_into(xd, s)
        finally:
            hooks.set(bmu_planes=planes_hook)
        dist, bmu = new(M, N), torch.empty(M, dtype=torch.int64, device=DEV)
        inx, inw = torch.empty(M, device=DEV), torch.empty(N, device=DEV)
        if form == ops.BMU_EXACT:
            ops.row_inv_norm(xd, inx); ops.row_inv_norm(Wd, inw)
            ops.bmu_cosine_fwd(xd, Wd, inx, inw, dist, bmu)
        elif form == ops.BMU_X3:
            ops.bmu_cosine_x3_fwd(xd, Wd, dist, bmu, inx, inw)
        else:
            xp, wp = ops.bmu_planes_alloc(M, K, DEV), ops.bmu_planes_alloc(N, K, DEV)
            ops.bmu_planes_from(xd, xp); ops.bmu_planes_from(Wd, wp)
            ops.bmu_cosine_x3_planes_fwd(xd, Wd, xp, wp, dist, bmu, inx, inw)
        for name, got, own in (("dist", s.dist, dist), ("bmu", s.bmu, bmu), ("inx", s.inx, inx), ("inw", s.inw, inw)):
            assert torch.equal(got, own), (engine, name)
        # 2. against fp64: 1e-5 for the three-product forms (test_bmu_cosine_x3_rerank), 2e-6 for the exact one (nt.slab)
        assert float((dist.cpu().double() - c["d64"]).abs().max()) < (2e-6 if form == ops.BMU_EXACT else 1e-5)
        # 3.
        assert torch.equal(bmu.cpu(), dist.cpu().argmin(1))
    elif row.op == R.ATTENTION_BWD:
        Nt, H, hd, B = M, N, K, 2
        qkv = d("qkv")
        out, lse = new(B, Nt, H * hd), new(B, H, Nt)
        ops.attention_fwd(qkv, out, lse, B, Nt, H, hd)
        dqkv, delta = new(B, Nt, 3 * H * hd), new(B, H, Nt)
        ops.attention_bwd(qkv, out, d("dout"), lse, dqkv, delta, B, Nt, H, hd)
        assert rel_err(dqkv.cpu(), c["dqkv"]) < (GRAD3_TOL if tol == GRAD3_TOL else 5e-6)
    else:
        raise AssertionError(row.op)


@pytest.mark.parametrize("mode", R.MODES, ids=["f32", "split_bf16", "grad3"])
@pytest.mark.parametrize("i", range(len(R.PLAN_ROWS)),
                         ids=[f"{r.row}-op{r.op}-{'x'.join(map(str, r.shape))}" for r in R.PLAN_ROWS])
def test_plan_row_against_fp64(ops, i, mode):
    from vit_som_amd._lib import lib
    row = R.PLAN_ROWS[i]
    c = case(i)
    prev = ops.get_gemm_mode()
    setter = getattr(ops, "set_" + row.hook) if row.hook else None
    ops.set_gemm_mode(mode)
    try:
        for hook in (R.HOOK_VALUES[row.hook] if row.hook else (None,)):
            if setter:
                setter(hook)
            want = row.expect[mode]
            if isinstance(want, dict):
                want = want[hook]
            got = describe(lib, row.op, row.shape, row.aligned)
            if want is R.UNSUPPORTED:                       # the entry point refuses what the plan refuses
                assert got is None
                assert not ops.linear_bwd_input_ln_supported(*row.shape)
                continue
            assert got[:4] == want, (hook, got, want)
            run(ops, row, c, GRAD3_TOL if want[2] == 2 else GEMM_TOL)
        torch.cuda.synchronize()
    finally:
        ops.set_gemm_mode(prev)
        if setter:
            setter(R.HOOK_DEFAULTS[row.hook])
