"""Time the LayerNorm-fused input-gradient GEMM (linear_bwd_input_ln_partial: one gemm_x6_ln*_kernel launch) alone at the
encoder's shapes, with both settings of vsom_set_ln_tiles.  usage: ln_gemm_bench.py [iters] [rounds]
Device events around `iters` back-to-back launches after a warm-up; settings alternate per round; min and median per call."""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from vit_som_amd import ops
from vit_som_amd._lib import lib

T, COLS = 33280, 192
iters = int(sys.argv[1]) if len(sys.argv) > 1 else 50
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
assert torch.cuda.is_available(), "ln_gemm_bench.py needs the GPU"
ops.set_gemm_mode(ops.GEMM_SPLIT_BF16_GRAD3)
g = torch.Generator().manual_seed(0)
for name, n in (("fc1", 768), ("qkv", 576)):
    r = lambda *s: torch.randn(*s, generator=g).cuda()
    dy, Wt, x, res = r(T, n), r(COLS, n) * 0.05, r(T, COLS), r(T, COLS)
    mean = x.mean(1).contiguous()
    rstd = torch.rsqrt(x.var(1, unbiased=False) + 1e-6).contiguous()
    gamma = 1 + 0.1 * r(COLS)
    dx = torch.empty_like(x)
    part = torch.empty(lib.vsom_linear_bwd_input_ln_partial_bytes(T, COLS), dtype=torch.uint8, device="cuda")
    call = lambda: ops.linear_bwd_input_ln_partial(dy, Wt, x, mean, rstd, gamma, res, dx, part)
    # HBM floor of one call: dY, X, residual, dX, mean / rstd (the weight and the partials are small)
    hbm = 4 * (T * n + 3 * T * COLS + 2 * T)
    times = {0: [], 1: []}
    for mode in (0, 1):
        ops.set_ln_tiles(mode)
        for _ in range(10):
            call()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for mode in (0, 1):
            ops.set_ln_tiles(mode)
            call()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                call()
            b.record()
            b.synchronize()
            times[mode].append(1e3 * a.elapsed_time(b) / iters)
    for mode in (0, 1):
        t = times[mode]
        print(f"{name} N={n} ln_tiles={mode}: min {min(t):.1f} us  median {statistics.median(t):.1f} us  "
              f"({hbm / min(t) / 1e6:.2f} TB/s of the {hbm / 1e6:.0f} MB HBM floor)  rounds " + " ".join(f"{v:.1f}" for v in t))
ops.set_ln_tiles(1)
