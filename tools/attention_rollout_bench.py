"""Attention rollout on one MI355X: the vector-matrix chain (vsom_attention_rollout_step) against what the library offered
before it for the same map -- vsom_attention_probs over every block plus an fp32 torch chain over the materialised
[B, H, N, N] tensors -- in one process, alternated, device events around single calls, with the spread of every figure;
the peak memory of both paths; and evaluate_attention end to end against evaluate_clustering's loader pass on one loader.

    python tools/attention_rollout_bench.py [--out FILE] [--repeats 7] [--images 4096]

Prints a table and, with --out, writes it to FILE."""
import argparse
import copy
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

SHAPES = [("c3", 512, 65, 3, 64), ("c5 tokens, B 256", 256, 257, 3, 64)]
BLOCKS = 12


def _event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def _alternate(fns, repeats):
    """{name: [ms] * repeats}: the calls alternated, each timed alone between two device events, after one warm call each."""
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            times[k].append(_event_ms(fn)[0])
    return times


def _fmt(ms):
    return f"median {statistics.median(ms):8.3f} ms  min {min(ms):8.3f}  max {max(ms):8.3f}  (n = {len(ms)})"


def _peak(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    del out
    return rise


def _materialised_step(ops, qkv, lse, v, B, N, H, hd, alpha):
    """The parent's path for one block: the [B, H, N, N] probabilities, head mean, residual mix, row sums, one bmm."""
    probs = torch.empty(B, H, N, N, dtype=torch.float32, device=qkv.device)
    ops.attention_probs(qkv, lse, probs, B, N, H, hd)
    F = probs.mean(dim=1)
    A = alpha * F
    A.diagonal(dim1=1, dim2=2).add_(1 - alpha)
    A = A / A.sum(-1, keepdim=True)
    return torch.bmm(v.unsqueeze(1), A).squeeze(1)


def _kernels(lines, repeats):
    from vit_som_amd import ops
    dev = "cuda:0"
    for name, B, N, H, hd in SHAPES:
        g = torch.Generator(device=dev).manual_seed(0)
        qkvs = [torch.randn(B * N, 3 * H * hd, device=dev, generator=g) for _ in range(BLOCKS)]
        lse = torch.zeros(B, H, N, device=dev)              # an argument of the entry that its kernel no longer reads
        w = torch.zeros(B, N, device=dev)
        w[:, 0] = 1.0
        dense = torch.rand(B, N, device=dev, generator=g)
        out = torch.empty(B, N, device=dev)

        def chain_new():
            return ops.attention_rollout(qkvs, w, H, hd, "mean", 0.5)

        def chain_old():
            v = w
            for qkv in reversed(qkvs):
                v = _materialised_step(ops, qkv, lse, v, B, N, H, hd, 0.5)
            return v

        fns = {"rollout step (dense v_in)": lambda: ops.attention_rollout_step(qkvs[0], dense, out, B, N, H, hd, "mean", 0.5),
               "materialised step": lambda: _materialised_step(ops, qkvs[0], lse, dense, B, N, H, hd, 0.5),
               f"rollout chain, {BLOCKS} blocks": chain_new,
               f"materialised chain, {BLOCKS} blocks": chain_old}
        t = _alternate(fns, repeats)
        diff = float((chain_new() - chain_old()).abs().max())
        lines.append(f"{name}: B = {B}, N = {N}, H = {H}, hd = {hd}  (largest |rollout - materialised| of the chains: {diff:.2e})")
        for k in fns:
            lines.append(f"  {k:34s} {_fmt(t[k])}")
        flops = 2.0 * B * H * N * N * hd
        step = statistics.median(t["rollout step (dense v_in)"])
        lines.append(f"  the step's score products: {flops / 1e9:.2f} GFLOP -> {flops / step / 1e9:.1f} TFLOP/s (f32 VALU)")
        lines.append(f"  peak memory over a chain: rollout {_peak(chain_new) / 2**20:9.2f} MiB, materialised {_peak(chain_old) / 2**20:9.2f} MiB "
                     f"(one block's probabilities: {B * H * N * N * 4 / 2**20:.1f} MiB; workspace "
                     f"{ops.attention_rollout_ws_size(B, N, H, hd) / 2**20:.2f} MiB, held by ops.scratch)")
        del qkvs


def _end_to_end(lines, repeats, images):
    import vit_som_amd
    from oracle.gen_golden import make_config
    from vit_som_amd.evaluation import evaluate_attention, evaluate_clustering
    cfg = make_config(3, 32, 4, 192, 12, 3, 96, 2, (40, 40), 0, 512)       # bench.py's architecture: c3
    torch.manual_seed(0)
    model = vit_som_amd.ViTSOM(copy.deepcopy(cfg), device="cuda:0")
    g = torch.Generator().manual_seed(1)
    loader = [(torch.randn(512, 3, 32, 32, generator=g), torch.randint(0, 10, (512,), generator=g)) for _ in range(max(images // 512, 1))]
    quiet = open(os.devnull, "w")

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        stdout, sys.stdout = sys.stdout, quiet
        try:
            fn()
        finally:
            sys.stdout = stdout
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    fns = {"evaluate_clustering": lambda: evaluate_clustering(model, cfg, loader),
           "evaluate_attention": lambda: evaluate_attention(model, cfg, loader)}
    for fn in fns.values():
        timed(fn)
    t = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            t[k].append(timed(fn))
    lines.append(f"end to end, host clock around the entry (a loader of {len(loader)} host batches of 512 images, ViT-SOM c3, 40 x 40 map):")
    for k in fns:
        lines.append(f"  {k:34s} {_fmt(t[k])}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--images", type=int, default=4096)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("attention_rollout_bench: needs the MI355X (a timing taken anywhere else says nothing)")
    lines = [f"attention rollout on {torch.cuda.get_device_name(0)}; {a.repeats} repeats, alternated in one process, device events around "
             f"single calls unless stated"]
    _kernels(lines, a.repeats)
    _end_to_end(lines, a.repeats, a.images)
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
