"""The memory contract of the C-ABI on the MI355X (include/vitsom_hip.h: "scratch is caller-supplied, sized by the matching
*_workspace_bytes() query"): every family runs three times on the same seeded inputs --

  1. plainly, through the ops wrapper, as the rest of the suite does (shared 1 MiB+ scratch, torch's allocator);
  2. with memcheck.ExactScratch in place of ops.scratch (a workspace of exactly the declared size, every byte 0xFF: NaN as
     a float, -1 as an integer), every output a poisoned memcheck.guarded view, every input in a guarded arena whose
     surroundings read as NaN, with 8 padding columns where the entry takes a leading dimension;
  3. the same with the workspace full of 0x7F7FFFFF words (huge, finite).

Every comparison is bitwise: it is the same kernel on the same inputs, only the memory around it differs.  Asserted: every
guard byte and padding element of workspaces, outputs and inputs intact; the outputs of the three runs identical (nothing
depends on what a workspace or an output held before, nothing read from outside an input reaches a result); every fully
written output without a poisoned element left; inputs unchanged.  Buffers that accumulate by contract (accumulate=True,
accumulate_gx, atomically folded counters, AdamW's p / m / v) start from the same values in all three runs instead.

No store can leave a test's own arena at these shapes: the kernels bound every store by the row / column count of the
output or of the slab they were given, so the most an under-reported size query can overrun is the slabs the launch code
addresses, all of them smaller than 1 MiB here (the back guard is max(1 MiB, payload bytes); the front guard 64 KiB)."""
import copy

import numpy as np
import pytest
import torch

import memcheck as MC

pytestmark = pytest.mark.gpu

DEV = "cuda"
PAD = 8                                       # padding columns of a strided operand: keeps ld % 4 (the vector-load path)


@pytest.fixture(scope="module")
def ops():
    """The ops module, with every hook the tests below move put back afterwards."""
    from vit_som_amd import ops as _ops
    prev = _ops.get_gemm_mode()
    yield _ops
    _ops.set_gemm_mode(prev)
    _ops.set_wgrad_tiles(2)
    _ops.set_ln_tiles(1)
    _ops.set_attention_fused(1)


MODES = {"grad3": 2, "split_bf16": 1, "f32": 0}


@pytest.fixture(params=list(MODES))
def gemm_mode(request, ops):
    prev = ops.get_gemm_mode()
    ops.set_gemm_mode(MODES[request.param])
    yield request.param
    ops.set_gemm_mode(prev)


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def randint(lo, hi, shape, seed=0):
    return torch.randint(lo, hi, shape, generator=torch.Generator().manual_seed(seed))


# ------------------------------------------------------------------ the three runs
class In:
    """An input: guarded, surrounded by NaN, `pad` extra columns per row in the guarded runs."""
    def __init__(self, t, pad=0):
        self.t, self.pad = t, pad


class Out:
    """An output the entry writes completely (written=False: guards and equality only, e.g. uint8 images)."""
    def __init__(self, shape, dtype=torch.float32, pad=0, written=True):
        self.shape, self.dtype, self.pad, self.written = tuple(shape), dtype, pad, written


class Acc:
    """A buffer the entry accumulates into or writes in part: starts from the same values in every run."""
    def __init__(self, t, pad=0):
        self.t, self.pad = t, pad


class Ws:
    """A workspace the entry takes from its caller: exactly `nbytes` bytes, guarded, filled like ExactScratch's."""
    def __init__(self, nbytes):
        self.nbytes = int(nbytes)


def bits(t):
    """The tensor's bits as integers: NaN compares equal to itself, -0.0 differs from 0.0."""
    t = t.contiguous()
    return t.view({4: torch.int32, 8: torch.int64, 1: torch.uint8}[t.element_size()]) if t.is_floating_point() else t


def same(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def contract(monkeypatch, ops, call, expect_scratch=None, **named):
    """Run `call(**tensors)` three times as the module docstring says.  named: In / Out / Acc / Ws, anything else is handed
    through.  `call` may return a dict of further device tensors to compare.  -> the plain run's tensors (dict)."""
    def plain():
        t = {}
        for name, s in named.items():
            if isinstance(s, (In, Acc)):
                t[name] = s.t.to(DEV).clone()
            elif isinstance(s, Out):
                t[name] = torch.empty(s.shape, dtype=s.dtype, device=DEV)
            elif isinstance(s, Ws):
                t[name] = torch.zeros(s.nbytes, dtype=torch.uint8, device=DEV)
            else:
                t[name] = s
        return t

    ref = plain()
    extra_ref = call(**ref)
    extra_ref = extra_ref if isinstance(extra_ref, dict) else {}
    torch.cuda.synchronize()
    for fill in (MC.FILL_FF, MC.FILL_HUGE):
        es = MC.ExactScratch(fill)
        t, handles = {}, {}
        for name, s in named.items():
            if isinstance(s, (In, Acc)):
                src = s.t.to(DEV)
                ld = src.shape[-1] + s.pad if s.pad else None
                t[name], handles[name] = MC.guarded_copy(src, ld=ld)
            elif isinstance(s, Out):
                t[name], handles[name] = MC.guarded(s.shape, s.dtype, DEV, ld=s.shape[-1] + s.pad if s.pad else None)
            elif isinstance(s, Ws):
                handles[name] = MC.Guarded((s.nbytes,), torch.uint8, DEV, poison=False)
                t[name] = handles[name].view
                es._fill(t[name])
            else:
                t[name] = s
        with monkeypatch.context() as mp:
            mp.setattr(ops, "scratch", es)
            extra = call(**t)
            extra = extra if isinstance(extra, dict) else {}
        torch.cuda.synchronize()
        what = f"[{fill} fill]"
        if expect_scratch is not None:
            assert (es.calls > 0) == expect_scratch, f"{what} the wrapper asked for {es.calls} workspaces"
        es.check()
        for name, h in handles.items():
            h.check(f"{what} {name}")
        for name, s in named.items():
            if isinstance(s, In):
                assert same(t[name], s.t.to(DEV)), f"{what} input {name} was modified"
            elif isinstance(s, Out):
                if s.written:
                    handles[name].all_written(f"{what} {name}")
                assert same(t[name], ref[name]), f"{what} output {name} differs from the plain run"
            elif isinstance(s, Acc):
                assert same(t[name], ref[name]), f"{what} accumulated {name} differs from the plain run"
        assert set(extra) == set(extra_ref)
        for name in extra:
            assert same(extra[name], extra_ref[name]), f"{what} result {name} differs from the plain run"
    return ref


def test_the_harness_catches_a_stray_store_on_the_device(monkeypatch, ops):
    """What test_memory_contract_cpu.py shows on CPU tensors, once on the device: a store one element past a guarded output,
    into a padding column, past an exact workspace, and an element left out are each caught (all inside the test's arenas)."""
    v, h = MC.guarded((33, 10), torch.float32, DEV, ld=18)
    v.zero_()
    torch.cuda.synchronize()
    h.check(); h.all_written()
    flat = h.arena[h.off:h.off + h.nbytes + 4].view(torch.float32)
    flat[10] = 1.0
    with pytest.raises(AssertionError, match="padding column"):
        h.check()
    flat[10] = flat[11]
    flat[-1] = 1.0
    with pytest.raises(AssertionError, match=rf"byte offset {h.nbytes} from the payload start \(the back guard"):
        h.check()
    v2, h2 = MC.guarded((7,), torch.int64, DEV)
    v2[:6] = 0
    with pytest.raises(AssertionError, match="flat index 6"):
        h2.all_written()
    es = MC.ExactScratch(MC.FILL_HUGE)
    with monkeypatch.context() as mp:
        mp.setattr(ops, "scratch", es)
        ws = ops.scratch(1000, DEV)
    assert ws.numel() == 1000 and ws.data_ptr() % 256 == 0 and bool((ws.view(torch.int32) == 0x7F7FFFFF).all())
    es.check()
    arena = next(iter(es.arenas.values()))
    arena.arena[arena.off + 1000] = 0
    with pytest.raises(AssertionError, match="workspace of 1000 bytes"):
        es.check()


# ------------------------------------------------------------------ Linear: forward and input gradient (no workspace)
LINEAR_SHAPES = [(33, 10, 24), (70, 50, 48), (257, 576, 192), (193, 192, 192)]


@pytest.mark.parametrize("M,N,K", LINEAR_SHAPES)
def test_linear_forward_family(monkeypatch, ops, gemm_mode, M, N, K):
    x, W, b = rnd(M, K, seed=1), rnd(N, K, seed=2, scale=0.1), rnd(N, seed=3)
    contract(monkeypatch, ops, lambda **t: ops.linear_fwd(t["x"], t["W"], t["b"], t["out"]), expect_scratch=False,
             x=In(x, PAD), W=In(W), b=In(b), out=Out((M, N), pad=PAD))
    contract(monkeypatch, ops, lambda **t: ops.linear_fwd(t["x"], t["W"], None, t["out"]),
             x=In(x, PAD), W=In(W), out=Out((M, N), pad=PAD))
    contract(monkeypatch, ops, lambda **t: ops.linear_gelu_fwd(t["x"], t["W"], t["b"], t["grad"], t["act"]),
             x=In(x, PAD), W=In(W), b=In(b), grad=Out((M, N)), act=Out((M, N)))
    contract(monkeypatch, ops, lambda **t: ops.linear_relu_fwd(t["x"], t["W"], t["b"], t["grad"], t["act"]),
             x=In(x, PAD), W=In(W), b=In(b), grad=Out((M, N)), act=Out((M, N)))
    rmod = M // 2 if M % 2 == 0 else M
    contract(monkeypatch, ops, lambda **t: ops.linear_residual_fwd(t["x"], t["W"], t["b"], t["R"], rmod, t["out"]),
             x=In(x, PAD), W=In(W), b=In(b), R=In(rnd(rmod, N, seed=4), PAD), out=Out((M, N), pad=PAD))


@pytest.mark.parametrize("M,N,K", LINEAR_SHAPES)
def test_linear_input_gradient_family(monkeypatch, ops, gemm_mode, M, N, K):
    dy, W, base, gg = rnd(M, N, seed=1), rnd(N, K, seed=2, scale=0.1), rnd(M, K, seed=5), rnd(M, K, seed=6)
    Wt = W.T.contiguous()
    for fn, w in ((ops.linear_bwd_input, W), (ops.linear_bwd_input_t, Wt)):
        contract(monkeypatch, ops, lambda **t: fn(t["dy"], t["w"], t["dx"]), expect_scratch=False,
                 dy=In(dy, PAD), w=In(w), dx=Out((M, K), pad=PAD))
        contract(monkeypatch, ops, lambda **t: fn(t["dy"], t["w"], t["dx"], accumulate=True),
                 dy=In(dy, PAD), w=In(w), dx=Acc(base, PAD))
        contract(monkeypatch, ops, lambda **t: fn(t["dy"], t["w"], t["dx"], gelu_grad=t["gg"]),
                 dy=In(dy, PAD), w=In(w), gg=In(gg), dx=Out((M, K), pad=PAD))


# ------------------------------------------------------------------ weight gradient (split-K slabs + bias partials)
@pytest.mark.parametrize("tiles", [0, 1, 2])
@pytest.mark.parametrize("M,N,K", [(33, 4, 16), (70, 10, 24), (257, 96, 96), (257, 192, 64), (257, 192, 192)])
def test_linear_bwd_weight(monkeypatch, ops, gemm_mode, tiles, M, N, K):
    """The size is queried by the wrapper under the same mode and tile hook as the launch."""
    ops.set_wgrad_tiles(tiles)
    try:
        dy, x = rnd(M, N, seed=1), rnd(M, K, seed=2)
        contract(monkeypatch, ops, lambda **t: ops.linear_bwd_weight(t["dy"], t["x"], t["dW"], t["db"]), expect_scratch=True,
                 dy=In(dy, PAD), x=In(x, PAD), dW=Out((N, K)), db=Out((N,)))
        contract(monkeypatch, ops, lambda **t: ops.linear_bwd_weight(t["dy"], t["x"], t["dW"], None), expect_scratch=True,
                 dy=In(dy, PAD), x=In(x, PAD), dW=Out((N, K)))
    finally:
        ops.set_wgrad_tiles(2)


@pytest.mark.parametrize("B,C,S,p,E", [(3, 3, 8, 4, 24), (6, 3, 32, 4, 192)])
def test_patch_embed(monkeypatch, ops, gemm_mode, B, C, S, p, E):
    n, pd = (S // p) ** 2, C * p * p
    img, W, b = rnd(B, C, S, S, seed=1), rnd(E, pd, seed=2, scale=0.2), rnd(E, seed=3)
    pos, cls = rnd(n + 1, E, seed=4), rnd(E, seed=5)
    r = contract(monkeypatch, ops,
                 lambda **t: ops.patch_embed_fwd(t["img"], t["W"], t["b"], t["pos"], t["cls"], t["tokens"], t["xp"], p),
                 expect_scratch=False, img=In(img), W=In(W), b=In(b), pos=In(pos), cls=In(cls),
                 tokens=Out((B, n + 1, E)), xp=Out((B * n, pd)))
    contract(monkeypatch, ops, lambda **t: ops.patch_embed_bwd(t["dt"], t["xp"], t["dW"], t["db"], t["dc"], B, C, S, p, E),
             expect_scratch=True, dt=In(rnd(B, n + 1, E, seed=6)), xp=In(r["xp"]), dW=Out((E, pd)), db=Out((E,)), dc=Out((E,)))


# ------------------------------------------------------------------ LayerNorm
def _ln_case(rows, cols, seed=0):
    x = rnd(rows, cols, seed=seed + 1) * 2 + 0.5
    g, b = 1 + 0.1 * rnd(cols, seed=seed + 2), 0.1 * rnd(cols, seed=seed + 3)
    return x, g, b, rnd(rows, cols, seed=seed + 4), rnd(rows, cols, seed=seed + 5)


@pytest.mark.parametrize("rows,cols", [(20, 4), (37, 16), (130, 192), (9, 768), (8200, 192)])     # the last: the 512-workgroup cap
def test_layernorm(monkeypatch, ops, rows, cols):
    x, g, b, dy, resid = _ln_case(rows, cols)
    r = contract(monkeypatch, ops,
                 lambda **t: ops.layernorm_fwd(t["x"], t["g"], t["b"], t["y"], t["mean"], t["rstd"], 1e-6), expect_scratch=False,
                 x=In(x), g=In(g), b=In(b), y=Out((rows, cols)), mean=Out((rows,)), rstd=Out((rows,)))
    for res in (resid, None):
        contract(monkeypatch, ops,
                 lambda **t: ops.layernorm_bwd(t["dy"], t["x"], t["mean"], t["rstd"], t["g"], t.get("resid"), t["dx"], t["dg"], t["db"]),
                 expect_scratch=True, dy=In(dy), x=In(x), mean=In(r["mean"]), rstd=In(r["rstd"]), g=In(g),
                 dx=Out((rows, cols)), dg=Out((cols,)), db=Out((cols,)), **({"resid": In(res)} if res is not None else {}))


def _finish_one(ops, part, dgamma, dbeta, cols):
    """vsom_layernorm_bwd_finish_many on a one-job table over the caller's partial buffer (what LayerNormJobs.flush does)."""
    from vit_som_amd._lib import check, lib, ptr, stream
    table = torch.tensor([[ptr(part), ptr(dgamma), ptr(dbeta), ((part.numel() // (8 * cols)) << 32) | cols]],
                         dtype=torch.int64, device=DEV)
    check(lib.vsom_layernorm_bwd_finish_many(ptr(table), 0, 1, cols, stream()), "vsom_layernorm_bwd_finish_many")
    return table


# 1985 = 31 * 64 + 1 and 3969 = 31 * 128 + 1: exactly 32 partial rows, one live row in the last
@pytest.mark.parametrize("rows,n,cols", [(1985, 64, 192), (3969, 64, 96)])
def test_layernorm_bwd_partial_and_finish_many(monkeypatch, ops, rows, n, cols):
    from vit_som_amd._lib import check, lib, ptr, stream
    assert ops.layernorm_bwd_deferrable(rows, cols)
    x, g, b, dy, resid = _ln_case(rows, cols, seed=10)
    xd = x.to(DEV)
    mean, rstd = xd.mean(1).contiguous(), torch.rsqrt(xd.var(1, unbiased=False) + 1e-6).contiguous()
    need = lib.vsom_layernorm_bwd_workspace_bytes(rows, cols)

    def call(**t):
        check(lib.vsom_layernorm_bwd_partial(ptr(t["dy"]), ptr(t["x"]), ptr(t["mean"]), ptr(t["rstd"]), ptr(t["g"]), ptr(t["resid"]),
                                             ptr(t["dx"]), rows, cols, ptr(t["part"]), t["part"].numel(), stream()),
              "vsom_layernorm_bwd_partial")
        keep = _finish_one(ops, t["part"], t["dg"], t["db"], cols)
        torch.cuda.synchronize()
        del keep

    r = contract(monkeypatch, ops, call, expect_scratch=False, dy=In(dy), x=In(x), mean=In(mean), rstd=In(rstd), g=In(g),
                 resid=In(resid), dx=Out((rows, cols)), dg=Out((cols,)), db=Out((cols,)), part=Ws(need))
    # the one-call form gives the same bits
    dx, dg, db = torch.empty(rows, cols, device=DEV), torch.empty(cols, device=DEV), torch.empty(cols, device=DEV)
    ops.layernorm_bwd(dy.to(DEV), xd, mean, rstd, g.to(DEV), resid.to(DEV), dx, dg, db)
    assert same(dx, r["dx"]) and same(dg, r["dg"]) and same(db, r["db"])


@pytest.mark.parametrize("mode", [1, 2])                      # the two split modes: the fused form does not exist in GEMM_F32
@pytest.mark.parametrize("rows,n,cols,ln_tiles", [(1985, 64, 192, 0), (1985, 64, 192, 1), (3969, 64, 96, 1)])     # the hook acts at 192
def test_linear_bwd_input_ln(monkeypatch, ops, mode, rows, n, cols, ln_tiles):
    from vit_som_amd._lib import lib
    prev = ops.get_gemm_mode()
    ops.set_gemm_mode(mode)
    ops.set_ln_tiles(ln_tiles)
    try:
        assert ops.linear_bwd_input_ln_supported(rows, n, cols)
        x, g, b, _, resid = _ln_case(rows, cols, seed=20)
        dy, Wt = rnd(rows, n, seed=7), rnd(cols, n, seed=8, scale=0.05)
        xd = x.to(DEV)
        mean, rstd = xd.mean(1).contiguous(), torch.rsqrt(xd.var(1, unbiased=False) + 1e-6).contiguous()
        common = dict(dy=In(dy, PAD), Wt=In(Wt), x=In(x), mean=In(mean), rstd=In(rstd), g=In(g), resid=In(resid))
        one = contract(monkeypatch, ops,
                       lambda **t: ops.linear_bwd_input_ln(t["dy"], t["Wt"], t["x"], t["mean"], t["rstd"], t["g"], t["resid"], t["dx"],
                                                           t["dg"], t["db"]),
                       expect_scratch=True, dx=Out((rows, cols)), dg=Out((cols,)), db=Out((cols,)), **common)

        def deferred(**t):
            ops.linear_bwd_input_ln_partial(t["dy"], t["Wt"], t["x"], t["mean"], t["rstd"], t["g"], t["resid"], t["dx"], t["part"])
            keep = _finish_one(ops, t["part"], t["dg"], t["db"], cols)
            torch.cuda.synchronize()
            del keep

        two = contract(monkeypatch, ops, deferred, expect_scratch=False, dx=Out((rows, cols)), dg=Out((cols,)), db=Out((cols,)),
                       part=Ws(lib.vsom_linear_bwd_input_ln_partial_bytes(rows, cols)), **common)
        assert same(one["dx"], two["dx"]) and same(one["dg"], two["dg"]) and same(one["db"], two["db"])
    finally:
        ops.set_ln_tiles(1)
        ops.set_gemm_mode(prev)


# ------------------------------------------------------------------ attention (outputs and inputs only)
@pytest.mark.parametrize("fused", [0, 1, 2, 3])
@pytest.mark.parametrize("B,N,H,hd", [(2, 5, 3, 4), (2, 37, 2, 2), (2, 17, 1, 64), (2, 65, 3, 64)])
def test_attention(monkeypatch, ops, fused, B, N, H, hd):
    E = H * hd
    qkv, dout = rnd(B, N, 3 * E, seed=1), rnd(B, N, E, seed=2)
    ops.set_attention_fused(fused)
    try:
        f = contract(monkeypatch, ops, lambda **t: ops.attention_fwd(t["qkv"], t["out"], t["lse"], B, N, H, hd), expect_scratch=False,
                     qkv=In(qkv), out=Out((B, N, E)), lse=Out((B, H, N)))
        contract(monkeypatch, ops,
                 lambda **t: ops.attention_bwd(t["qkv"], t["out"], t["dout"], t["lse"], t["dqkv"], t["delta"], B, N, H, hd),
                 expect_scratch=False, qkv=In(qkv), out=In(f["out"]), dout=In(dout), lse=In(f["lse"]),
                 dqkv=Out((B, N, 3 * E)), delta=Out((B, H, N)))
        contract(monkeypatch, ops, lambda **t: ops.attention_probs(t["qkv"], t["lse"], t["probs"], B, N, H, hd),
                 qkv=In(qkv), lse=In(f["lse"]), probs=Out((B, H, N, N)))
        if fused == 1:                               # the single-query form has no switch; it takes head sizes 8, 16, 32, 64
            hd = hd if hd >= 8 else 8
            E = H * hd
            q, kv = rnd(B, E, seed=3), rnd(B * N, 2 * E, seed=4)
            f1 = contract(monkeypatch, ops, lambda **t: ops.attention_q1_fwd(t["q"], t["kv"], t["out"], t["lse"], B, N, H, hd),
                          q=In(q), kv=In(kv), out=Out((B, E)), lse=Out((B, H)))
            contract(monkeypatch, ops,
                     lambda **t: ops.attention_q1_bwd(t["dout"], t["out"], t["lse"], t["q"], t["kv"], t["dq"], t["dkv"], B, N, H, hd),
                     dout=In(rnd(B, E, seed=5)), out=In(f1["out"]), lse=In(f1["lse"]), q=In(q), kv=In(kv),
                     dq=Out((B, E)), dkv=Out((B * N, 2 * E)))
    finally:
        ops.set_attention_fused(1)


# ------------------------------------------------------------------ BMU
def _protos(K, L, seed=2):
    return torch.nn.functional.normalize(torch.rand(K, L, generator=torch.Generator().manual_seed(seed)), dim=1)


@pytest.mark.parametrize("B,K,L", [(5, 7, 20), (33, 100, 48), (70, 15, 256)])
def test_bmu_cosine_and_euclid(monkeypatch, ops, gemm_mode, B, K, L):
    x, W = rnd(B, L, seed=1), _protos(K, L)
    n = {}
    for name, fn in (("inv", ops.row_inv_norm), ("sq", ops.row_sqnorm)):
        n[name + "x"] = contract(monkeypatch, ops, lambda **t: fn(t["x"], t["o"]), expect_scratch=False, x=In(x, PAD), o=Out((B,)))["o"]
        n[name + "w"] = contract(monkeypatch, ops, lambda **t: fn(t["x"], t["o"]), x=In(W), o=Out((K,)))["o"]
    for fn, a, b in ((ops.bmu_cosine_fwd, "invx", "invw"), (ops.bmu_euclid_fwd, "sqx", "sqw")):
        full = contract(monkeypatch, ops, lambda **t: fn(t["x"], t["W"], t["nx"], t["nw"], t["dist"], t["bmu"]), expect_scratch=True,
                        x=In(x, PAD), W=In(W), nx=In(n[a]), nw=In(n[b]), dist=Out((B, K)), bmu=Out((B,), torch.int64))
        lean = contract(monkeypatch, ops, lambda **t: fn(t["x"], t["W"], t["nx"], t["nw"], None, t["bmu"]), expect_scratch=True,
                        x=In(x, PAD), W=In(W), nx=In(n[a]), nw=In(n[b]), bmu=Out((B,), torch.int64))
        assert same(full["bmu"], lean["bmu"])


# (193, 193, 72): the B >= 192 path with a ragged second tile in both directions
@pytest.mark.parametrize("B,K,L", [(5, 8, 20), (70, 15, 256), (193, 193, 72)])
def test_bmu_cosine_x3(monkeypatch, ops, B, K, L):
    x, W = rnd(B, L, seed=1), _protos(K, L)
    zero = torch.zeros(1, dtype=torch.int32)
    contract(monkeypatch, ops,
             lambda **t: ops.bmu_cosine_x3_fwd(t["x"], t["W"], t["dist"], t["bmu"], t["inx"], t["inw"], t["cnt"]), expect_scratch=True,
             x=In(x, PAD), W=In(W), dist=Out((B, K)), bmu=Out((B,), torch.int64), inx=Out((B,)), inw=Out((K,)), cnt=Acc(zero))
    contract(monkeypatch, ops, lambda **t: ops.bmu_cosine_x3_fwd(t["x"], t["W"], None, t["bmu"], t["inx"], t["inw"]),
             expect_scratch=True, x=In(x, PAD), W=In(W), bmu=Out((B,), torch.int64), inx=Out((B,)), inw=Out((K,)))


@pytest.mark.parametrize("B,K,L", [(192, 33, 8), (200, 70, 72)])
def test_bmu_planes(monkeypatch, ops, B, K, L):
    """The plane buffers are the caller's: guarded views of exactly vsom_bmu_planes_bytes bytes.  (An image's padding rows
    belong to nobody: the buffers start from zeros, as the optimiser's do.)"""
    from vit_som_amd._lib import lib
    assert ops.get_gemm_mode() != ops.GEMM_F32 and ops.bmu_planes_supported(B, K, L)
    x, W = rnd(B, L, seed=3), _protos(K, L, seed=4)
    xp = contract(monkeypatch, ops, lambda **t: ops.bmu_planes_from(t["src"], t["planes"]), expect_scratch=False,
                  src=In(x, PAD), planes=Acc(torch.zeros(lib.vsom_bmu_planes_bytes(B, L), dtype=torch.uint8)))["planes"]
    wp = contract(monkeypatch, ops, lambda **t: ops.bmu_planes_from(t["src"], t["planes"]),
                  src=In(W), planes=Acc(torch.zeros(lib.vsom_bmu_planes_bytes(K, L), dtype=torch.uint8)))["planes"]
    zero = torch.zeros(1, dtype=torch.int32)
    contract(monkeypatch, ops,
             lambda **t: ops.bmu_cosine_x3_planes_fwd(t["x"], t["W"], t["xp"], t["wp"], t["dist"], t["bmu"], t["inx"], t["inw"], t["cnt"]),
             expect_scratch=True, x=In(x, PAD), W=In(W), xp=In(xp), wp=In(wp), dist=Out((B, K)), bmu=Out((B,), torch.int64),
             inx=Out((B,)), inw=Out((K,)), cnt=Acc(zero))


def test_adamw_step_planes(monkeypatch, ops):
    """The setup of test_adamw_step_planes_is_the_flat_step_plus_the_split, the plane buffer guarded and exact."""
    from vit_som_amd._lib import lib
    R, L = 70, 136
    lead, tail = 256 * 3, 256 * 2
    padded = (R * L + 255) // 256 * 256
    n = lead + padded + tail
    g0 = torch.Generator().manual_seed(0)
    p, gr = torch.randn(n, generator=g0), torch.randn(n, generator=g0)
    p[lead + R * L:lead + padded] = 0; gr[lead + R * L:lead + padded] = 0
    wd = torch.rand(n // 256, generator=g0) * 0.05
    zeros = torch.zeros(n)
    for adamw in (True, False):
        def call(**t):
            ops.adamw_step(t["p"], t["g"], t["m"], t["v"], t["wd"], 3e-3, 0.9, 0.999, 1e-8, 2, grad_scale=0.5, adamw=adamw,
                           planes=(lead, R, L, t["planes"]))
        r = contract(monkeypatch, ops, call, expect_scratch=False, p=Acc(p), g=In(gr), m=Acc(zeros), v=Acc(zeros), wd=In(wd),
                     planes=Acc(torch.zeros(lib.vsom_bmu_planes_bytes(R, L), dtype=torch.uint8)))
        flat = contract(monkeypatch, ops,
                        lambda **t: ops.adamw_step(t["p"], t["g"], t["m"], t["v"], t["wd"], 3e-3, 0.9, 0.999, 1e-8, 2, grad_scale=0.5,
                                                   adamw=adamw),
                        expect_scratch=False, p=Acc(p), g=In(gr), m=Acc(zeros), v=Acc(zeros), wd=In(wd))
        assert same(r["p"], flat["p"]) and same(r["m"], flat["m"]) and same(r["v"], flat["v"])


@pytest.mark.parametrize("B,K,L", [(33, 12, 48), (70, 65, 100)])
def test_bmu_manhattan_and_its_backward(monkeypatch, ops, B, K, L):
    x, W = rnd(B, L, seed=1), torch.rand(K, L, generator=torch.Generator().manual_seed(2))
    contract(monkeypatch, ops, lambda **t: ops.bmu_manhattan_fwd(t["x"], t["W"], t["dist"], t["bmu"]), expect_scratch=True,
             x=In(x, PAD), W=In(W), dist=Out((B, K)), bmu=Out((B,), torch.int64))
    contract(monkeypatch, ops, lambda **t: ops.bmu_manhattan_fwd(t["x"], t["W"], None, t["bmu"]), expect_scratch=True,
             x=In(x, PAD), W=In(W), bmu=Out((B,), torch.int64))
    coef = rnd(B, K, seed=3, scale=1e-3)
    contract(monkeypatch, ops, lambda **t: ops.som_bwd_manhattan(t["x"], t["W"], t["coef"], t["gW"], t["gX"], accumulate_gx=False),
             expect_scratch=False, x=In(x, PAD), W=In(W), coef=In(coef), gW=Out((K, L)), gX=Out((B, L), pad=PAD))
    contract(monkeypatch, ops, lambda **t: ops.som_bwd_manhattan(t["x"], t["W"], t["coef"], t["gW"], t["gX"], accumulate_gx=True),
             x=In(x, PAD), W=In(W), coef=In(coef), gW=Out((K, L)), gX=Acc(rnd(B, L, seed=9), PAD))


# ------------------------------------------------------------------ SOM loss and backward
@pytest.mark.parametrize("distance", [0, 1, 2])               # cosine, euclidean, manhattan
@pytest.mark.parametrize("B,K", [(33, 12), (70, 15)])
def test_som_loss_and_backward(monkeypatch, ops, gemm_mode, distance, B, K):
    L = 48
    x, W = rnd(B, L, seed=1), _protos(K, L)
    dist = torch.rand(B, K, generator=torch.Generator().manual_seed(3)) + 0.1
    bmu = dist.argmin(1)
    grid = torch.stack([torch.arange(K) // 4, torch.arange(K) % 4], 1).float()
    inx, inw = 1 / x.norm(dim=1), 1 / W.norm(dim=1)
    outs = dict(coef=Out((B, K))) if distance == 2 else dict(coef=Out((B, K)), rd=Out((B,)), cd=Out((K,)))
    norms = dict(inx=In(inx), inw=In(inw)) if distance == 0 else {}
    r = contract(monkeypatch, ops,
                 lambda **t: ops.som_neigh_loss(t["dist"], t["bmu"], t["grid"], 1.7, t["loss"], h=t["h"], inv_nx=t.get("inx"),
                                                inv_nw=t.get("inw"), grad_scale=0.37 / (B * K), coef=t["coef"], row_dot=t.get("rd"),
                                                col_dot=t.get("cd"), distance=distance),
                 expect_scratch=True, dist=In(dist), bmu=In(bmu), grid=In(grid), loss=Out((1,)), h=Out((B, K)), **outs, **norms)
    lean = contract(monkeypatch, ops, lambda **t: ops.som_neigh_loss(t["dist"], t["bmu"], t["grid"], 1.7, t["loss"], distance=distance),
                    expect_scratch=True, dist=In(dist), bmu=In(bmu), grid=In(grid), loss=Out((1,)))
    assert same(r["loss"], lean["loss"])
    contract(monkeypatch, ops,
             lambda **t: ops.som_weighted_loss(t["dist"], t["w"], t["loss"], inv_nx=t.get("inx"), inv_nw=t.get("inw"),
                                               grad_scale=0.37 / (B * K), coef=t["coef"], row_dot=t.get("rd"), col_dot=t.get("cd"),
                                               distance=distance),
             expect_scratch=True, dist=In(dist), w=In(r["h"]), loss=Out((1,)), **outs, **norms)
    if distance != 2:
        for acc in (False, True):
            gx = Acc(rnd(B, L, seed=9, scale=1e-5), PAD) if acc else Out((B, L), pad=PAD)
            contract(monkeypatch, ops,
                     lambda **t: ops.som_bwd(t["x"], t["W"], t["coef"], t["rd"], t["cd"], t["gW"], t["gX"], accumulate_gx=acc),
                     expect_scratch=False, x=In(x, PAD), W=In(W), coef=In(r["coef"]), rd=In(r["rd"]), cd=In(r["cd"]),
                     gW=Out((K, L)), gX=gx)


# ------------------------------------------------------------------ losses
@pytest.mark.parametrize("n", [7, 1024, 1025, 128 * 784 + 3])
def test_l1_loss(monkeypatch, ops, n):
    p, t_ = rnd(n, seed=1), rnd(n, seed=2)
    p[:2] = t_[:2]
    contract(monkeypatch, ops, lambda **t: ops.l1_loss(t["p"], t["t"], t["loss"], dpred=t["dp"], grad_scale=0.25), expect_scratch=True,
             p=In(p), t=In(t_), loss=Out((1,)), dp=Out((n,)))
    contract(monkeypatch, ops, lambda **t: ops.l1_loss(t["p"], t["t"], t["loss"]), expect_scratch=True,
             p=In(p), t=In(t_), loss=Out((1,)))


@pytest.mark.parametrize("B,C,S,p", [(3, 3, 8, 4), (4, 1, 28, 2)])
def test_l1_unpatchify(monkeypatch, ops, B, C, S, p):
    n = (S // p) ** 2
    pred, img = rnd(B, n + 1, p * p * C, seed=1), rnd(B, C, S, S, seed=2)
    contract(monkeypatch, ops,
             lambda **t: ops.l1_unpatchify(t["pred"], t["img"], t["loss"], recon=t["recon"], dpred=t["dpred"],
                                           grad_scale=1.0 / img.numel(), p=p),
             expect_scratch=True, pred=In(pred), img=In(img), loss=Out((1,)), recon=Out((B, C, S, S)), dpred=Out(pred.shape))
    contract(monkeypatch, ops, lambda **t: ops.l1_unpatchify(t["pred"], t["img"], t["loss"], p=p), expect_scratch=True,
             pred=In(pred), img=In(img), loss=Out((1,)))


@pytest.mark.parametrize("B,C", [(7, 5), (33, 100)])
def test_cross_entropy_ls(monkeypatch, ops, B, C):
    z, y = rnd(B, C, seed=1) * 3, randint(0, C, (B,), seed=2)
    contract(monkeypatch, ops, lambda **t: ops.cross_entropy_ls(t["z"], t["y"], 0.1, t["loss"], dlogits=t["dz"], grad_scale=1.0 / B),
             expect_scratch=True, z=In(z), y=In(y), loss=Out((1,)), dz=Out((B, C)))
    contract(monkeypatch, ops, lambda **t: ops.cross_entropy_ls(t["z"], t["y"], 0.1, t["loss"]), expect_scratch=True,
             z=In(z), y=In(y), loss=Out((1,)))


# ------------------------------------------------------------------ the kNN family
KNN_N, KNN_NQ = 257, 129


@pytest.mark.parametrize("metric", [0, 1])                    # cosine, euclidean
@pytest.mark.parametrize("k", [3, 64])
@pytest.mark.parametrize("D", [5, 8])                         # the element-wise and the vector load path
def test_knn_search_and_ranks(monkeypatch, ops, D, k, metric):
    X, Q = rnd(KNN_N, D, seed=1), rnd(KNN_NQ, D, seed=2)
    own = contract(monkeypatch, ops, lambda **t: ops.umap_knn(t["X"], k, metric, t["idx"], t["dist"]), expect_scratch=True,
                   X=In(X, PAD), idx=Out((KNN_N, k), torch.int64), dist=Out((KNN_N, k)))
    # the bank in two chunks: the second call folds its candidates into the lists of the first
    first = contract(monkeypatch, ops, lambda **t: ops.knn_query(t["Q"], t["X"], k, metric, t["idx"], t["dist"]), expect_scratch=True,
                     Q=In(Q, PAD), X=In(X[:128], PAD), idx=Out((KNN_NQ, k), torch.int64), dist=Out((KNN_NQ, k)))
    both = contract(monkeypatch, ops,
                    lambda **t: ops.knn_query(t["Q"], t["X"], k, metric, t["idx"], t["dist"], index_base=128, accumulate=True),
                    expect_scratch=True, Q=In(Q, PAD), X=In(X[128:], PAD), idx=Acc(first["idx"]), dist=Acc(first["dist"]))
    whole = contract(monkeypatch, ops, lambda **t: ops.knn_query(t["Q"], t["X"], k, metric, t["idx"], t["dist"], exclude=t["ex"]),
                     expect_scratch=True, Q=In(Q, PAD), X=In(X, PAD), ex=In(torch.arange(KNN_NQ) * 2),
                     idx=Out((KNN_NQ, k), torch.int64), dist=Out((KNN_NQ, k)))
    assert bool((whole["idx"] != (torch.arange(KNN_NQ, device=DEV) * 2)[:, None]).all())
    assert bool((both["idx"] >= 0).all()) and bool((both["idx"] < KNN_N).all())
    nbr = own["idx"].clone()
    nbr[::7, -1] = -1                                        # some empty slots
    contract(monkeypatch, ops, lambda **t: ops.knn_ranks(t["A"], t["nbr"], metric, t["less"], t["tied"]), expect_scratch=True,
             A=In(X, PAD), nbr=In(nbr), less=Out((KNN_N, k), torch.int32), tied=Out((KNN_N, k), torch.int32))


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("C", [3, 257])
@pytest.mark.parametrize("D", [5, 8])
def test_silhouette(monkeypatch, ops, D, C, metric):
    """The entry itself, with every output and the workspace the caller's own (the wrapper allocates its outputs)."""
    from vit_som_amd._lib import check, lib, ptr, stream
    N = KNN_N
    X, labels = rnd(N, D, seed=1), (torch.arange(N) * 7) % C
    ref = ops.silhouette(X.to(DEV), labels.to(DEV), metric, C)

    def call(**t):
        ld = t["X"].stride(0)
        check(lib.vsom_silhouette(ptr(t["X"]), ld, N, D, metric, ptr(t["labels"]), C, ptr(t["sil"]), ptr(t["a"]), ptr(t["b"]),
                                  ptr(t["nearest"]), ptr(t["counts"]), ptr(t["mean"]), ptr(t["score"]), ptr(t["status"]),
                                  ptr(t["ws"]), t["ws"].numel(), stream()), "vsom_silhouette")

    f64 = torch.float64
    r = contract(monkeypatch, ops, call, expect_scratch=False, X=In(X, PAD), labels=In(labels), sil=Out((N,), f64), a=Out((N,), f64),
                 b=Out((N,), f64), nearest=Out((N,), torch.int64), counts=Out((C,), torch.int64), mean=Out((C,), f64),
                 score=Out((1,), f64), status=Out((4,), torch.int64), ws=Ws(lib.vsom_silhouette_workspace_bytes(N, C)))
    for name, got in (("sil", r["sil"]), ("a", r["a"]), ("b", r["b"]), ("nearest", r["nearest"]), ("counts", r["counts"]),
                      ("cluster_mean", r["mean"]), ("score", r["score"])):
        assert same(getattr(ref, name), got), name
    # the wrapper with a workspace of the caller's own, and with the exact scratch
    own = contract(monkeypatch, ops, lambda **t: {"sil": ops.silhouette(t["X"], t["labels"], metric, C, ws=t["ws"]).sil},
                   expect_scratch=False, X=In(X, PAD), labels=In(labels), ws=Ws(lib.vsom_silhouette_workspace_bytes(N, C)))
    contract(monkeypatch, ops, lambda **t: {"sil": ops.silhouette(t["X"], t["labels"], metric, C).sil}, expect_scratch=True,
             X=In(X, PAD), labels=In(labels))
    del own


@pytest.mark.parametrize("weights", [0, 1, 2])
@pytest.mark.parametrize("C", [3, 257])
@pytest.mark.parametrize("k", [3, 64])
def test_knn_vote(monkeypatch, ops, k, C, weights):
    idx = randint(0, KNN_N, (KNN_NQ, k), seed=1)
    idx[::5, -1] = -1
    dist = torch.rand(KNN_NQ, k, generator=torch.Generator().manual_seed(2)).sort(1).values
    dist[::5, -1] = float("inf")
    labels = randint(0, C, (KNN_N,), seed=3)
    contract(monkeypatch, ops,
             lambda **t: ops.knn_vote(t["idx"], t["dist"], t["labels"], C, weights, 0.07, t["pred"], t["status"], t["scores"]),
             expect_scratch=False, idx=In(idx), dist=In(dist), labels=In(labels), pred=Out((KNN_NQ,), torch.int64),
             status=Acc(torch.zeros(2, dtype=torch.int32)), scores=Out((KNN_NQ, C), torch.float64))
    contract(monkeypatch, ops, lambda **t: ops.knn_vote(t["idx"], t["dist"], t["labels"], C, weights, 0.07, t["pred"], t["status"]),
             idx=In(idx), dist=In(dist), labels=In(labels), pred=Out((KNN_NQ,), torch.int64),
             status=Acc(torch.zeros(2, dtype=torch.int32)))


# ------------------------------------------------------------------ k-means
@pytest.mark.parametrize("D", [5, 8])
def test_kmeans(monkeypatch, ops, D):
    """assign -> update -> relocate share one workspace of the caller's (exactly kmeans_workspace_bytes, guarded)."""
    N, k = 70, 3
    X = rnd(N, D, seed=1)
    centers = X[[3, 30, 60]].clone()
    centers[1] = 100.0                                       # nobody's nearest centre: cluster 1 comes out empty ...
    prev = randint(0, k, (N,), seed=2)
    far = int(torch.cdist(X.double(), centers[[0, 2]].double()).min(1).values.argmax())
    moves = torch.tensor([[1, far]], dtype=torch.int64)      # ... and takes the sample farthest from its centre
    f64 = torch.float64

    def lloyd(**t):
        ops.kmeans_assign(t["X"], t["C"], t["labels"], t["prev"], t["mind"], t["ws"])
        ops.kmeans_update(t["C"], t["cnew"], N, t["mind"], t["counts"], t["status"], t["ws"])
        ops.kmeans_relocate(t["X"], t["labels"], t["moves"], t["C"], t["cnew2"], t["counts"], t["status"], t["ws"])

    r = contract(monkeypatch, ops, lloyd, expect_scratch=False, X=In(X, PAD), C=In(centers), prev=In(prev), moves=In(moves),
                 labels=Out((N,), torch.int64), mind=Out((N,)), cnew=Out((k, D)), counts=Out((k,), torch.int64), status=Out((4,), f64),
                 cnew2=Out((k, D)), ws=Ws(ops.kmeans_workspace_bytes(N, D, k)))
    assert int(r["counts"].sum()) == N and int(r["counts"][1]) == 1
    contract(monkeypatch, ops, lambda **t: ops.kmeans_colvar(t["X"], k, t["out"], t["ws"]), expect_scratch=False,
             X=In(X, PAD), out=Out((1,), f64), ws=Ws(ops.kmeans_workspace_bytes(N, D, k)))
    T = 4
    contract(monkeypatch, ops, lambda **t: ops.kmeanspp_dist(t["X"], t["cand"], t["closest"], t["dist"], t["pots"]), expect_scratch=False,
             X=In(X, PAD), cand=In(torch.tensor([0, 17, 33, 69], dtype=torch.int64)), closest=In(torch.rand(N) * 4),
             dist=Out((T, N)), pots=Out((T,), f64))


# ------------------------------------------------------------------ UMAP
@pytest.mark.parametrize("dim", [2, 3])
def test_umap_epoch(monkeypatch, ops, dim):
    """The case of test_umap_gpu.py::test_epoch_against_restatement, epoch 3 of 30."""
    from test_umap_gpu import knn_table
    from vit_som_amd.umap import find_ab_params, fuzzy_simplicial_set, make_schedule
    rng = np.random.default_rng(dim)
    pts = rng.normal(size=(80, 4))
    idx, dist = knn_table(pts, 8)
    G = fuzzy_simplicial_set(idx, dist, 1.0, 1.0)[0].astype(np.float32)
    P, eps, eps_neg = make_schedule(G, 30, 5)
    a, b = find_ab_params(1.0, 0.1)
    Y = torch.from_numpy(rng.uniform(0.0, 10.0, size=(80, dim)).astype(np.float32))
    t_ = lambda v: torch.from_numpy(np.ascontiguousarray(v))      # noqa: E731
    indptr, indices = t_(P.indptr.astype(np.int64)), t_(P.indices.astype(np.int64))
    contract(monkeypatch, ops,
             lambda **t: ops.umap_epoch(t["indptr"], t["indices"], t["eps"], t["nxt"], t["eps_neg"], t["nxt_neg"], t["Yin"], t["Yout"],
                                        a, b, 1.0, 0.9, 3, 0x1234_5678_9ABC_DEF1),
             expect_scratch=False, indptr=In(indptr), indices=In(indices), eps=In(t_(eps)), eps_neg=In(t_(eps_neg)),
             nxt=Acc(t_(eps)), nxt_neg=Acc(t_(eps_neg)), Yin=In(Y), Yout=Out((80, dim)))


@pytest.mark.parametrize("dim", [2, 3])
def test_umap_transform_layout(monkeypatch, ops, dim):
    """The case of test_umap_transform_gpu.py::test_layout_against_restatement_sliced: epochs [0, 6) of 30, then [6, 9) on
    the state the first slice left in the caller's workspace."""
    from test_umap_transform_gpu import ALPHA, GAMMA, RATE, SEED, _ab, _small
    from vit_som_amd._lib import lib
    idx, w, eps, Yt = (torch.from_numpy(np.ascontiguousarray(v)) for v in _small(dim))
    a, b = _ab()
    M, k = idx.shape
    need = lib.vsom_umap_transform_workspace_bytes(M, k)
    assert need == ops.umap_transform_workspace(M, k, DEV).numel()

    def call(**t):
        for e0, e1 in ((0, 6), (6, 9)):
            ops.umap_transform_layout(t["idx"], t["w"], t["eps"], t["Yt"], t["Y"], a, b, GAMMA, ALPHA, 30, e0, e1, RATE, SEED,
                                      t["status"], t["ws"])
        nxt, nxt_neg = ops.umap_transform_state(t["ws"], M, k)
        return {"next": nxt, "next_neg": nxt_neg}

    contract(monkeypatch, ops, call, expect_scratch=False, idx=In(idx), w=In(w), eps=In(eps), Yt=In(Yt), Y=Out((M, dim)),
             status=Acc(torch.zeros(1, dtype=torch.int32)), ws=Ws(need))


# ------------------------------------------------------------------ small entries (outputs and inputs only)
def test_small_vector_entries(monkeypatch, ops):
    for n in (1000, 1283):
        contract(monkeypatch, ops, lambda **t: ops.fill(t["t"], 2.5), expect_scratch=False, t=Out((n,)))
        a, b, s = rnd(n, seed=1), rnd(n, seed=2), torch.tensor([0.75])
        contract(monkeypatch, ops, lambda **t: ops.scaled_mul(t["out"], t["a"], t["b"], t["s"], 0.5),
                 out=Out((n,)), a=In(a), b=In(b), s=In(s))
        contract(monkeypatch, ops, lambda **t: ops.scaled_mul(t["out"], t["a"]), out=Out((n,)), a=In(a))
        contract(monkeypatch, ops, lambda **t: ops.scale_by(t["t"], t["s"]), t=Acc(a), s=In(s))
    one, two, cnt = torch.tensor([1.5]), torch.tensor([-0.25]), torch.tensor(41, dtype=torch.int64)
    contract(monkeypatch, ops, lambda **t: ops.lincomb2(t["out"], t["a"], 2.0, t["b"], 3.0, t["cnt"]),
             out=Out((1,)), a=In(one), b=In(two), cnt=Acc(cnt.view(1)))
    contract(monkeypatch, ops, lambda **t: ops.loss_parts(t["parts"], t["a"], 0.5, t["b"], 0.3, 0.25, t["cnt"]),
             parts=Out((3,)), a=In(one), b=In(two), cnt=Acc(cnt.view(1)))


def test_adamw_step(monkeypatch, ops):
    n = 256 * 5
    p, gr = rnd(n, seed=1), rnd(n, seed=2)
    wd = torch.tensor([0.05, 0.0, 0.01, 0.05, 0.0])
    contract(monkeypatch, ops, lambda **t: ops.adamw_step(t["p"], t["g"], t["m"], t["v"], t["wd"], 3e-3, 0.9, 0.999, 1e-8, 3, grad_scale=0.5),
             expect_scratch=False, p=Acc(p), g=In(gr), m=Acc(rnd(n, seed=3, scale=0.1)), v=Acc(rnd(n, seed=4).abs() * 0.01), wd=In(wd))


def test_transpose_rows_add_reduce(monkeypatch, ops):
    shapes = [(192, 576), (37, 5), (4, 4), (1, 33)]
    total = sum(r * c for r, c in shapes)
    rows, off = [], 0
    for r, c in shapes:
        rows.append([off, off, r, c]); off += r * c
    contract(monkeypatch, ops, lambda **t: ops.transpose_many(t["src"], t["dst"], t["table"], 192, 576), expect_scratch=False,
             src=In(rnd(total, seed=3)), dst=Out((total,)), table=In(torch.tensor(rows, dtype=torch.int64)))
    for r, c in ((8, 192), (5, 37)):
        contract(monkeypatch, ops, lambda **t: ops.rows_add(t["src"], t["dst"]),
                 src=In(rnd(r, c, seed=1), PAD), dst=Acc(rnd(r, c, seed=2), PAD))
    for ns, n in ((7, 1003), (40, 192), (3, 2)):
        contract(monkeypatch, ops, lambda **t: ops.reduce_slabs(t["slabs"], t["out"]),
                 slabs=In(rnd(ns, n, seed=1), PAD if n > 2 else 0), out=Out((n,)))


def test_evaluation_counters(monkeypatch, ops):
    n, na, nb = 1003, 7, 5
    a, b = randint(0, na, (n,), seed=1), randint(0, nb, (n,), seed=2)
    contract(monkeypatch, ops, lambda **t: ops.contingency(t["a"], t["b"], t["table"], t["bad"]), expect_scratch=False,
             a=In(a), b=In(b), table=Acc(torch.zeros(na, nb, dtype=torch.int64)), bad=Acc(torch.zeros(1, dtype=torch.int32)))
    for rows, cols in ((33, 10), (5, 257)):
        contract(monkeypatch, ops, lambda **t: ops.argmax_rows(t["x"], t["out"]),
                 x=In(rnd(rows, cols, seed=3), PAD), out=Out((rows,), torch.int64))
    K = 12
    bmu, label = randint(0, K, (n,), seed=4), randint(0, 10, (n,), seed=5)
    contract(monkeypatch, ops, lambda **t: ops.last_label(t["bmu"], t["label"], 100, t["cells"], t["bad"]),
             bmu=In(bmu), label=In(label), cells=Acc(torch.zeros(K, dtype=torch.int64)), bad=Acc(torch.zeros(1, dtype=torch.int32)))
    B = 70
    dist = torch.rand(B, K, generator=torch.Generator().manual_seed(6)) + 0.1
    grid = torch.stack([torch.arange(K) // 4, torch.arange(K) % 4], 1).float()
    z = lambda m: Acc(torch.zeros(m, dtype=torch.int64))          # noqa: E731
    contract(monkeypatch, ops,
             lambda **t: ops.map_stats(t["dist"], t["bmu"], t["grid"], 1.0, 0, t["hits"], t["qe"], t["te"], t["nearest"], t["bad"],
                                       second=t["second"]),
             dist=In(dist), bmu=In(dist.argmin(1)), grid=In(grid), hits=z(K), qe=z(K), te=z(1),
             nearest=Acc(torch.full((K,), -1, dtype=torch.int64)), bad=Acc(torch.zeros(1, dtype=torch.int32)),
             second=Out((B,), torch.int64))


@pytest.mark.parametrize("distance", [0, 1, 2])
def test_umatrix(monkeypatch, ops, distance):
    """The entry itself: the wrapper allocates its outputs."""
    from vit_som_amd._lib import check, lib, ptr, stream
    K, L = 15, 37
    W = _protos(K, L)
    grid = torch.stack([torch.arange(K) // 5, torch.arange(K) % 5], 1).float()
    u, nbr_idx, nbr_dist = ops.umatrix(W.to(DEV), grid.to(DEV), 1.0, distance)

    def call(**t):
        check(lib.vsom_umatrix(ptr(t["W"]), K, L, ptr(t["grid"]), 1.0, distance, ptr(t["idx"]), ptr(t["nd"]), ptr(t["u"]),
                               ptr(t["status"]), stream()), "vsom_umatrix")

    r = contract(monkeypatch, ops, call, expect_scratch=False, W=In(W), grid=In(grid), idx=Out((K, 8), torch.int32),
                 nd=Out((K, 8)), u=Out((K,)), status=Acc(torch.zeros(1, dtype=torch.int32)))
    assert same(r["u"], u) and same(r["idx"], nbr_idx) and same(r["nd"], nbr_dist)


def test_proto_mosaic(monkeypatch, ops):
    """The smallest committed case (test_mapviz_gpu.py::test_proto_mosaic_unaligned_pred's shape); the canvas keeps its gaps:
    it starts from the same bytes in every run."""
    C, p, rows, cols = 3, 2, 2, 3
    K, n, S = 6, 9, 6
    pred = torch.rand(K * (n + 1), p * p * C, generator=torch.Generator().manual_seed(5))
    canvas = torch.full((rows * S + rows - 1, cols * S + cols - 1, 3), 7, dtype=torch.uint8)
    contract(monkeypatch, ops, lambda **t: ops.proto_mosaic(t["pred"], n, p, C, 0, (rows, cols), images=t["images"], canvas=t["canvas"], gap=1),
             expect_scratch=False, pred=In(pred), images=Out((K, C, S, S)), canvas=Acc(canvas))
    contract(monkeypatch, ops, lambda **t: ops.proto_mosaic(t["pred"], n, p, C, 3, (rows, cols), images=t["images"]),
             pred=In(pred[:3 * (n + 1)]), images=Acc(torch.zeros(K, C, S, S)))


# ------------------------------------------------------------------ the data pipeline
def test_data_pipeline(monkeypatch, ops):
    """augment_batch, augment_batch_ra and augment_batch_ragged (with its scratch, the caller's) on a 16-image set: the uint8
    source in a guarded arena, both outputs guarded.  The plans come from the device entries, guarded as well."""
    import math

    import data_ref as R
    from test_ragged_gpu import ragged_set
    N, B, C, H, S, seed, epoch = 16, 8, 3, 32, 32, 20240611, 3
    g = torch.Generator().manual_seed(C)
    images = torch.randint(0, 256, (N, C, H, H), dtype=torch.uint8, generator=g)
    index = torch.randint(0, N, (B,), generator=g)
    mean, std = torch.tensor((0.485, 0.456, 0.406)), torch.tensor((0.229, 0.224, 0.225))
    args = (S, (0.08, 1.0), (math.log(0.75), math.log(1.3333)), R.TIMM_SCALE, (math.log(R.TIMM_RATIO[0]), math.log(R.TIMM_RATIO[1])),
            0.5, 0.6, seed, epoch)
    zeros = lambda w: Acc(torch.zeros(B, w, dtype=torch.int32))    # noqa: E731
    plan = contract(monkeypatch, ops, lambda **t: ops.augment_plan(t["index"], t["params"], N, H, *args), expect_scratch=False,
                    index=In(index), params=zeros(ops.AUGMENT_PARAMS))["params"]
    rec = contract(monkeypatch, ops,
                   lambda **t: ops.randaug_plan(t["index"], t["ra"], N, S, 2, True, 0.5, (0, 0, 0), (125, 123, 114), seed, epoch),
                   index=In(index), ra=zeros(ops.RANDAUG_PARAMS))["ra"]
    outs = lambda: dict(out=Out((B, C, S, S)), out8=Out((B, C, S, S), torch.uint8, written=False))    # noqa: E731
    common = dict(src=In(images), index=In(index), mean=In(mean), std=In(std))
    contract(monkeypatch, ops,
             lambda **t: ops.augment_batch(t["src"], t["index"], t["params"], t["out"], S, S, 0, t["mean"], t["std"], seed, epoch, out_u8=t["out8"]),
             expect_scratch=False, params=In(plan), **common, **outs())
    contract(monkeypatch, ops,
             lambda **t: ops.augment_batch(t["src"], t["index"], None, t["out"], S, 36, 2, t["mean"], t["std"], seed, epoch, out_u8=t["out8"]),
             **common, **outs())
    contract(monkeypatch, ops,
             lambda **t: ops.augment_batch_ra(t["src"], t["index"], t["params"], t["ra"], t["out"], S, t["mean"], t["std"], seed, epoch,
                                              out_u8=t["out8"]),
             params=In(plan), ra=In(rec), **common, **outs())
    # images of their own sizes
    sizes = [(20, 28), (32, 32), (40, 25), (33, 47)] * 4
    ds = ragged_set([torch.randint(0, 256, (C, h, w), dtype=torch.uint8, generator=g).numpy() for h, w in sizes])
    rag = dict(data=In(ds.data.cpu()), offsets=In(ds.offsets.cpu()), shapes=In(ds.shapes.cpu()), index=In(index), mean=In(mean), std=In(std))
    rplan = contract(monkeypatch, ops, lambda **t: ops.augment_plan_ragged(t["index"], t["shapes"], t["params"], *args),
                     index=In(index), shapes=In(ds.shapes.cpu()), params=zeros(ops.AUGMENT_PARAMS))["params"]
    contract(monkeypatch, ops,
             lambda **t: ops.augment_batch_ragged(t["data"], t["offsets"], t["shapes"], C, ds.max_h, ds.max_w, t["index"], t["params"], t["out"],
                                                  S, S, t["mean"], t["std"], seed, epoch, scratch=t["scratch"], out_u8=t["out8"]),
             expect_scratch=False, params=In(rplan), scratch=Ws(ops.augment_ragged_scratch_bytes(B, C, S)), **rag, **outs())
    contract(monkeypatch, ops,
             lambda **t: ops.augment_batch_ragged(t["data"], t["offsets"], t["shapes"], C, ds.max_h, ds.max_w, t["index"], None, t["out"],
                                                  S, 36, t["mean"], t["std"], seed, epoch, out_u8=t["out8"]),
             **rag, **outs())


# ------------------------------------------------------------------ one training run, end to end
def test_two_training_steps_with_exact_workspaces(monkeypatch, ops):
    """The tiny ViTSOM of the goldens, two training steps with the launch tape off (every call asks for its workspace
    afresh): plainly, and with every workspace exact, guarded and full of NaN -- on the main and the side streams, in the
    real call order, consecutive kernels reusing one workspace.  Loss, parameters and gradients bit for bit."""
    import vit_som_amd
    from helpers import golden_params, load_golden
    from vit_som_amd.tuning import hooks
    z, cfg = load_golden("ref_cluster_tiny")
    x, y = torch.from_numpy(z["x"]).to(DEV), torch.from_numpy(z["y"]).to(DEV)

    def run():
        m = vit_som_amd.ViTSOM(copy.deepcopy(cfg), device=DEV)
        m.load_state_dict(golden_params(z))
        m.set_schedule(60, 40)
        (opt,), _ = m.configure_optimizers()
        losses = []
        for _ in range(2):
            out = m.train_step_fused(x, y)
            if isinstance(out, torch.Tensor):
                losses.append(out.detach().clone().reshape(-1))
            opt.step()
        torch.cuda.synchronize()
        return m.arena.params.clone(), m.arena.grads.clone(), losses

    hooks.set(launch_tape=False)
    try:
        p0, g0, l0 = run()
        es = MC.ExactScratch(MC.FILL_FF)
        with monkeypatch.context() as mp:
            mp.setattr(ops, "scratch", es)
            p1, g1, l1 = run()
    finally:
        hooks.reset()
    torch.cuda.synchronize()
    assert es.calls > 10 and len(es.arenas) > 1
    es.check()
    assert same(p0, p1), "parameters differ"
    assert same(g0, g1), "gradients differ"
    assert len(l0) == len(l1) and all(same(a, b) for a, b in zip(l0, l1))
    assert bool(torch.isfinite(p1).all()) and bool(torch.isfinite(g1).all())
