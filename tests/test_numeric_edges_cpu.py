"""The edge cases of tests/numeric_edges.py themselves, without a GPU: every reference and yardstick is finite, every
yardstick error e32 is at most 1e-3 (the bound max(FLOOR, 4 e32) would be vacuous otherwise), the property that names a
case holds in its fp64 reference -- and the comparison the GPU tests make rejects the defect each of them is named
after, shown by feeding it a deliberately wrong torch evaluation."""
import pytest
import torch

import numeric_edges as NE
from helpers import rel_err
from test_ops_gpu import GEMM_TOL

ATTN_IDS = NE.attention_ids()
Q1_IDS = NE.attention_ids(NE.Q1_SHAPES)
LN_IDS = [(s, k) for s in NE.LN_SHAPES for k in NE.LN_KINDS]
LN_FUSED_IDS = [(i, k) for i in range(len(NE.LN_FUSED_ROWS)) for k in NE.LN_KINDS]
CE_IDS = [(C, s, k) for C in NE.CE_CLASSES for s in NE.CE_SMOOTHING for k in NE.CE_KINDS]
SOM_IDS = [(i, k, T) for i in range(len(NE.SOM_SHAPES)) for k in NE.SOM_KINDS for T in NE.SOM_T]


def name(v):
    return "-".join(str(e) for e in v) if isinstance(v, tuple) else str(v)


def check_case(c):
    assert NE.finite(c.ref), c.name
    assert NE.finite(c.y32), c.name
    for out, e in c.e32.items():
        assert e <= NE.E32_MAX, (c.name, out, e)
    assert c.prop and all(c.prop.values()), (c.name, c.prop)


@pytest.mark.parametrize("shape,kind", ATTN_IDS, ids=name)
def test_attention_case(shape, kind):
    check_case(NE.attention_case(shape, kind))


@pytest.mark.parametrize("shape,kind", Q1_IDS, ids=name)
def test_q1_case(shape, kind):
    check_case(NE.q1_case(shape, kind))


@pytest.mark.parametrize("shape,kind", LN_IDS, ids=name)
def test_layernorm_case(shape, kind):
    check_case(NE.layernorm_case(shape, kind))


@pytest.mark.parametrize("i,kind", LN_FUSED_IDS, ids=name)
def test_ln_fused_case(i, kind):
    check_case(NE.ln_fused_case(i, kind))


@pytest.mark.parametrize("shape", [(70, 64, 4), (64, 16, 8)], ids=name)
def test_gelu_case(shape):
    check_case(NE.gelu_case(*shape))


@pytest.mark.parametrize("C,smoothing,kind", CE_IDS, ids=name)
def test_cross_entropy_case(C, smoothing, kind):
    check_case(NE.ce_case(C, smoothing, kind))


def test_l1_cases():
    for n in NE.L1_SIZES:
        check_case(NE.l1_case(n))
    for shape in NE.L1_UNPATCHIFY_SHAPES:
        check_case(NE.l1_unpatchify_case(shape))


@pytest.mark.parametrize("i,kind,T", SOM_IDS, ids=name)
def test_som_case(i, kind, T):
    check_case(NE.som_case(i, kind, T))


def test_adamw_cases():
    for step in NE.ADAMW_STEPS:
        check_case(NE.adamw_case(step))


def test_case_lists_are_the_issue_s():
    """Five inputs per attention shape, three at hd = 8; every LayerNorm shape in five kinds; both fused rows."""
    assert len(ATTN_IDS) == 7 * 5 + 3 and len(Q1_IDS) == 4 * 5 + 2 * 3
    assert len(LN_IDS) == 35 and [r.shape for r in NE.LN_FUSED_ROWS] == [(2048, 64, 192), (4096, 64, 96)]
    assert len(CE_IDS) == 40 and len(SOM_IDS) == 30


# ------------------------------------------------------------------------------------ the bound rejects the named defects
def rejected(c, wrong, floors):
    """The outputs of `wrong` that the GPU test's comparison refuses."""
    return [k for k, floor in floors.items() if not NE.accepts(c.metric[k](wrong[k], c.ref[k]), floor, c.e32[k])]


def unshifted_must_fail(c, kind):
    """exp(s) overflows above 88.7 and is flushed below -103: certain on the offset inputs, and on a saturated input
    wherever a score got that far."""
    s = c.ref["scores"]
    return kind.startswith("offset") or float(s.max()) > 89 or float(s.max(-1).values.min()) < -104


@pytest.mark.parametrize("shape,kind", [i for i in ATTN_IDS if i[0][1] > 1], ids=name)
def test_softmax_without_the_max_shift_is_rejected(shape, kind):
    """exp(s) / sum exp(s) on the edge inputs: overflow (scores above 88) or a flushed denominator (below -88)."""
    c = NE.attention_case(shape, kind)
    floors = {"out": 3e-6, "probs": 3e-6, "dqkv": 5e-6}
    right = NE.attention_eval(c.inp["qkv"], c.inp["dout"], *shape, torch.float32)
    assert rejected(c, right, floors) == []
    if unshifted_must_fail(c, kind):
        wrong = NE.attention_eval(c.inp["qkv"], c.inp["dout"], *shape, torch.float32, shift=False)
        assert set(rejected(c, wrong, floors)) == set(floors), c.name


@pytest.mark.parametrize("shape,kind", [i for i in Q1_IDS if i[1].startswith("offset")], ids=name)
def test_q1_softmax_without_the_max_shift_is_rejected(shape, kind):
    c = NE.q1_case(shape, kind)
    wrong = NE.q1_eval(c.inp["q"], c.inp["kv"], c.inp["dout"], *shape, torch.float32, shift=False)
    assert set(rejected(c, wrong, {"out": 1e-5, "dq": 1e-5, "dkv": 1e-5})) == {"out", "dq", "dkv"}, c.name


@pytest.mark.parametrize("shape", NE.LN_SHAPES, ids=name)
@pytest.mark.parametrize("kind", ["offset", "mixed"])
def test_one_pass_variance_is_rejected(shape, kind):
    """E[x^2] - E[x]^2 at a mean of 1000: the variance of 4 is the difference of two numbers near 1e6.  (In the mixed
    launch the outlier rows carry most of dx's norm, so there the forward output is what gives it away.)"""
    c = NE.layernorm_case(shape, kind)
    i = c.inp
    wrong = NE.layernorm_eval(i["x"], i["gamma"], i["beta"], i["dy"], i["resid"], torch.float32, one_pass=True)
    assert ({"y", "dx"} if kind == "offset" else {"y"}) <= set(rejected(c, wrong, {"y": 3e-6, "dx": 5e-6, "dgamma": 5e-6})), c.name
    right = NE.layernorm_eval(i["x"], i["gamma"], i["beta"], i["dy"], i["resid"], torch.float32)
    assert rejected(c, right, {"y": 3e-6, "dx": 5e-6, "dgamma": 5e-6, "dbeta": 5e-6}) == []


@pytest.mark.parametrize("T", NE.SOM_T)
def test_sign_of_zero_equal_to_one_is_rejected(T):
    c = NE.som_case(0, "manhattan_grid", T)
    right = NE.manhattan_grads(c.inp["x"], c.inp["W"], c.ref["h"])
    wrong = NE.manhattan_grads(c.inp["x"], c.inp["W"], c.ref["h"], sign0=1.0)
    assert rejected(c, right, {"gW": 5e-6, "gX": 5e-6}) == []                  # the written-out gradient is the autograd one
    assert set(rejected(c, wrong, {"gW": 5e-6, "gX": 5e-6})) == {"gW", "gX"}


@pytest.mark.parametrize("i", range(len(NE.SOM_SHAPES)))
def test_a_norm_without_the_eps_clamp_is_rejected(i):
    """x / |x| on the all-zero row and prototype: 0 / 0."""
    c = NE.som_case(i, "cos_zero", NE.SOM_T[0])
    wrong = NE.som_eval(c.inp["x"], c.inp["W"], c.inp["grid"], c.T, "cosine", torch.float32, bmu=c.ref["bmu"], clamp=False)
    assert set(rejected(c, wrong, {"dist": 2e-6, "gW": 2e-5, "gX": 2e-5})) == {"dist", "gW", "gX"}
    assert not NE.finite({"d": wrong["dist"]})


def test_the_bound_itself():
    assert NE.accepts(3e-6, 3e-6, 0.0) and not NE.accepts(3.1e-6, 3e-6, 0.0)
    assert NE.accepts(4e-5, 3e-6, 1e-5) and not NE.accepts(4.1e-5, 3e-6, 1e-5)
    assert not NE.accepts(float("nan"), 3e-6, 1e-5)
    assert NE.bound(GEMM_TOL, 0.0) == GEMM_TOL and rel_err(torch.ones(3), torch.ones(3)) == 0.0
