"""Attention rollout without a GPU: the reference restatement checks itself, the two C entries agree between header,
ctypes table and library and refuse bad calls before any launch, and every Python refusal says what it wants."""
import ctypes
import os
import re

import pytest
import torch

import attention_rollout_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("vsom_attention_rollout_ws_size", "vsom_attention_rollout_step")
EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -3, -4


def _qkv(B, N, H, hd, seed=0, scale=1.0):
    return torch.randn(B * N, 3 * H * hd, generator=torch.Generator().manual_seed(seed)) * scale


# ---------------------------------------------------------------- the reference checks itself
@pytest.mark.parametrize("fusion", R.FUSIONS)
@pytest.mark.parametrize("alpha", [0.5, 1.0])
def test_reference_rows_sum_to_one(fusion, alpha):
    B, N, H, hd = 2, 9, 3, 4
    A = R.mixed(R.probabilities(_qkv(B, N, H, hd), B, N, H, hd, torch.float64), fusion, alpha)
    assert float((A.sum(-1) - 1).abs().max()) < 1e-14
    assert bool((A >= 0).all())
    w = R.query("random", B, N, seed=3).double()
    out = R.step(_qkv(B, N, H, hd), w, B, N, H, hd, fusion, alpha, torch.float64)
    assert float((out.sum(1) - w.sum(1)).abs().max()) < 1e-13


def test_reference_two_blocks_are_the_matrix_product():
    B, N, H, hd = 2, 7, 2, 4
    q1, q2 = _qkv(B, N, H, hd, 1), _qkv(B, N, H, hd, 2)          # q1 the first block, q2 the last
    A1 = R.mixed(R.probabilities(q1, B, N, H, hd, torch.float64), "mean", 0.5)
    A2 = R.mixed(R.probabilities(q2, B, N, H, hd, torch.float64), "mean", 0.5)
    w = R.query("random", B, N, seed=5).double()
    want = torch.einsum("bi,bij->bj", w, A2 @ A1)
    got = R.rollout([q1, q2], w, B, N, H, hd, "mean", 0.5, torch.float64)
    assert float((got - want).abs().max()) < 1e-15
    assert float((got - R.rollout([q2, q1], w, B, N, H, hd, "mean", 0.5, torch.float64)).abs().max()) > 1e-4     # the order matters


def test_reference_alpha_one_is_the_head_mean_probability_row():
    B, N, H, hd = 2, 6, 3, 4
    qkv = _qkv(B, N, H, hd, 7)
    P = R.probabilities(qkv, B, N, H, hd, torch.float64)
    got = R.rollout([qkv], R.query("cls", B, N), B, N, H, hd, "mean", 1.0, torch.float64)
    assert float((got - P.mean(1)[:, 0]).abs().max()) < 1e-15


def test_reference_fusions_agree_with_one_head():
    B, N, H, hd = 2, 6, 1, 8
    qkv, w = _qkv(B, N, H, hd, 9), R.query("random", B, N, seed=1)
    mean = R.step(qkv, w, B, N, H, hd, "mean", 0.5, torch.float64)
    for fusion in ("max", "min"):
        assert torch.equal(R.step(qkv, w, B, N, H, hd, fusion, 0.5, torch.float64), mean)


def test_reference_max_and_min_need_the_renormalisation():
    B, N, H, hd = 1, 6, 3, 4
    P = R.probabilities(_qkv(B, N, H, hd, 11), B, N, H, hd, torch.float64)
    assert float(R.fuse(P, "max").sum(-1).min()) > 1.0 + 1e-3 and float(R.fuse(P, "min").sum(-1).max()) < 1.0 - 1e-3


def test_row_scaled_error_measures_each_row_against_its_own_peak():
    ref = torch.tensor([[1.0, 0.5], [1e-3, 5e-4]], dtype=torch.float64)
    got = ref + torch.tensor([[1e-6, 0.0], [0.0, 1e-6]], dtype=torch.float64)
    assert abs(R.row_scaled_error(got, ref) - 1e-3) < 1e-12
    assert R.bound(1e-9) == R.FLOOR == 3e-6 and R.bound(1e-5) == pytest.approx(4e-5, rel=1e-12)


# ---------------------------------------------------------------- the C boundary
def _header():
    src = open(os.path.join(ROOT, "include", "vitsom_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_header_signatures_and_symbols_agree():
    import vit_som_amd  # noqa: F401
    from vit_som_amd._lib import LIB_PATH, SIGNATURES
    src = _header()
    raw = ctypes.CDLL(LIB_PATH)
    for name in ENTRIES:
        assert re.search(r"\b" + name + r"\s*\(", src), f"{name} is not declared in include/vitsom_hip.h"
        assert name in SIGNATURES and hasattr(raw, name)
    m = re.search(r"long\s+vsom_attention_rollout_ws_size\s*\(([^)]*)\)", src)
    assert [a.split()[0] for a in m.group(1).split(",")] == ["int"] * 4
    assert SIGNATURES["vsom_attention_rollout_ws_size"] == (ctypes.c_long, [ctypes.c_int] * 4)
    m = re.search(r"int\s+vsom_attention_rollout_step\s*\(([^)]*)\)", src, flags=re.S)
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["const float* qkv", "const float* v_in", "float* v_out", "int B", "int N", "int H", "int hd", "int fusion",
                    "float alpha", "void* ws", "long ws_size", "vsom_stream_t stream"]
    res, argtypes = SIGNATURES["vsom_attention_rollout_step"]
    assert res is ctypes.c_int and len(argtypes) == len(args)
    assert argtypes[3:9] == [ctypes.c_int] * 5 + [ctypes.c_float] and argtypes[10] is ctypes.c_long


def test_workspace_size_is_zero_outside_the_limits():
    from vit_som_amd._lib import lib
    size = lib.vsom_attention_rollout_ws_size
    assert size(1, 4096, 1, 64) == 0                                  # N past five chunks of keys, and past the LDS
    assert size(1, 321, 1, 8) == 0 and size(1, 320, 1, 8) > 0
    assert size(1, 257, 1, 200) == 0                                  # 257 x 201 floats of K do not fit 160 KiB
    for bad in [(0, 5, 1, 8), (1, 0, 1, 8), (1, 5, 0, 8), (1, 5, 1, 0), (-1, 5, 1, 8)]:
        assert size(*bad) == 0, bad
    # every project shape (SURVEY.md section 8, c1 .. c5) and the tests' own: B ceil(N / 16) rows of N floats
    for B, N, H, hd in [(512, 197, 3, 64), (512, 65, 3, 64), (256, 257, 3, 64), (3, 5, 2, 8), (2, 1, 2, 64), (2, 64, 1, 16)]:
        assert size(B, N, H, hd) == B * -(-N // 16) * N * 4
    assert size(64, 257, 3, 64) < 64 * 3 * 257 * 257 * 4 // 8         # far below one block's probability tensor


def test_every_refusal_comes_before_a_launch():
    """Small integers as pointers (test_abi.py): a launch would fault, a refusal returns its code."""
    from vit_som_amd._lib import last_error, lib
    step = lib.vsom_attention_rollout_step
    ok = dict(qkv=1 << 28, v_in=1 << 20, v_out=1 << 24, B=2, N=5, H=2, hd=8, fusion=0, alpha=0.5, ws=1 << 30, ws_size=1 << 20)

    def call(**kw):
        a = dict(ok, **kw)
        return step(a["qkv"], a["v_in"], a["v_out"], a["B"], a["N"], a["H"], a["hd"], a["fusion"], a["alpha"], a["ws"], a["ws_size"], None)

    for name in ("qkv", "v_in", "v_out"):
        assert call(**{name: None}) == EINVAL and "null" in last_error(), name
    for name in ("B", "N", "H", "hd"):
        for v in (0, -3):
            assert call(**{name: v}) == EINVAL and "bad shape" in last_error(), (name, v)
    for fusion in (-1, 3):
        assert call(fusion=fusion) == EINVAL and "fusion" in last_error()
    for alpha in (0.0, -0.5, 1.5, float("nan"), float("inf")):
        assert call(alpha=alpha) == EINVAL and "alpha" in last_error(), alpha
    assert call(v_out=1 << 20) == EINVAL and "overlaps" in last_error()
    assert call(v_out=(1 << 20) + 2 * 5 * 4 - 4) == EINVAL and "overlaps" in last_error()     # the last float of v_in
    assert call(v_out=(1 << 20) - 2 * 5 * 4 + 4) == EINVAL and "overlaps" in last_error()     # its first, from below
    assert call(N=4096, hd=64) == EUNSUPPORTED
    msg = last_error()
    assert "N=4096" in msg and "hd=64" in msg and str((4096 * 65 + 16 * 64 + 4 * 64 * 64) * 4) in msg
    assert call(N=257, hd=200) == EUNSUPPORTED and "N=257" in last_error() and "hd=200" in last_error()
    need = lib.vsom_attention_rollout_ws_size(2, 5, 2, 8)
    assert call(ws=None) == EWORKSPACE and "workspace" in last_error()
    assert call(ws_size=need - 1) == EWORKSPACE and str(need) in last_error()
    assert call(ws_size=0) == EWORKSPACE


# ---------------------------------------------------------------- the Python refusals
def test_check_arguments_names_the_argument_and_its_values():
    from vit_som_amd.attention_rollout import check_arguments
    assert check_arguments("f", "mean", 0.5, 0, 2) == 0.5 and check_arguments("f", "min", 0, 1, 2) == 1.0
    with pytest.raises(ValueError, match=r"f: head_fusion must be one of 'mean', 'max', 'min', got 'sum'"):
        check_arguments("f", "sum", 0.5, 0, 2)
    for bad in (1.0, -0.1, 2, "0.5", None, True, float("nan")):
        with pytest.raises(ValueError, match=r"f: residual must be a number in \[0, 1\)"):
            check_arguments("f", "mean", bad, 0, 2)
    for bad in (-1, 2, 1.0, None, True, "0"):
        with pytest.raises(ValueError, match=r"f: start_layer must be an int in \[0, 2\)"):
            check_arguments("f", "mean", 0.5, bad, 2)


def test_query_weights_and_their_refusals():
    from vit_som_amd.attention_rollout import query_weights
    cpu = torch.device("cpu")
    assert torch.equal(query_weights("cls", 2, 5, cpu), R.query("cls", 2, 5))
    assert torch.equal(query_weights("patches", 2, 5, cpu), R.query("patches", 2, 5))
    assert torch.equal(query_weights(3, 2, 5, cpu), torch.eye(5)[3].expand(2, 5))
    t = torch.rand(5)
    assert torch.equal(query_weights(t, 2, 5, cpu), t.expand(2, 5)) and query_weights(t, 2, 5, cpu).is_contiguous()
    t2 = torch.rand(2, 5, dtype=torch.float64)
    assert torch.equal(query_weights(t2, 2, 5, cpu), t2.float())
    sentence = r"f: query must be 'cls', 'patches', a token index in \[0, 5\) or a non-negative float tensor of shape \[5\] or \[B, 5\]"
    for bad in ("CLS", "mean", 5, -1, 2.0, None, True, torch.rand(4), torch.rand(3, 5), torch.rand(2, 5, 1), torch.ones(5, dtype=torch.int64)):
        with pytest.raises(ValueError, match=sentence):
            query_weights(bad, 2, 5, cpu, "f")
    with pytest.raises(ValueError, match="f: query must be non-negative"):
        query_weights(torch.tensor([0.5, -1e-9, 0, 0, 0]), 2, 5, cpu, "f")
    with pytest.raises(ValueError, match="f: query must be non-negative"):
        query_weights(torch.tensor([0.5, float("nan"), 0, 0, 0]), 2, 5, cpu, "f")
    with pytest.raises(ValueError, match=r"f: query must be 'cls', 'patches', a token index in \[0, 1\) .* got 'patches'"):
        query_weights("patches", 2, 1, cpu, "f")                      # a single token has no patches


def test_desom_and_unknown_models_are_refused_with_the_reason():
    import vit_som_amd
    from vit_som_amd import attention_rollout as AR
    cfg = {"hyperparameters": {"model_arch": "desom"}, "data": {}}
    for entry in (AR.evaluate_attention, AR.visualize_attention_rollout, AR.visualize_attention_map):
        with pytest.raises(ValueError, match=entry.__name__ + ": a DESOM model has no attention layers"):
            entry(object(), cfg, [])
    with pytest.raises(ValueError, match="a DESOM model has no attention layers"):
        vit_som_amd.DESOM.attention_rollout(None, None)
    with pytest.raises(ValueError, match=r"evaluate_attention: needs a vit_som or a vit model; got object with model_arch 'mlp'"):
        AR.evaluate_attention(object(), {"hyperparameters": {"model_arch": "mlp"}, "data": {}}, [])
    with pytest.raises(ValueError, match="needs a vit_som or a vit model"):
        AR.evaluate_attention(object(), {"hyperparameters": {"model_arch": "vit_som"}, "data": {}}, [])


def test_evaluate_attention_refuses_more_than_one_rank_and_bad_arguments():
    from vit_som_amd import attention_rollout as AR

    class Fake:                                                         # what the refusals look at before any batch
        world_size, rank = 2, 0
        _vit = type("V", (), {"blocks": [0, 1], "img_size": 8, "patch_embed": type("P", (), {"patch_size": (4, 4)})()})()
    cfg = {"hyperparameters": {"model_arch": "vit"}, "data": {"num_channels": 1, "input_size": 8, "num_classes": 3}}
    with pytest.raises(ValueError, match="evaluate_attention: model.world_size > 1 is not supported; run it on one rank"):
        AR.evaluate_attention(Fake(), cfg, [])
    Fake.world_size = 1
    with pytest.raises(ValueError, match="evaluate_attention: head_fusion must be one of"):
        AR.evaluate_attention(Fake(), cfg, [], head_fusion="median")
    with pytest.raises(ValueError, match=r"evaluate_attention: start_layer must be an int in \[0, 2\)"):
        AR.evaluate_attention(Fake(), cfg, [], start_layer=2)
    with pytest.raises(ValueError, match=r"visualize_attention_rollout: residual must be a number in \[0, 1\)"):
        AR.visualize_attention_rollout(Fake(), cfg, [], residual=1.0)
    with pytest.raises(ValueError, match="visualize_attention_rollout: n_images must be an int >= 1"):
        AR.visualize_attention_rollout(Fake(), cfg, [], n_images=0)


def test_model_methods_refuse_before_touching_the_device():
    import vit_som_amd
    vit = vit_som_amd.ViTAutoencoder(img_size=8, patch_size=4, in_chans=1, embed_dim=16, depth=2, num_heads=2, decoder_embed_dim=16,
                                     decoder_depth=1, decoder_num_heads=2, mlp_ratio=2.0)
    x = torch.zeros(2, 1, 8, 8)
    with pytest.raises(ValueError, match="attention_rollout: head_fusion must be one of"):
        vit.attention_rollout(x, head_fusion="sum")
    with pytest.raises(ValueError, match=r"attention_rollout: residual must be a number in \[0, 1\)"):
        vit.attention_rollout(x, residual=1.0)
    with pytest.raises(ValueError, match=r"attention_rollout: start_layer must be an int in \[0, 2\)"):
        vit.attention_rollout(x, start_layer=2)
    with pytest.raises(ValueError, match="attention_rollout: input must live on the MI355X"):
        vit.attention_rollout(x)
    with pytest.raises(ValueError, match=r"patch_map: expected a rollout of shape \[B, 5\]"):
        vit.patch_map(torch.zeros(2, 4))
    assert vit.patch_map(torch.arange(10.0).view(2, 5)).shape == (2, 2, 2)


def test_ops_wrappers_validate_with_value_errors():
    from vit_som_amd import ops
    t = torch.zeros(10, 48)
    with pytest.raises(ValueError, match="qkv: expected a HIP device tensor"):
        ops.attention_rollout_step(t, torch.zeros(2, 5), torch.zeros(2, 5), 2, 5, 2, 8, "mean", 0.5)
    with pytest.raises(ValueError, match="qkvs: expected at least one"):
        ops.attention_rollout([], torch.zeros(2, 5), 2, 8)
    assert ops.ROLLOUT_FUSIONS == {"mean": 0, "max": 1, "min": 2}
    assert ops.attention_rollout_ws_size(1, 4096, 1, 64) == 0 and ops.attention_rollout_ws_size(2, 5, 2, 8) == 2 * 5 * 4


def test_the_package_exports_the_entries_from_their_own_module():
    import vit_som_amd
    from vit_som_amd import attention_rollout as AR, evaluation
    for name in ("AttentionReport", "evaluate_attention", "visualize_attention_rollout", "visualize_attention_map"):
        assert getattr(vit_som_amd, name) is getattr(AR, name) is getattr(evaluation, name)
        assert getattr(AR, name).__module__ == "vit_som_amd.attention_rollout"
    import dataclasses
    fields = [f.name for f in dataclasses.fields(AR.AttentionReport)]
    assert fields[:13] == ["mean_map", "class_maps", "class_counts", "unit_maps", "unit_counts", "cls_mass", "entropy", "query",
                           "head_fusion", "residual", "start_layer", "n_samples", "inference_time"]
