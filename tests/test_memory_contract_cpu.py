"""The memory contract without a GPU: (a) the guard-band harness of memcheck.py catches what it is meant to catch, shown on
CPU tensors; (b) every C-ABI entry that takes a caller-supplied workspace refuses one that is a byte short of its
*_workspace_bytes() query -- on the host, with VSOM_EWORKSPACE and a message that names the buffer, before any launch."""
import os
import re

import pytest
import torch

import memcheck as MC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ (a) the harness tests itself
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.int32, torch.int64, torch.uint8])
def test_guarded_layout_poison_and_alignment(dtype):
    v, h = MC.guarded((5, 7), dtype, "cpu")
    assert v.shape == (5, 7) and v.dtype == dtype and v.is_contiguous() and v.data_ptr() % 256 == 0
    assert h.front == 64 << 10 and h.back == 1 << 20 and h.off >= h.front
    assert h.arena.numel() >= h.off + h.nbytes + h.back
    if dtype.is_floating_point:
        assert bool(torch.isnan(v).all())
    elif dtype != torch.uint8:
        assert bool((v < 0).all())
    h.check()
    with pytest.raises(AssertionError, match="never written"):
        h.all_written()
    v.zero_()
    h.all_written()
    h.check()
    # what surrounds the payload reads as NaN (float) or a negative number (signed integers)
    before = h.arena[h.off - 8:h.off].view(dtype if dtype != torch.uint8 else torch.int32)
    end = (h.off + h.nbytes + 7) // 8 * 8
    after = h.arena[end + 24:end + 32].view(torch.float32)
    assert bool(torch.isnan(after).all())
    assert bool(torch.isnan(before).all()) if dtype.is_floating_point else bool((before < 0).all())


def test_back_guard_grows_with_the_payload():
    v, h = MC.guarded((600, 512), torch.float32, "cpu")
    assert h.nbytes == 600 * 512 * 4 and h.back == h.nbytes > 1 << 20
    h.check()


def test_one_byte_past_the_payload_is_caught():
    v, h = MC.guarded((3, 4), torch.float32, "cpu")
    v.zero_()
    h.arena[h.off + h.nbytes] ^= 1                   # one byte, one element past the end
    with pytest.raises(AssertionError, match=r"byte offset 48 from the payload start \(the back guard"):
        h.check()
    h.arena[h.off + h.nbytes] ^= 1
    h.check()
    h.arena[-1 - 256] ^= 0x80                        # the far end of the back guard
    with pytest.raises(AssertionError, match="back guard"):
        h.check()


def test_one_byte_in_the_front_guard_is_caught():
    v, h = MC.guarded((10,), torch.int64, "cpu")
    h.arena[h.off - 1] ^= 1
    with pytest.raises(AssertionError, match=r"byte offset -1 from the payload start \(the front guard"):
        h.check()
    h.arena[h.off - 1] ^= 1
    h.arena[0] ^= 1                                  # the arena's very first byte
    with pytest.raises(AssertionError, match="front guard"):
        h.check()


def test_one_padding_column_is_caught():
    v, h = MC.guarded((4, 6), torch.float32, "cpu", ld=14)
    assert v.shape == (4, 6) and v.stride() == (14, 1) and v.data_ptr() % 256 == 0
    assert h.nbytes == (3 * 14 + 6) * 4
    v.copy_(torch.arange(24.0).view(4, 6))
    h.check(); h.all_written()
    flat = h.arena[h.off:h.off + h.nbytes].view(torch.float32)
    assert bool(torch.isnan(flat[6:14]).all())        # the padding reads as NaN
    flat[14 + 6] = 1.0                               # the first padding element of the second row
    with pytest.raises(AssertionError, match=r"byte offset 80 from the payload start \(a padding column"):
        h.check()


def test_one_unwritten_element_is_caught():
    for dtype in (torch.float32, torch.float64, torch.int32, torch.int64):
        v, h = MC.guarded((4, 6), dtype, "cpu", ld=8)
        v.zero_()
        h.all_written()
        keep, _ = MC.guarded((1,), dtype, "cpu")
        v[2, 5] = keep[0]                            # the poison itself
        with pytest.raises(AssertionError, match=r"1 of 24 elements were never written, the first at flat index 17"):
            h.all_written()
    v, h = MC.guarded((9,), torch.float32, "cpu")
    v[:8] = float("nan")                             # a NaN a kernel computed is not the poison
    with pytest.raises(AssertionError, match="flat index 8"):
        h.all_written()


def test_guarded_copy_keeps_the_values():
    t = torch.arange(35, dtype=torch.float32).view(5, 7)
    v, h = MC.guarded_copy(t, ld=15)
    assert torch.equal(v, t) and v.stride() == (15, 1)
    h.check(); h.all_written()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.int32, torch.int64, torch.uint8])
@pytest.mark.parametrize("shift", [1, 2, 3])
def test_a_shifted_payload_starts_off_the_boundary_and_keeps_its_guards(dtype, shift):
    size = torch.empty(0, dtype=dtype).element_size()
    v, h = MC.guarded((5, 7), dtype, "cpu", shift=shift)
    assert v.shape == (5, 7) and v.is_contiguous() and v.data_ptr() % 256 == shift * size and h.shift == shift
    assert (v.data_ptr() % 16 != 0) == (shift * size % 16 != 0)
    assert h.off >= h.front + shift * size and h.arena.numel() >= h.off + h.nbytes + h.back
    h.check()
    with pytest.raises(AssertionError, match="never written"):
        h.all_written()
    v.zero_()
    h.all_written(); h.check()
    # the elements between the boundary and the payload are guard: the byte just before the payload, and the boundary itself
    for back_by in (1, shift * size):
        h.arena[h.off - back_by] ^= 1
        with pytest.raises(AssertionError, match=rf"byte offset -{back_by} from the payload start \(the front guard"):
            h.check()
        h.arena[h.off - back_by] ^= 1
    h.arena[h.off + h.nbytes] ^= 1                   # and the first byte past the shifted payload
    with pytest.raises(AssertionError, match=rf"byte offset {35 * size} from the payload start \(the back guard"):
        h.check()
    h.arena[h.off + h.nbytes] ^= 1
    h.check()
    if dtype.is_floating_point:                      # what surrounds the payload still reads as NaN
        assert bool(torch.isnan(h.arena[h.off - size:h.off].view(dtype)).all())


@pytest.mark.parametrize("shift", [1, 2])
def test_a_shifted_payload_with_a_row_pitch(shift):
    v, h = MC.guarded((4, 6), torch.float32, "cpu", ld=9, shift=shift)
    assert v.shape == (4, 6) and v.stride() == (9, 1) and v.data_ptr() % 256 == 4 * shift and h.nbytes == (3 * 9 + 6) * 4
    v.copy_(torch.arange(24.0).view(4, 6))
    h.check(); h.all_written()
    flat = h.arena[h.off:h.off + h.nbytes].view(torch.float32)
    assert bool(torch.isnan(flat[6:9]).all()) and float(flat[9]) == 6.0
    flat[9 + 6] = 1.0                                # the first padding element of the second row
    with pytest.raises(AssertionError, match=r"byte offset 60 from the payload start \(a padding column"):
        h.check()
    v, h = MC.guarded((4, 6), torch.float32, "cpu", ld=9, shift=shift)
    v.zero_()
    keep, _ = MC.guarded((1,), torch.float32, "cpu")
    v[3, 5] = keep[0]
    with pytest.raises(AssertionError, match=r"1 of 24 elements were never written, the first at flat index 23"):
        h.all_written()
    t = torch.arange(35, dtype=torch.float32).view(5, 7)
    c, hc = MC.guarded_copy(t, ld=10, shift=shift)
    assert torch.equal(c, t) and c.stride() == (10, 1) and c.data_ptr() % 16 == 4 * shift
    hc.check(); hc.all_written()


def test_the_default_shift_is_none():
    v, h = MC.guarded((3, 4), torch.float32, "cpu")
    assert h.shift == 0 and v.data_ptr() % 256 == 0


@pytest.mark.parametrize("fill", MC.FILLS)
def test_exact_scratch_size_alignment_and_fill(fill):
    es = MC.ExactScratch(fill)
    for n in (1, 4, 37, 4096, 100003, (1 << 20) + 12):
        ws = es(n, "cpu")
        assert ws.dtype == torch.uint8 and ws.numel() == n and ws.is_contiguous() and ws.data_ptr() % 256 == 0
        if fill == MC.FILL_FF:
            assert bool((ws == 0xFF).all())
            if n >= 4:
                assert bool(torch.isnan(ws[:n // 4 * 4].view(torch.float32)).all())
                assert bool((ws[:n // 4 * 4].view(torch.int32) == -1).all())
        elif fill == MC.FILL_00:
            assert bool((ws == 0).all())
        elif n >= 4:
            f = ws[:n // 4 * 4].view(torch.float32)
            assert bool((f == torch.finfo(torch.float32).max).all())
    assert es(0, "cpu").numel() == 16 and es(-5, "cpu").numel() == 16
    es.check()
    # the same size again: the same arena, refilled
    a = es(4096, "cpu")
    a.fill_(3)
    b = es(4096, "cpu")
    assert a.data_ptr() == b.data_ptr() and int(b[0]) != 3
    es.check()
    b_end = es.arenas[(0, 0, 4096)]
    b_end.arena[b_end.off + 4096] ^= 1               # one byte past a workspace of exactly 4096 bytes
    with pytest.raises(AssertionError, match=r"workspace of 4096 bytes.*byte offset 4096 from the payload start"):
        es.check()


def test_exact_scratch_replaces_ops_scratch(monkeypatch):
    from vit_som_amd import ops
    es = MC.ExactScratch()
    monkeypatch.setattr(ops, "scratch", es)
    assert ops.scratch(100, "cpu").numel() == 100 and es.calls == 1


# ------------------------------------------------------------------ (b) short workspaces are refused on the host
P = 4096                    # stands for a non-null, 16-byte aligned device pointer: nothing is launched, nothing dereferenced
BIG = 1 << 40


def _entries():
    """name -> (need, call(ws, ws_bytes), word the message must contain, refuses a misaligned workspace?).  Every check
    that precedes the workspace check in the entry must pass with these arguments: the test then sees -4, not -1 / -3.
    Read in csrc/*.hip: each entry's VSOM_REQUIRE(..., VSOM_EWORKSPACE, ...) precedes its first VSOM_LAUNCH / launch_gemm."""
    from vit_som_amd._lib import lib as L
    e = {}
    need = L.vsom_linear_bwd_weight_workspace_bytes(70, 10, 24)
    e["vsom_linear_bwd_weight"] = (need, lambda ws, n: L.vsom_linear_bwd_weight(P, 10, P, 24, P, P, 70, 10, 24, ws, n, None),
                                   "workspace", True)
    need = L.vsom_patch_embed_bwd_workspace_bytes(3, 3, 8, 4, 24)
    e["vsom_patch_embed_bwd"] = (need, lambda ws, n: L.vsom_patch_embed_bwd(P, P, P, P, P, 3, 3, 8, 4, 24, ws, n, None),
                                 "workspace", True)
    need = L.vsom_layernorm_bwd_workspace_bytes(37, 16)
    e["vsom_layernorm_bwd"] = (need, lambda ws, n: L.vsom_layernorm_bwd(*[P] * 9, 37, 16, ws, n, None), "workspace", True)
    need = L.vsom_layernorm_bwd_workspace_bytes(8200, 192)
    e["vsom_layernorm_bwd_partial"] = (need, lambda ws, n: L.vsom_layernorm_bwd_partial(*[P] * 7, 8200, 192, ws, n, None),
                                       "partial buffer", True)
    need = L.vsom_linear_bwd_input_ln_partial_bytes(1985, 192)
    ln = (P, 64, P, 1985, 64, 192, P, P, P, P, P, P)
    e["vsom_linear_bwd_input_ln"] = (need, lambda ws, n: L.vsom_linear_bwd_input_ln(*ln, P, P, ws, n, None), "partial buffer", True)
    e["vsom_linear_bwd_input_ln_partial"] = (need, lambda ws, n: L.vsom_linear_bwd_input_ln_partial(*ln, ws, n, None),
                                             "partial buffer", True)
    B, K, Ld = 70, 15, 256
    need = L.vsom_bmu_cosine_workspace_bytes(B, K, Ld)
    e["vsom_bmu_cosine_dots"] = (need, lambda ws, n: L.vsom_bmu_cosine_dots(P, Ld, P, B, K, Ld, ws, n, None), "workspace", False)
    e["vsom_bmu_cosine_finalize"] = (need, lambda ws, n: L.vsom_bmu_cosine_finalize(ws, n, P, P, P, P, B, K, Ld, None),
                                     "workspace", False)
    e["vsom_bmu_cosine_fwd"] = (need, lambda ws, n: L.vsom_bmu_cosine_fwd(P, Ld, P, P, P, P, P, B, K, Ld, ws, n, None),
                                "workspace", False)
    e["vsom_bmu_euclid_fwd"] = (need, lambda ws, n: L.vsom_bmu_euclid_fwd(P, Ld, P, P, P, P, P, B, K, Ld, ws, n, None),
                                "workspace", False)
    need = L.vsom_bmu_manhattan_workspace_bytes(70, 65, 100)
    e["vsom_bmu_manhattan_fwd"] = (need, lambda ws, n: L.vsom_bmu_manhattan_fwd(P, 100, P, P, P, 70, 65, 100, ws, n, None),
                                   "workspace", False)
    need = L.vsom_bmu_cosine_x3_workspace_bytes(B, K, Ld)
    e["vsom_bmu_cosine_x3_dots"] = (need, lambda ws, n: L.vsom_bmu_cosine_x3_dots(P, Ld, P, B, K, Ld, ws, n, None), "workspace", True)
    e["vsom_bmu_cosine_x3_finalize"] = (need, lambda ws, n: L.vsom_bmu_cosine_x3_finalize(P, Ld, P, ws, n, P, P, P, P, None, B, K, Ld, None),
                                        "workspace", False)
    B2, K2, L2 = 200, 70, 72
    need = L.vsom_bmu_cosine_x3_planes_workspace_bytes(B2, K2, L2)
    e["vsom_bmu_cosine_x3_planes_dots"] = (need, lambda ws, n: L.vsom_bmu_cosine_x3_planes_dots(P, P, B2, K2, L2, ws, n, None),
                                           "workspace", True)
    e["vsom_bmu_cosine_x3_planes_finalize"] = (need, lambda ws, n: L.vsom_bmu_cosine_x3_planes_finalize(
        P, L2, P, P, P, ws, n, P, P, P, P, None, B2, K2, L2, None), "workspace", False)
    need = L.vsom_bmu_planes_bytes(K2, L2)
    e["vsom_bmu_planes_from"] = (need, lambda ws, n: L.vsom_bmu_planes_from(P, L2, K2, L2, ws, n, None), "plane buffer", True)
    padded = (K2 * L2 + 255) // 256 * 256
    e["vsom_adamw_step_planes"] = (need, lambda ws, n: L.vsom_adamw_step_planes(P, P, P, P, P, padded + 512, 1e-3, 0.9, 0.999, 1e-8, 1,
                                                                                 1.0, 1, 256, K2, L2, ws, n, None), "plane buffer", True)
    need = L.vsom_som_neigh_workspace_bytes(33, 12)
    e["vsom_som_neigh_loss"] = (need, lambda ws, n: L.vsom_som_neigh_loss(P, P, P, 1.5, None, None, 0.0, None, P, None, None, None,
                                                                          33, 12, 0, ws, n, None), "workspace", False)
    e["vsom_som_weighted_loss"] = (need, lambda ws, n: L.vsom_som_weighted_loss(P, P, None, None, 0.0, P, None, None, None, 33, 12, 0,
                                                                                ws, n, None), "workspace", False)
    need = L.vsom_l1_loss_workspace_bytes(1025)
    e["vsom_l1_loss"] = (need, lambda ws, n: L.vsom_l1_loss(P, P, P, None, 0.0, 1025, ws, n, None), "workspace", False)
    need = L.vsom_l1_unpatchify_workspace_bytes(3, 3, 8, 4)
    e["vsom_l1_unpatchify"] = (need, lambda ws, n: L.vsom_l1_unpatchify(P, P, None, P, None, 0.0, 3, 3, 8, 4, ws, n, None),
                               "workspace", False)
    need = L.vsom_cross_entropy_ls_workspace_bytes(33)
    e["vsom_cross_entropy_ls"] = (need, lambda ws, n: L.vsom_cross_entropy_ls(P, P, 0.1, P, None, 0.0, 33, 100, ws, n, None),
                                  "workspace", False)
    need = L.vsom_umap_knn_workspace_bytes(257, 3)
    e["vsom_umap_knn"] = (need, lambda ws, n: L.vsom_umap_knn(P, 8, 257, 8, 3, 1, P, P, ws, n, None), "workspace", True)
    N, D, k = 70, 8, 3
    need = L.vsom_kmeans_workspace_bytes(N, D, k)
    e["vsom_kmeans_assign"] = (need, lambda ws, n: L.vsom_kmeans_assign(P, D, N, D, P, k, P, P, P, ws, n, None), "workspace", True)
    e["vsom_kmeans_update"] = (need, lambda ws, n: L.vsom_kmeans_update(P, 2 * P, N, D, k, P, P, P, ws, n, None), "workspace", True)
    e["vsom_kmeans_relocate"] = (need, lambda ws, n: L.vsom_kmeans_relocate(P, D, N, D, k, P, P, 1, P, 2 * P, P, P, ws, n, None),
                                 "workspace", True)
    e["vsom_kmeans_colvar"] = (need, lambda ws, n: L.vsom_kmeans_colvar(P, D, N, D, k, P, ws, n, None), "workspace", True)
    need = L.vsom_umap_transform_workspace_bytes(70, 8)
    e["vsom_umap_transform_layout"] = (need, lambda ws, n: L.vsom_umap_transform_layout(
        P, P, P, P, 100, 2 * P, 70, 8, 2, 1.5, 0.9, 1.0, 1.0, 10, 0, 10, 5, 42, P, ws, n, None), "workspace", True)
    return e


# Entries with a caller-sized buffer whose refusals another CPU test already pins down (size, null and alignment alike).
COVERED_ELSEWHERE = {
    "vsom_knn_query": "test_knn_cpu.py::test_argument_refusals_without_a_launch",
    "vsom_knn_ranks": "test_embedding_quality_cpu.py (ranks(ws_bytes=need - 1), ws=24)",
    "vsom_silhouette": "test_silhouette_cpu.py (call(ws_bytes=need - 1), ws=264)",
    "vsom_augment_batch_ragged": "test_ragged_cpu.py (batch(scratch_bytes=100)): scratch_bytes, the image between two crops",
}
BUFFER_ARGS = ("ws_bytes", "part_bytes", "planes_bytes", "scratch_bytes")


def _entries_with_a_sized_buffer():
    """The entries of include/vitsom_hip.h whose parameter list names a caller-sized scratch buffer."""
    src = open(os.path.join(ROOT, "include", "vitsom_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    found = set()
    for name, params in re.findall(r"\b(vsom_[a-z0-9_]+)\s*\(([^)]*)\)", src):
        if any(re.search(rf"\b{a}\b", params) for a in BUFFER_ARGS):
            found.add(name)
    return found


def test_the_refusal_table_covers_every_entry_with_a_workspace():
    """A later entry with a ws_bytes / part_bytes / planes_bytes argument and no refusal test fails here."""
    from vit_som_amd._lib import SIGNATURES
    declared = _entries_with_a_sized_buffer()
    assert declared <= set(SIGNATURES) and len(declared) >= 30
    table = set(_entries())
    assert not (table & set(COVERED_ELSEWHERE))
    assert declared == table | set(COVERED_ELSEWHERE), (sorted(declared - table - set(COVERED_ELSEWHERE)),
                                                         sorted((table | set(COVERED_ELSEWHERE)) - declared))


@pytest.mark.parametrize("name", sorted(_entries()) if os.path.exists(os.path.join(ROOT, "vit_som_amd", "libvitsom_hip.so")) else [])
def test_a_workspace_one_byte_short_is_refused_before_any_launch(name):
    from vit_som_amd._lib import last_error
    need, call, word, checks_alignment = _entries()[name]
    assert need > 0, "the size query must want a workspace at this shape"
    assert call(P, need - 1) == -4, last_error()
    msg = last_error()
    assert word in msg and ("too small" in msg or "<" in msg), msg
    assert call(P, 0) == -4 and call(None, BIG) == -4
    if checks_alignment:
        # documented 16-byte alignment: a pointer at +8 is refused too (VSOM_EALIGN or VSOM_EWORKSPACE), size notwithstanding
        assert call(P + 8, BIG) in (-2, -4), last_error()


def test_the_library_is_there_for_the_refusal_table():
    """The parametrisation above is empty without the shared library: say so instead of passing silently."""
    import vit_som_amd  # noqa: F401
    assert len(_entries()) == 28
