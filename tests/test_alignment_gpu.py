"""Every row of tests/alignment.py on the MI355X, through its ops wrapper, inside guarded arenas (memcheck.py) and with
ExactScratch standing in for ops.scratch (workspaces stay aligned: they are not the subject here):

  1. the aligned call passes the row's check against its CPU reference; its outputs are kept;
  2. each operand alone with its base shifted by 1 element and by 2 (two float32 are 8 bytes: aligned for a `& 7`, not for 16);
  3. each operand that has a leading dimension alone at pitch + 1 and + 2;
  4. every operand shifted by 1 and every pitch + 1 at once, where nothing refuses.

By the table's marking: ELEMENT -- no error, the outputs pass the same check, every output fully written, every guard of
inputs and outputs intact, and the outputs of all ELEMENT variants of a row equal one another bit for bit (there is one
element-wise path, whichever operand sends the call there: a variant that stayed on the 16-byte kernels shows even where the
hardware serves a misaligned wide load); SAME -- as ELEMENT, and the outputs equal the aligned call's bit for bit; REFUSED -- a VsomError
with the named status (or the wrapper's ValueError), every output still poisoned, every in-out operand and every guard
untouched, the workspace guards included.  Outputs a wrapper allocates itself (silhouette, umatrix, the plane buffer of
bmu_planes_from) have no arena: they are held to the row's check and to the bit comparisons only.  No variant is meant to fault: a wide access that straddled an extent would land in the arena's own guards
(64 KiB in front, at least 1 MiB behind) and show there."""
import pytest
import torch

import alignment as A
import memcheck as MC

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    from vit_som_amd import ops as _ops
    prev = _ops.get_gemm_mode()
    yield _ops
    _ops.set_gemm_mode(prev)


def bits(t):
    t = t.contiguous()
    return t.view({4: torch.int32, 8: torch.int64, 1: torch.uint8}[t.element_size()]) if t.is_floating_point() else t


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def build(row, c, moved):
    """-> (tensors, handles): every operand in an arena of its own, `moved` = {name: (shift, pad)}."""
    t, h = {}, {}
    for op in row.ops:
        shift, pad = moved.get(op.name, (0, 0))
        v = c.t[op.name]
        if op.role == A.OUT:
            ld = v.shape[-1] + pad if pad else None
            t[op.name], h[op.name] = MC.guarded(v.shape, v.dtype, DEV, ld=ld, shift=shift)
        else:
            ld = v.shape[-1] + pad if pad else None
            t[op.name], h[op.name] = MC.guarded_copy(v.to(DEV), ld=ld, shift=shift)
        assert t[op.name].data_ptr() % 256 == shift * t[op.name].element_size()
    return t, h


def run(monkeypatch, ops, row, c, moved):
    """One call.  -> (outputs on the CPU, handles, the scratch stand-in); raises what the wrapper raises."""
    t, h = build(row, c, moved)
    es = MC.ExactScratch(MC.FILL_FF)
    with monkeypatch.context() as mp:
        mp.setattr(ops, "scratch", es)
        try:
            extra = row.call(ops, t, c.a)
            torch.cuda.synchronize()
        except Exception as e:
            torch.cuda.synchronize()
            e.alignment_state = (t, h, es)
            raise
    out = {op.name: t[op.name].detach().cpu().clone() for op in row.ops if op.role != A.IN}
    for k, v in (extra if isinstance(extra, dict) else {}).items():
        out[k] = v.detach().cpu().clone() if v is not None else None
    return out, t, h, es


def guards(row, h, es, label):
    bad = []
    for op in row.ops:
        try:
            h[op.name].check(f"{label}: {op.name}")
            if op.role == A.OUT:
                h[op.name].all_written(f"{label}: {op.name}")
        except AssertionError as e:
            bad.append(str(e))
    try:
        es.check()
    except AssertionError as e:
        bad.append(f"{label}: {e}")
    return bad


def case_ids():
    return [(r, m) for r in A.ROWS for m in (r.modes or (None,))]


@pytest.mark.parametrize("row,mode", case_ids(), ids=lambda v: v.id if isinstance(v, A.Row) else A.MODE_IDS.get(v, "default"))
def test_row(monkeypatch, ops, row, mode):
    from vit_som_amd._lib import VsomError
    c = row.make()
    prev = ops.get_gemm_mode()
    if mode is not None:
        ops.set_gemm_mode(mode)
    bad = []
    try:
        # 1. aligned
        base, _, h, es = run(monkeypatch, ops, row, c, {})
        bad += [f"aligned: {m}" for m in row.check(c, base)] + guards(row, h, es, "aligned")
        assert not bad, (row.id, bad)                      # nothing below means anything if the aligned call is wrong
        # 2. - 4.
        elem = elem_label = None
        for label, moved, expect in A.variants(row):
            if isinstance(expect, A.REFUSED):
                try:
                    run(monkeypatch, ops, row, c, moved)
                except (VsomError, ValueError) as e:
                    t, h, es = e.alignment_state
                    name = next(iter(moved))
                    if expect.by == "wrapper":
                        ok = isinstance(e, ValueError) and name in str(e)
                    else:
                        ok = isinstance(e, VsomError) and f"failed with status {expect.code}:" in str(e)
                    if not ok:
                        bad.append(f"{label}: refused with `{e}`, not with {expect}")
                    try:                                   # a stage before the refusing one may have used a workspace
                        es.check()
                    except AssertionError as g:
                        bad.append(f"{label}: {g}")
                    for op in row.ops:
                        try:
                            h[op.name].check(f"{label}: {op.name}")
                        except AssertionError as g:
                            bad.append(str(g))
                        if op.role == A.OUT and t[op.name].numel():
                            _, val = MC._POISON[op.dtype]
                            if not bool((h[op.name]._int_view(h[op.name].arena) == val).all()):
                                bad.append(f"{label}: {op.name} was written although the call was refused")
                        elif op.role != A.OUT and not same_bits(t[op.name].cpu(), c.t[op.name]):
                            bad.append(f"{label}: {op.name} changed although the call was refused")
                else:
                    bad.append(f"{label}: not refused (the table expects {expect})")
                continue
            try:
                out, _, h, es = run(monkeypatch, ops, row, c, moved)
            except (VsomError, ValueError, AssertionError) as e:
                bad.append(f"{label}: {type(e).__name__}: {e}")
                continue
            bad += [f"{label}: {m}" for m in row.check(c, out)] + guards(row, h, es, label)
            if expect == A.SAME:
                for k, v in base.items():
                    if v is not None and not same_bits(out[k], v):
                        bad.append(f"{label}: {k} differs from the aligned call's bits although the operand takes part in no dispatch")
            else:                                          # one element-wise path per row, whichever operand sends the call there
                if elem is None:
                    elem, elem_label = out, label
                for k, v in elem.items():
                    if v is not None and not same_bits(out[k], v):
                        bad.append(f"{label}: {k} differs from the bits of {elem_label}: not the same element-wise path")
    except RuntimeError as e:                              # a HIP error is no test failure: nothing more may run on the device
        if not isinstance(e, VsomError) and ("HIP error" in str(e) or "hipError" in str(e)):
            pytest.exit(f"{row.id}: the device reported `{e}`; no further row is run", returncode=3)
        raise
    finally:
        ops.set_gemm_mode(prev)
    assert not bad, (row.id, bad)


def test_every_row_of_the_table_runs():
    ids = {r.id for r, _ in case_ids()}
    assert ids == set(A.ROW_BY_ID) and len(ids) == len(A.ROWS) >= 57
