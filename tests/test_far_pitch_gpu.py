"""Every entry of tests/far_pitch.py on the MI355X, through its ops wrapper, with ExactScratch standing in for ops.scratch:

  1. the contiguous call, inside ordinary memcheck arenas, passes the row's check against its CPU reference; its outputs
     are kept (and, for a row with ELEMENT expectations, those of alignment.py's `pitch + 1` variant);
  2. each pitched operand alone inside a far arena (memcheck.GuardedFar) in `signed`, `wrapped`, `element`, in that order;
  3. all pitched operands of the row at once in `signed`.

By the table's marking: SAME -- no error, the row's check passes, every output fully written, every guard of every operand
intact (front guard, every gap between the far rows, back guard, the workspaces'), the outputs bit-identical to the contiguous
call's; ELEMENT -- the same, the bits those of alignment.py's element-wise variant; REFUSED -- a VsomError with status -3
whose message names the limit, every output still poisoned, every input and guard untouched.  One far arena is alive at a
time (all of a row's in step 3): the arenas of a variant are carved from one allocation of the table's peak, below 40 GiB
(the fixture `pool` says why), and filled anew; without room for that they are allocated one by one and freed before the
next is made, and a variant whose arenas do not fit the free device memory is skipped with that reason, never shrunk.
One line per variant: FAR|row[mode]|operand|window|ld|arena GiB|verdict (and a FARTIME| line: where its time went).

No variant is meant to fault: a truncated or sign-extended 32-bit offset lands inside the far arena (far_pitch.front_for).  A
HIP error ends the session as in test_alignment_gpu.py: nothing more runs on the device."""
import re
import time

import pytest
import torch

import alignment as A
import far_pitch as FP
import memcheck as MC
from test_alignment_gpu import same_bits

pytestmark = pytest.mark.gpu

DEV = "cuda"
SECONDS = [0.0, 0.0]                     # of the last run(): making the arenas, the call
LIMIT_WORDS = ("4 GB", "2 GB")


@pytest.fixture(scope="module")
def ops():
    from vit_som_amd import ops as _ops
    prev = _ops.get_gemm_mode()
    yield _ops
    _ops.set_gemm_mode(prev)


@pytest.fixture(scope="module")
def pool():
    """One allocation of the table's peak (far_pitch.peak_bytes, at most PEAK_BYTES), made once: the far arenas of a variant
    are carved from it and filled anew, so the budget holds as it would with an allocation per arena -- which stalled for
    3 to 6 s in hipMalloc on one variant in thirty.  Without room for it the arenas are allocated and freed one by one."""
    need = max(FP.peak_bytes(r) for r in FP.FAR_ROWS)
    assert need <= FP.PEAK_BYTES
    torch.cuda.empty_cache()
    box = {"words": None}
    if need + FP.GIB <= torch.cuda.mem_get_info()[0]:
        box["words"] = torch.empty(need // 4 + 4096, dtype=torch.int32, device=DEV)      # each carved arena is rounded up to 256 bytes
    yield box
    box["words"] = None
    torch.cuda.empty_cache()


def far_plan(row, far):
    """[(operands, rows, columns, dtype size, ld, front, arena bytes)]: the far arenas of `far` = {name: window}
    (far_pitch.arenas: one per operand, or one for a group of column slices)."""
    return [(names, rows, cols, size, FP.pitch_for(rows, size, w), FP.front_for(size, w), FP.arena_bytes(rows, cols, size, w))
            for names, rows, cols, size, w in FP.arenas(row, far)]


def build(row, c, far, pad, words=None):
    """-> (tensors, handles): every operand in an arena of its own -- `far` = {name: window} in far arenas (carved from
    `words` when given; the operands of a wide group side by side in one), `pad` = {name: 1} at pitch + 1 (alignment.py's
    element-wise variant)."""
    t, h = {}, {}
    at = 0
    role = {op.name: op.role for op in row.ops}
    for names, rows, cols, _, ld, front, nbytes in far_plan(row, far):
        backing = None
        if words is not None:
            n = (nbytes + 255) // 256 * 64
            backing, at = words[at:at + n], at + n
            assert backing.numel() == n, "the pool is the table's peak"
        arena = MC.GuardedFar(rows, cols, c.t[names[0]].dtype, DEV, ld, front=front, backing=backing)      # poisoned throughout
        c0 = 0
        for name in names:
            v = c.t[name]
            h[name] = MC.FarColumns(arena, c0, c0 + v.shape[1])
            t[name] = h[name].view
            if role[name] != A.OUT:
                t[name].copy_(v.to(DEV))
            assert t[name].stride() == (ld, 1) and t[name].shape == tuple(v.shape) and t[name].data_ptr() % 16 == 0
            c0 += v.shape[1]
        assert c0 == cols and arena.view.data_ptr() % 256 == 0
    for op in row.ops:
        if op.name in t:
            continue
        v = c.t[op.name]
        ld = v.shape[-1] + pad[op.name] if op.name in pad else None
        if op.role == A.OUT:
            t[op.name], h[op.name] = MC.guarded(v.shape, v.dtype, DEV, ld=ld)
        else:
            t[op.name], h[op.name] = MC.guarded_copy(v.to(DEV), ld=ld)
        assert t[op.name].data_ptr() % 256 == 0
    return t, h


def run(monkeypatch, ops, row, c, far=None, pad=None, words=None):
    """One call.  -> (outputs on the CPU, tensors, handles, the scratch stand-in); raises what the wrapper raises."""
    t0 = time.perf_counter()
    t, h = build(row, c, far or {}, pad or {}, words)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    es = MC.ExactScratch(MC.FILL_FF)
    with monkeypatch.context() as mp:
        mp.setattr(ops, "scratch", es)
        try:
            extra = row.call(ops, t, c.a)
            torch.cuda.synchronize()
        except Exception as e:
            torch.cuda.synchronize()
            e.far_state = (t, h, es)
            raise
        finally:
            SECONDS[:] = [t1 - t0, time.perf_counter() - t1]
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


def refused_state(row, c, e, label):
    """What a refused call must have left: every output poisoned, every input as it was, every guard intact."""
    t, h, es = e.far_state
    bad = []
    try:
        es.check()
    except AssertionError as g:
        bad.append(f"{label}: {g}")
    for op in row.ops:
        try:
            h[op.name].check(f"{label}: {op.name}")
        except AssertionError as g:
            bad.append(str(g))
        if op.role == A.OUT and t[op.name].numel():
            hh = h[op.name]
            still = hh.untouched() if isinstance(hh, MC.FarColumns) else bool((hh._int_view(hh.arena) == MC._POISON[op.dtype][1]).all())
            if not still:
                bad.append(f"{label}: {op.name} was written although the call was refused")
        elif op.role != A.OUT and not same_bits(t[op.name].cpu(), c.t[op.name]):
            bad.append(f"{label}: {op.name} changed although the call was refused")
    return bad


def ends_the_session(row, e):
    """A HIP error (torch's RuntimeError, or a positive hipError_t in a VsomError) is no test failure: nothing more may run
    on the device."""
    from vit_som_amd._lib import VsomError
    text = str(e)
    if isinstance(e, VsomError):
        m = re.search(r"failed with status (-?\d+):", text)
        fault = m is not None and int(m.group(1)) > 0
    else:
        fault = isinstance(e, RuntimeError) and ("HIP error" in text or "hipError" in text)
    if fault:
        pytest.exit(f"{row.id}: the device reported `{e}`; no further row is run", returncode=3)


def case_ids():
    return [(r, m) for r in FP.FAR_ROWS for m in (r.modes or (None,))]


def _id(v):
    return v.id if isinstance(v, A.Row) else A.MODE_IDS.get(v, "default")


@pytest.mark.parametrize("row,mode", case_ids(), ids=_id)
def test_row(monkeypatch, ops, pool, row, mode):
    from vit_som_amd._lib import VsomError
    c = row.make()
    tag = f"{row.id}[{_id(mode)}]"
    prev = ops.get_gemm_mode()
    if mode is not None:
        ops.set_gemm_mode(mode)
    bad, skipped = [], []
    try:
        # 1. contiguous
        base, _, h, es = run(monkeypatch, ops, row, c)
        bad += [f"contiguous: {m}" for m in row.check(c, base)] + guards(row, h, es, "contiguous")
        assert not bad, (row.id, bad)                      # nothing below means anything if the contiguous call is wrong
        # the element-wise reference is taken once, at the first such operand's pitch + 1: test_alignment_gpu.py holds every
        # row to ONE element-wise path, bit for bit, whichever operand sends the call there
        elem = None
        if any(e == A.ELEMENT for f in FP.FAR_BY_ROW[row.id] for e in f.expect):
            name = next(f.op for f in FP.FAR_BY_ROW[row.id] if A.ELEMENT in f.expect)
            assert FP.op_of(row, name).pitched == A.ELEMENT, (row.id, name)
            elem, _, h, es = run(monkeypatch, ops, row, c, pad={name: 1})
            bad += [f"{name}.ld+1: {m}" for m in row.check(c, elem)] + guards(row, h, es, f"{name}.ld+1")
        del h, es
        # 2., 3.
        for label, far, expect in FP.variants(row):
            torch.cuda.empty_cache()
            plan = far_plan(row, far)
            words = pool["words"]
            need, free = sum(p[6] for p in plan), (1 << 62) if words is not None else torch.cuda.mem_get_info()[0]
            where = "|".join([tag, label.split("@")[0], label.split("@")[1], "+".join(str(p[4]) for p in plan), f"{need / FP.GIB:.2f}"])
            if need + (1 << 30) > free:
                skipped.append(f"{label}: needs {need / FP.GIB:.1f} GiB, {free / FP.GIB:.1f} GiB are free")
                print(f"FAR|{where}|skipped: {skipped[-1]}")
                continue
            n_bad, began = len(bad), time.perf_counter()
            if isinstance(expect, A.REFUSED):
                try:
                    run(monkeypatch, ops, row, c, far, words=words)
                except VsomError as e:
                    ends_the_session(row, e)
                    if f"failed with status {expect.code}:" not in str(e) or not any(w in str(e) for w in LIMIT_WORDS):
                        bad.append(f"{label}: refused with `{e}`, not with status {expect.code} and the limit")
                    bad += refused_state(row, c, e, label)
                    del e.far_state
                else:
                    bad.append(f"{label}: not refused (the table expects {expect})")
            else:
                try:
                    out, t, h, es = run(monkeypatch, ops, row, c, far, words=words)
                except (VsomError, ValueError, AssertionError) as e:
                    ends_the_session(row, e)
                    bad.append(f"{label}: {type(e).__name__}: {e}")
                    e.far_state = None
                else:
                    bad += [f"{label}: {m}" for m in row.check(c, out)] + guards(row, h, es, label)
                    want, what = (base, "the contiguous call's") if expect == A.SAME else (elem, "the element-wise variant's")
                    for k, v in want.items():
                        if v is not None and not same_bits(out[k], v):
                            bad.append(f"{label}: {k} differs from {what} bits")
                    del out, t, h, es
            verdict = "FAILED" if len(bad) > n_bad else "refused" if isinstance(expect, A.REFUSED) else expect
            print(f"FAR|{where}|{verdict}")
            torch.cuda.empty_cache()
            whole = time.perf_counter() - began
            print(f"FARTIME|{where}|arenas {SECONDS[0]:.3f} s|call {SECONDS[1]:.3f} s|checks and free {whole - sum(SECONDS):.3f} s")
    except RuntimeError as e:
        ends_the_session(row, e)
        raise
    finally:
        ops.set_gemm_mode(prev)
        torch.cuda.empty_cache()
    assert not bad, (row.id, bad)
    if skipped:
        pytest.skip(f"{row.id}: {skipped}")


def test_every_row_of_the_table_runs():
    ids = {r.id for r, _ in case_ids()}
    assert ids == set(FP.FAR_BY_ROW) and len(ids) == len(FP.FAR_ROWS)
    assert {r.id for r in A.ROWS if any(op.ld for op in r.ops)} <= ids
