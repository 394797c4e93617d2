"""The far-pitch table (tests/far_pitch.py) without a GPU: (a) every pitch lies in its window and every extent on the side of
the source's bound that the table claims, the bounds pinned to the sources; (b) every `long ld*` parameter of
include/vitsom_hip.h is covered by the table in all three windows or left out with a reason; (c) every refusal happens on the
host with VSOM_EUNSUPPORTED and a message that names the limit; (d) the header states the limits and the fall-backs."""
import os
import re

import pytest
import torch

import far_pitch as FP
import memcheck as MC
from alignment import ELEMENT, REFUSED, SAME, SPLIT
from test_alignment_cpu import _comment_before

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vit_som_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "vitsom_hip.h")
IDS = [f"{f.row}:{f.op}" for f in FP.TABLE]


# ------------------------------------------------------------------ (a) windows, bounds, memory
def test_pitch_for_returns_the_smallest_pitch_of_each_window():
    for rows in (2, 12, 33, 70, 130, 193, 2048):
        for size in (4, 8):
            for w in FP.WINDOWS:
                ld = FP.pitch_for(rows, size, w)
                assert ld % 4 == 0 and ld & (ld - 1) != 0 and FP.window_of(rows, ld, size) == w
                # the smallest: the window's first offset divided over the rows and rounded up to a multiple of 4 is the least
                # multiple of 4 in the window (4 less starts the last row below it); the pitch is that, or 4 more where it
                # is a power of two
                start = {FP.SIGNED: (2 ** 31 + 2 ** 24) // size, FP.WRAPPED: (2 ** 32 + 2 ** 24) // size, FP.ELEMENTW: 2 ** 31 + 2 ** 22}[w]
                least = (-(-start // (rows - 1)) + 3) // 4 * 4
                assert (rows - 1) * (least - 4) < start <= (rows - 1) * least and FP.window_of(rows, least - 4, size) != w
                assert ld == (least + 4 if least & (least - 1) == 0 else least), (rows, size, w, ld, least)
    # the windows are what their names say
    ld = FP.pitch_for(130, 4, FP.SIGNED)
    off = 129 * ld * 4
    assert off >= 2 ** 31 and off < 2 ** 32 and off - 2 ** 32 < 0                      # negative as int, valid as unsigned
    ld = FP.pitch_for(130, 4, FP.WRAPPED)
    assert 129 * ld * 4 >= 2 ** 32 and 129 * ld < 2 ** 31
    assert 129 * FP.pitch_for(130, 4, FP.ELEMENTW) >= 2 ** 31 and 129 * FP.pitch_for(130, 8, FP.ELEMENTW) * 8 > 17e9


@pytest.mark.parametrize("key", sorted(FP.BOUNDS))
def test_bounds_are_what_the_table_assumes(key):
    """A bound that somebody moves must fail here, not quietly move a window to the other side of it."""
    assert FP.read_bound(key, CSRC) == FP.BOUNDS[key].value


@pytest.mark.parametrize("f", FP.TABLE, ids=IDS)
def test_every_pitch_lies_in_its_window_and_on_its_side_of_the_bound(f):
    row = FP.ROW_BY_ID[f.row]
    op = FP.op_of(row, f.op)
    assert op.ld, "the table moves pitched operands only"
    rows, cols, size = FP.shape_of(row, f.op)
    assert size == FP.itemsize(op.dtype)
    assert (f.family is None) == all(e in (SAME, None) for e in f.expect), f
    for w, e in zip(FP.WINDOWS, f.expect):
        if e is None:                                                                  # a window that is not run has its reason
            assert all(len(FP.WINDOW_LEFT_OUT[(entry, name, w)]) > 20 for entry, name in f.covers) and f.covers, (f, w)
            continue
        ld = FP.pitch_for(rows, size, w)
        assert ld % 4 == 0 and ld >= cols and FP.window_of(rows, ld, size) == w
        # below EVERY bound in `signed`, whichever formula a kernel family applies to the operand
        if w == FP.SIGNED:
            assert e == SAME
            if size == 4:
                for fam in FP.FAMILIES:
                    assert FP.EXTENT[fam](rows, ld, cols) < FP.limit_of(fam, CSRC), (fam, w)
        elif f.family is not None:
            assert e == ELEMENT or (isinstance(e, REFUSED) and e.code == FP.EUNSUPPORTED)
            assert FP.EXTENT[f.family](rows, ld, cols) >= FP.limit_of(f.family, CSRC), (f.family, w)
        else:
            assert e == SAME


def test_the_memory_budget():
    worst = max(FP.peak_bytes(r) for r in FP.FAR_ROWS)
    assert worst <= FP.PEAK_BYTES == 40 * 2 ** 30, worst
    # the largest single arena: an 8-byte operand in `element` (16 GiB in front of 16 GiB and a little)
    assert FP.arena_bytes(130, 52, 8, FP.ELEMENTW) <= FP.PEAK_BYTES
    for size in (4, 8):
        assert FP.front_for(size, FP.SIGNED) >= 2 ** 31 and FP.front_for(size, FP.WRAPPED) >= 2 ** 31
        assert FP.front_for(size, FP.ELEMENTW) >= 2 ** 31 * size
    assert MC.FAR_PIECE * 4 + MC.FAR_PIECE <= 2 ** 30                                  # what check() holds at a time


def test_rows_are_well_formed():
    from vit_som_amd import ops
    assert [f.row for f in FP.TABLE if f.row not in FP.ROW_BY_ID] == []
    assert len({(f.row, f.op) for f in FP.TABLE}) == len(FP.TABLE)
    for r in FP.FAR_ROWS:
        c = r.make()
        assert hasattr(ops, r.wrapper) or r.wrapper == "lib", r.id
        assert sorted(op.name for op in r.ops) == sorted(c.t), r.id
        pitched = {op.name for op in r.ops if op.ld}
        moved = {n for f in FP.FAR_BY_ROW[r.id] for n in (f.op,) + tuple(f.tied)}
        assert pitched == moved, (r.id, pitched)                                       # every pitched operand of a row is moved
        for op in r.ops:
            v = c.t[op.name]
            assert isinstance(v, FP.Spec) == (op.role == FP.OUT) and v.dtype == op.dtype, (r.id, op.name)
            assert not op.ld or (len(v.shape) == 2 and v.shape[0] >= 2), (r.id, op.name)
        labels = [v[0] for v in FP.variants(r)]
        n_far = len(FP.FAR_BY_ROW[r.id])
        not_run = sum(e is None for f in FP.FAR_BY_ROW[r.id] for e in f.expect)
        assert len(labels) == len(set(labels)) == 3 * n_far - not_run + (n_far > 1)
    # every operand alignment.py marks ld=True is here
    import alignment as A
    for r in A.ROWS:
        for op in r.ops:
            if op.ld:
                assert any(f.op == op.name for f in FP.FAR_BY_ROW.get(r.id, [])), (r.id, op.name)


# ------------------------------------------------------------------ (b) completeness
def header_ld_parameters():
    """[(entry, parameter, argument position)] for every `long ld*` parameter of every vsom_* declaration."""
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    src = re.sub(r"//[^\n]*", " ", src)
    out = []
    for m in re.finditer(r"^(?:int|long|size_t)\s+(vsom_\w+)\s*\(([^;]*?)\)\s*;", src, flags=re.M | re.S):
        for i, a in enumerate(m.group(2).split(",")):
            a = " ".join(a.split())
            if re.fullmatch(r"long ld\w*", a):
                out.append((m.group(1), a.split()[1], i))
    return out


def test_every_ld_parameter_of_the_header_is_covered_or_left_out():
    import ctypes as C
    from vit_som_amd._lib import SIGNATURES
    params = header_ld_parameters()
    for entry, name, i in params:                                                     # the binding agrees, position by position
        assert SIGNATURES[entry][1][i] is C.c_long, (entry, name, i)
    covered = {}
    for f in FP.TABLE:
        for pair in f.covers:
            covered.setdefault(pair, []).append(f)
    problems = []
    for entry, name, _ in params:
        pair = (entry, name)
        if pair in FP.LEFT_OUT:
            if len(FP.LEFT_OUT[pair]) <= 20 or pair in covered:
                problems.append(f"{entry}({name}): left out without a reason, or left out and covered")
        elif pair not in covered:
            problems.append(f"{entry}({name}): no entry of far_pitch.TABLE moves it and far_pitch.LEFT_OUT does not name it")
    known = {(e, n) for e, n, _ in params}
    problems += [f"{p}: covered by the table but not a `long ld*` parameter of the header" for p in covered if p not in known]
    problems += [f"{p}: in LEFT_OUT but not a `long ld*` parameter of the header" for p in FP.LEFT_OUT if p not in known]
    assert not problems, "\n".join(problems)
    # every covering entry runs all three windows, bar those WINDOW_LEFT_OUT names with a reason, and its row reaches the C
    # entry it names
    not_run = set()
    for pair, fs in covered.items():
        for f in fs:
            assert len(f.expect) == 3 and pair[0] in FP.ROW_BY_ID[f.row].entry, (pair, f.row)
            not_run |= {pair + (w,) for w, e in zip(FP.WINDOWS, f.expect) if e is None}
    assert not_run == set(FP.WINDOW_LEFT_OUT) and all(len(v) > 20 for v in FP.WINDOW_LEFT_OUT.values()), not_run ^ set(FP.WINDOW_LEFT_OUT)
    assert len(params) == 82 and len(covered) == 79 and len(FP.LEFT_OUT) == 3 and len(FP.WINDOW_LEFT_OUT) == 1


# ------------------------------------------------------------------ (c) refusals on the host
def _refusals():
    from vit_som_amd._lib import lib
    return FP.host_refusals(lib)


@pytest.mark.parametrize("entry,operand", FP.REFUSING)
def test_an_operand_of_4_gb_is_refused_before_any_launch(entry, operand):
    from vit_som_amd._lib import last_error, lib
    code, words, rows, size, cols, call = _refusals()[(entry, operand)]
    prev = lib.vsom_get_gemm_mode()
    lib.vsom_set_gemm_mode(SPLIT)
    try:
        # a call that is NOT refused goes on to launch, on the stand-in pointers: only where there is no device to launch on
        # (with one, test_far_pitch_gpu.py runs the contiguous and the signed call on real operands)
        if not torch.cuda.is_available():
            assert call(cols) != code, f"{entry}: the contiguous call already answers {code}: {last_error()}"
            rc = call(FP.pitch_for(rows, size, FP.SIGNED))
            assert rc != code, f"{entry}: refused in the signed window, below 4 GB: {last_error()}"
        for w in (FP.WRAPPED, FP.ELEMENTW):
            rc = call(FP.pitch_for(rows, size, w))
            msg = last_error()
            assert rc == code == -3, f"{entry}: {operand} at the {w} pitch answers {rc}, not {code}: {msg}"
            assert words in msg, f"{entry}: the message does not name the limit ({words}): {msg}"
    finally:
        lib.vsom_set_gemm_mode(prev)


def test_every_refused_operand_of_the_table_is_called_on_the_host():
    called = {e for e, _ in _refusals()}
    assert len(called) == 5
    for f in FP.TABLE:
        if f.expect == FP.NO4GB:
            assert f.covers and all(e in called for e, _ in f.covers), f


def test_a_plane_image_of_2_gb_is_refused_whatever_the_pitch():
    from vit_som_amd._lib import last_error, lib
    limit = FP.read_bound("planes", CSRC)
    per_block = 2 * (256 // 32) * 2048                                                # bmu_x3.hip: planes_image_bytes, L = 256
    fits, over = (limit // per_block - 1) * 32, (limit // per_block) * 32
    for entry, call in FP.planes_refusals(lib).items():
        if not torch.cuda.is_available():                                              # not refused: it would launch
            assert call(fits) != -3, (entry, last_error())
        assert call(over) == -3 and "2 GB" in last_error(), (entry, last_error())


# ------------------------------------------------------------------ (d) the header
def _said_before(src, entry):
    """The words of the comment that ends last before the declaration of `entry`, without the stars that lead its lines."""
    lines = [re.sub(r"^\s*\*(?!/)\s?", "", line) for line in _comment_before(src, entry).splitlines()]
    return " ".join(" ".join(lines).split())


def test_the_header_states_every_limit():
    src = open(HEADER).read()
    for entry, words in FP.HEADER_REFUSES.items():
        comment = _said_before(src, entry)
        for w in words:
            assert w in comment, f"{entry}: its comment in include/vitsom_hip.h does not say `{w}`"
    for entry, owner in FP.HEADER_FALLS_BACK.items():
        comment = _said_before(src, owner)
        assert FP.FALLBACK_WORDS in comment, f"{owner}: its comment does not say that operands of `{FP.FALLBACK_WORDS}`"
        assert entry in comment or entry == owner, f"{entry}: the comment of {owner} does not name it"
    # every BUFFER operand's entry is one of them
    for f in FP.TABLE:
        if f.expect == FP.BUFFER:
            assert all(e in FP.HEADER_FALLS_BACK for e, _ in f.covers), f


# ------------------------------------------------------------------ the arena itself (memcheck.GuardedFar), at small sizes
DTYPES = [torch.float32, torch.float64, torch.int64]


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_far_arena_layout_and_fill(dtype):
    v, h = MC.guarded_far((7, 12), dtype, "cpu", ld=1004)
    size = h.size
    assert v.shape == (7, 12) and v.stride() == (1004, 1) and v.data_ptr() % 256 == 0
    assert h.front == MC.FRONT_GUARD and h.back == 1 << 20 == MC.FAR_BACK
    assert h.arena.numel() >= h.front + (6 * 1004 + 12) * size + h.back
    assert h.untouched()
    words = h.arena.view(torch.int32)
    assert int((words != MC.GUARD_WORD).sum()) == 7 * 12 * size // 4                  # the payload rows and nothing else
    for piece in (MC.FAR_PIECE, 1001, 100):                                           # one piece, ragged pieces, many pieces
        h.check("fresh", piece=piece)
    with pytest.raises(AssertionError, match=r"84 of 84 elements were never written, the first at flat index 0 \(row 0, column 0"):
        h.all_written("out")
    v.fill_(1)
    v[5, 3] = torch.tensor([MC._POISON[dtype][1]], dtype=MC._POISON[dtype][0]).view(dtype)[0]
    with pytest.raises(AssertionError, match=r"1 of 84 elements were never written, the first at flat index 63 \(row 5, column 3"):
        h.all_written("out")
    h.check("written", piece=513)
    big, hb = MC.guarded_far((3, 4), dtype, "cpu", ld=64, front=MC.FRONT_GUARD + 4096)
    assert hb.front == MC.FRONT_GUARD + 4096 and big.data_ptr() % 256 == 0


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("piece", [MC.FAR_PIECE, 777])
def test_far_arena_reports_damage_with_the_right_offset(dtype, piece):
    t = (torch.arange(35) - 17).view(5, 7).to(dtype)
    v, h = MC.guarded_far_copy(t, ld=300)
    assert torch.equal(v, t)
    h.check("input", piece=piece)
    size = h.size
    saved = h.arena.clone()
    cases = [(h.off + 2 * 300 * size + 7 * size, "the gap after row 2"),              # the first byte behind row 2
             (h.off + 3 * 300 * size - 1, "the gap after row 2"),                      # the last byte in front of row 3
             (h.off - 1, "the front guard"), (5, "the front guard"),
             (h.off + h.nbytes, "the back guard"), (h.off + h.nbytes + h.back - 1, "the back guard")]
    for at, where in cases:
        h.arena[at] ^= 0x10
        with pytest.raises(AssertionError) as e:
            h.check("input", piece=piece)
        assert f"the first at byte offset {at - h.off} from the payload start ({where};" in str(e.value), (at, str(e.value))
        assert "1 guard words damaged" in str(e.value)
        h.arena.copy_(saved)
        h.check("input", piece=piece)
    # the first of several, in another piece than the last
    h.arena[h.off + 300 * size + 7 * size + 2] = 0
    h.arena[h.off + 4 * 300 * size - 3] = 0
    with pytest.raises(AssertionError, match=rf"2 guard words damaged, the first at byte offset {300 * size + 7 * size + 2} "):
        h.check("input", piece=piece)
    h.arena.copy_(saved)
    # a write inside a payload row is no guard damage
    v[4, 6] = 99
    h.check("input", piece=piece)


def test_far_arena_in_the_callers_memory():
    """`backing`: the arena is a slice of memory the caller reuses; the same fill, the same checks, nothing outside the slice."""
    words = torch.zeros(400000, dtype=torch.int32)
    v, h = MC.guarded_far((5, 8), torch.float32, "cpu", ld=1000, backing=words[1000:])
    n = h.words.numel()
    assert h.words.data_ptr() == words[1000:].data_ptr() and v.data_ptr() % 256 == 0 and n < 399000
    assert not bool(words[:1000].any()) and not bool(words[1000 + n:].any())         # filled to the arena's end and no further
    h.check("reused", piece=4099)
    assert h.untouched()
    t = torch.arange(40.).view(5, 8)
    v2, h2 = MC.guarded_far_copy(t, ld=1000, backing=words[1000:])                    # the next arena in the same memory
    assert torch.equal(v2, t)
    h2.check("reused", piece=4099)
    h2.arena[h2.off + 1000 * 4 - 1] = 1
    with pytest.raises(AssertionError, match=rf"the first at byte offset {1000 * 4 - 1} from the payload start \(the gap after row 0;"):
        h2.check("reused", piece=4099)
    with pytest.raises(AssertionError):
        MC.guarded_far((5, 8), torch.float32, "cpu", ld=1000, backing=words[:100])   # too small for the arena


def test_far_columns_are_operands_of_one_arena():
    """Blocks that share one ld as column slices of one wide payload: the guards are the arena's, written / untouched a block's."""
    h = MC.GuardedFar(6, 12, torch.float64, "cpu", ld=500)
    a, b, c = (MC.FarColumns(h, k, k + 4) for k in (0, 4, 8))
    assert b.view.shape == (6, 4) and b.view.stride() == (500, 1) and b.view.data_ptr() == h.view.data_ptr() + 32
    a.view.copy_(torch.arange(24.).view(6, 4).double())
    assert not a.untouched() and b.untouched() and c.untouched()
    a.all_written("a")
    c.view[:, :3] = 1.0
    with pytest.raises(AssertionError, match=r"6 of 24 elements were never written, the first at flat index 3 \(row 0, column 3 of columns \[8, 12\)"):
        c.all_written("c")
    b.check("b", piece=999)                                                           # every block of a row is payload
    h.arena[h.off + 12 * 8] ^= 1                                                      # the first byte behind the last block of row 0
    with pytest.raises(AssertionError, match=r"the first at byte offset 96 from the payload start \(the gap after row 0;"):
        a.check("a", piece=999)
