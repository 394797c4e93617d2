"""The alignment table (tests/alignment.py) without a GPU: (a) every refusal of a misaligned operand happens on the host, with
the status the table names and a message that speaks of alignment or names the operand; (b) every alignment test in the
sources is pinned to the rows that cross it, or to a reason -- a test added later fails here until somebody has decided how it
is tested; (c) the GEMM-family rows really straddle launch_gemm's choice; (d) include/vitsom_hip.h states every requirement
the library enforces."""
import os
import re

import pytest

import alignment as A
from test_launch_plan_cpu import describe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vit_som_amd", "csrc")
HAVE_LIB = os.path.exists(os.path.join(ROOT, "vit_som_amd", "libvitsom_hip.so"))


@pytest.fixture(scope="module")
def lib():
    from vit_som_amd._lib import lib as _lib
    return _lib


def _refusals():
    if not HAVE_LIB:
        return {}
    from vit_som_amd._lib import lib as _lib
    return A.host_refusals(_lib)


# ------------------------------------------------------------------ (a) refusals on the host
@pytest.mark.parametrize("entry,operand", sorted(_refusals()))
def test_a_misaligned_operand_is_refused_before_any_launch(entry, operand):
    from vit_som_amd._lib import last_error
    code, call = _refusals()[(entry, operand)]
    aligned = call(lambda name: A.P)
    assert aligned != code, f"{entry}: the aligned call already answers {code}: {last_error()}"
    for moved in A.WEAK.get(operand, (4, 8)):
        rc = call(lambda name: A.P + moved if name == operand else A.P)
        msg = last_error()
        assert rc == code, f"{entry}: {operand} at +{moved} bytes answers {rc}, not {code}: {msg}"
        said = "align" in msg.lower() or re.search(rf"\b{re.escape(operand)}\b", msg) is not None
        assert said, f"{entry}: the message neither mentions alignment nor names {operand}: {msg}"


def test_the_library_is_there_for_the_refusals():
    """The parametrisation above is empty without the shared library: say so instead of passing silently."""
    import vit_som_amd  # noqa: F401
    assert len(_refusals()) >= 50


def test_every_refused_operand_of_the_table_is_called_on_the_host():
    """Each REFUSED marking of a row reaches one of the host calls above, under the C entry's name for the operand."""
    called = set(_refusals())
    missing = []
    for r in A.ROWS:
        entries = [e.strip() for e in r.entry.split("+")]
        for op in r.ops:
            if not isinstance(op.shifted, A.REFUSED):        # (a refused pitch is no pointer: the GPU rows run it)
                continue
            if not any((e, A.ENTRY_OPERAND.get(e, {}).get(op.name, op.name)) in called for e in entries):
                missing.append((r.id, op.name))
    assert not missing, missing


def test_the_refusal_codes_of_table_and_host_calls_agree():
    calls = _refusals()
    for r in A.ROWS:
        entries = [e.strip() for e in r.entry.split("+")]
        for op in r.ops:
            if isinstance(op.shifted, A.REFUSED):
                codes = {calls[(e, A.ENTRY_OPERAND.get(e, {}).get(op.name, op.name))][0] for e in entries
                         if (e, A.ENTRY_OPERAND.get(e, {}).get(op.name, op.name)) in calls}
                assert op.shifted.code in codes, (r.id, op.name, op.shifted, codes)


# ------------------------------------------------------------------ (b) completeness
def _source_sites():
    """file -> [(line number, stripped line, alignment tests on it)] for every file under csrc."""
    found = {}
    for name in sorted(os.listdir(CSRC)):
        if not name.endswith((".hip", ".h")):
            continue
        for no, line in enumerate(open(os.path.join(CSRC, name)), 1):
            n = len(A.SITE.findall(line))
            if n:
                found.setdefault(name, []).append((no, line.strip(), n))
    return found


def test_every_alignment_test_in_the_sources_is_pinned():
    found = _source_sites()
    assert set(found) == set(A.SITES), (sorted(set(found) - set(A.SITES)), sorted(set(A.SITES) - set(found)))
    problems = []
    for name, lines in found.items():
        pins = list(A.SITES[name])
        for no, text, n in lines:
            hit = next((p for p in pins if p[0] in text), None)
            if hit is None:
                problems.append(f"{name}:{no}: no entry of alignment.SITES for `{text}`")
                continue
            pins.remove(hit)
            if hit[1] != n:
                problems.append(f"{name}:{no}: {n} alignment tests on the line, the table counts {hit[1]}")
        problems += [f"{name}: `{p[0]}` is in alignment.SITES but no longer in the source" for p in pins]
    assert not problems, "\n".join(problems)
    total = sum(n for lines in found.values() for _, _, n in lines)
    assert total == sum(p[1] for pins in A.SITES.values() for p in pins) and total == 124


def test_every_pin_names_rows_of_the_table_or_a_reason():
    for name, pins in A.SITES.items():
        for needle, _, who in pins:
            if isinstance(who, str):
                assert who in A.LEFT_OUT and len(A.LEFT_OUT[who]) > 20, (name, needle, who)
            else:
                assert who and all(w in A.ROW_BY_ID for w in who), (name, needle, who)
    used = {who for pins in A.SITES.values() for _, _, who in pins if isinstance(who, str)}
    assert used == set(A.LEFT_OUT), (used ^ set(A.LEFT_OUT))
    pinned = {w for pins in A.SITES.values() for _, _, who in pins if not isinstance(who, str) for w in who}
    # rows no site pins: their kernels take no part in any choice (every operand SAME)
    free = {r.id for r in A.ROWS} - pinned
    assert all(all(op.shifted == A.SAME for op in A.ROW_BY_ID[i].ops) for i in free), free


def test_the_existing_tests_the_reasons_name_exist():
    tests = os.path.join(ROOT, "tests")
    for key, where, what in (("agglomerative", "test_agglomerative_gpu.py", '"offset"'),
                             ("map_stats", "test_mapquality_gpu.py", "def test_map_stats_crafted_rows_and_unaligned_base"),
                             ("proto_mosaic", "test_mapviz_gpu.py", "def test_proto_mosaic_unaligned_pred")):
        assert where.split(":")[0] in A.LEFT_OUT[key]
        assert what in open(os.path.join(tests, where)).read(), (key, where, what)


# ------------------------------------------------------------------ (c) the GEMM rows straddle the choice
GEMM_ROWS = [r for r in A.ROWS if r.plan is not None]


@pytest.mark.parametrize("row", GEMM_ROWS, ids=lambda r: r.id)
def test_gemm_rows_take_the_16_byte_path_aligned_and_leave_it_misaligned(lib, row):
    op, shape = row.plan
    prev = lib.vsom_get_gemm_mode()
    try:
        for mode in A.ALL_MODES:
            assert lib.vsom_set_gemm_mode(mode) == 0
            fast, slow = describe(lib, op, shape, 1), describe(lib, op, shape, 0)
            assert fast is not None and fast[3] == 1, (row.id, mode, fast)
            assert slow is not None and slow[3] == 0 and slow[0] == "f32", (row.id, mode, slow)
    finally:
        lib.vsom_set_gemm_mode(prev)


def test_every_gemm_family_row_has_a_plan():
    assert len(GEMM_ROWS) == 14
    assert {r.wrapper for r in GEMM_ROWS} >= {"linear_fwd", "linear_gelu_fwd", "linear_relu_fwd", "linear_residual_fwd", "linear_bwd_input",
                                             "linear_bwd_input_t", "linear_bwd_weight", "som_bwd", "bmu_euclid_fwd", "bmu_cosine_fwd"}


# ------------------------------------------------------------------ (d) the header
def _comment_before(src, entry):
    """The comment that ends last before the first declaration of `entry`."""
    m = re.search(rf"^(?:int|long|size_t)\s+{entry}\s*\(", src, flags=re.M)
    assert m, entry
    ends = [c for c in re.finditer(r"/\*.*?\*/", src[:m.start()], flags=re.S)]
    assert ends, entry
    return ends[-1].group(0)


def test_the_header_states_every_requirement_the_library_enforces():
    src = open(os.path.join(ROOT, "include", "vitsom_hip.h")).read()
    refused = {e for e, _ in _refusals()} if HAVE_LIB else set(A.HEADER_WORDS)
    # entries that share the comment of an entry declared before them: that comment names them with their requirement
    shared = {"vsom_linear_bwd_input_ln_partial": "vsom_linear_bwd_input_ln", "vsom_bmu_cosine_x3_finalize": "vsom_bmu_cosine_x3_dots",
              "vsom_bmu_cosine_x3_planes_dots": "vsom_bmu_planes_from", "vsom_bmu_cosine_x3_planes_finalize": "vsom_bmu_planes_from"}
    assert refused == set(A.HEADER_WORDS) | set(shared), refused ^ (set(A.HEADER_WORDS) | set(shared))
    for entry, words in A.HEADER_WORDS.items():
        comment = " ".join(_comment_before(src, entry).split())
        for w in words:
            assert w in comment, f"{entry}: its comment in include/vitsom_hip.h does not say `{w}`"
    for entry, owner in shared.items():
        comment = " ".join(_comment_before(src, owner).split())
        at = comment.find(entry)
        assert at >= 0, f"{entry}: the comment of {owner} in include/vitsom_hip.h does not name it"
        assert "16-byte aligned" in comment[at:] or "misaligned" in comment[at:], f"{entry}: no requirement after its name in {owner}'s comment"
    x3 = " ".join(_comment_before(src, "vsom_bmu_cosine_x3_dots").split())
    assert "vsom_bmu_cosine_x3_finalize" in x3 and "VSOM_EALIGN" in x3
    pl = " ".join(_comment_before(src, "vsom_bmu_planes_from").split())
    assert "vsom_bmu_cosine_x3_planes_finalize" in pl and "vsom_bmu_cosine_x3_planes_dots" in pl and "VSOM_EALIGN" in pl


# ------------------------------------------------------------------ the table itself
def test_rows_are_well_formed():
    import torch
    from vit_som_amd import ops
    for r in A.ROWS:
        assert hasattr(ops, r.wrapper), r.id
        c = r.make()
        names = [op.name for op in r.ops]
        assert sorted(names) == sorted(c.t), (r.id, names, list(c.t))
        for op in r.ops:
            v = c.t[op.name]
            assert (isinstance(v, A.Spec)) == (op.role == A.OUT), (r.id, op.name)
            dtype = v.dtype
            assert dtype == op.dtype, (r.id, op.name, dtype)
            shape = v.shape
            assert not op.ld or len(shape) == 2, (r.id, op.name)
            assert (op.pitched is not None) == op.ld, (r.id, op.name)
            if not isinstance(v, A.Spec):
                assert isinstance(v, torch.Tensor) and v.is_contiguous(), (r.id, op.name)
        labels = [v[0] for v in A.variants(r)]
        assert len(labels) == len(set(labels)) and len(labels) >= 2 * len(r.ops), r.id
        refuses = any(isinstance(k, A.REFUSED) for op in r.ops for k in (op.shifted, op.pitched))
        assert ("all+1" in labels) == (not refuses), r.id


def test_shapes_are_those_the_table_promises():
    """Rows: a full tile and a ragged tail; inner extents multiples of 4 but not of 16; LayerNorm at 16, 96, 192; attention at
    hd 16, 64 (refusing) and 8, 3 (not), N 17 and 65; two 64-column tiles and more for kNN, ranks, silhouette."""
    assert (A.LIN_M, A.LIN_N, A.LIN_K) == (130, 70, 52) and A.LIN_K % 4 == 0 and A.LIN_K % 16 != 0
    assert {r.id for r in A.ROWS if r.wrapper == "layernorm_fwd"} == {"layernorm_fwd-16", "layernorm_fwd-96", "layernorm_fwd-192"}
    assert {r.id for r in A.ROWS if r.wrapper == "attention_bwd"} == {f"attention_bwd-N{n}-hd{h}" for n, h in ((17, 16), (65, 64), (17, 8), (65, 3))}
    assert A.KNN_NB > 128 and A.KNN_D % 4 == 0 and A.KNN_D % 16 != 0
    for hd, kind in ((16, A.ALIGN), (64, A.ALIGN), (8, A.SAME), (3, A.SAME)):
        rows = [r for r in A.ROWS if r.id.endswith(f"-hd{hd}")]
        assert len(rows) == 2 and all(op.shifted == kind for r in rows for op in r.ops if op.name in ("qkv", "dqkv")), hd
