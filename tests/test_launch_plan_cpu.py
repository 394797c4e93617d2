"""Which kernel runs ("Which kernel runs"), pinned on the host: vsom_describe_plan must report, for every entry
of PLAN_ROWS, the engine, tile, plane count and load path the table gives -- in all three GEMM modes and every setting of
the family's hook.  Pure host code: no GPU needed."""
import ctypes
import re

import pytest

from launch_plan_rows import ATTENTION_BWD, F32, GRAD3, HOOK_DEFAULTS, HOOK_VALUES, MODES, PLAN_ROWS, TABLE_ROWS, UNSUPPORTED

LINE = re.compile(r"engine=(\S+) tile=(\d+x\d+) planes=(\d+) fast=([01]) threads=(\d+) splits=(\d+) workgroups=(\d+)$")


def describe(lib, op, shape, aligned):
    """(engine, tile, planes, fast, threads, splits, workgroups), or None where the entry point refuses the shape."""
    buf = ctypes.create_string_buffer(160)
    rc = lib.vsom_describe_plan(op, *shape, int(aligned), buf, len(buf))
    if rc == -3:
        return None
    assert rc == 0, (rc, op, shape)
    m = LINE.match(buf.value.decode())
    assert m, buf.value
    return (m.group(1), m.group(2)) + tuple(int(g) for g in m.groups()[2:])


@pytest.fixture(scope="module")
def ops():
    from vit_som_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def lib():
    from vit_som_amd._lib import lib as _lib
    return _lib


def test_plan_rows_cover_the_table():
    assert {r.row for r in PLAN_ROWS} == TABLE_ROWS


@pytest.mark.parametrize("row", PLAN_ROWS, ids=lambda r: f"{r.row}-op{r.op}-{'x'.join(map(str, r.shape))}")
def test_describe_plan_matches_the_table(ops, lib, row):
    prev = ops.get_gemm_mode()
    setter = getattr(ops, "set_" + row.hook) if row.hook else None
    try:
        for mode in MODES:
            ops.set_gemm_mode(mode)
            for hook in (HOOK_VALUES[row.hook] if row.hook else (None,)):
                if setter:
                    setter(hook)
                want = row.expect[mode]
                if isinstance(want, dict):
                    want = want[hook]
                got = describe(lib, row.op, row.shape, row.aligned)
                if want is UNSUPPORTED:
                    assert got is None, (mode, hook, got)
                else:
                    assert got is not None and got[:4] == want, (mode, hook, got, want)
    finally:
        ops.set_gemm_mode(prev)
        if setter:
            setter(HOOK_DEFAULTS[row.hook])


def attention_bwd_plan(N, hd, hook, mode):
    """(engine, waves) of the attention backward, restated from DESIGN.md's table and LDS layout (not from the C++)."""
    extra = N >= 17 and N % 16 == 1
    nt = (N - 1) // 16 if extra else -(-N // 16)
    nrows = N if extra else 16 * nt
    nrp = (nrows + 3) & ~3
    waves = 8 if nt >= 8 else min(nt, 4)
    hdp = hd if hd in (16, 32, 64) else (4 if hd <= 4 else 8)
    fused = 4 * (4 * nrows * (hdp + 4) + 2 * nrp + 3 * hdp * waves)
    shared = fused + 8 * hdp
    vec = hdp % 16 == 0
    if (vec and hook in (1, 3) and nt <= 4 and waves == nt and 16 * nt * (16 * nt + 4) <= nrows * (hdp + 4)
            and shared <= 81920):
        return ("attn_shared_bf16x3" if hdp == 64 and mode == GRAD3 and hook == 1 else "attn_shared"), waves
    if vec and hook != 0 and fused <= 81920:
        return "attn_fused", waves
    return "attn_two_launch", waves


def test_attention_backward_plan_over_the_whole_range(ops, lib):
    """Engine and workgroup size for every N = 1..320, head dim, hook and GEMM mode: pins attn_bwd_plan and the LDS
    byte counts it rests on, where PLAN_ROWS pins single shapes."""
    prev = ops.get_gemm_mode()
    bad = []
    try:
        for mode in MODES:
            ops.set_gemm_mode(mode)
            for hook in HOOK_VALUES["attention_fused"]:
                ops.set_attention_fused(hook)
                for hd in (2, 4, 8, 16, 32, 64):
                    for N in range(1, 321):
                        engine, waves = attention_bwd_plan(N, hd, hook, mode)
                        got = describe(lib, ATTENTION_BWD, (N, 2, hd), 1)
                        if got is None or (got[0], got[4]) != (engine, 64 * waves):
                            bad.append((mode, hook, hd, N, got, engine, 64 * waves))
    finally:
        ops.set_gemm_mode(prev)
        ops.set_attention_fused(HOOK_DEFAULTS["attention_fused"])
    assert not bad, (len(bad), bad[:8])


def bmu_cosine_form(B, K, L, ldx, flags, mode):
    """0 exact, 1 in-loop three-product, 2 planes: the "Cosine BMU pass" table of DESIGN.md restated (not from the C++)."""
    aligned, planes = bool(flags & 1), bool(flags & 2)
    x3 = mode != F32 and K <= 256 * 8 and L % 4 == 0 and ldx % 4 == 0 and aligned
    if not x3:
        return 0

    def image(R):                       # bytes of an operand's fragment image: 2 planes of 32 x 32 bf16 blocks
        return 2 * -(-L // 32) * -(-R // 32) * 2048
    if planes and B >= 192 and L % 8 == 0 and image(B) < 2 ** 31 and image(K) < 2 ** 31:
        return 2
    return 1


def test_bmu_cosine_form_over_the_whole_range(ops, lib):
    """vsom_bmu_cosine_form against the table on both sides of every clause: the batch threshold of the big tile and the
    planes, the prototype limit, L % 4 and L % 8, the row stride, both flags, the three modes, and the 2 GiB image bound
    (1365 resp. 1366 row blocks of 384 x 2 x 2048 = 1 572 864 bytes)."""
    prev = ops.get_gemm_mode()
    bad = []
    try:
        for mode in MODES:
            ops.set_gemm_mode(mode)
            shapes = [(B, K, L) for B in (1, 64, 191, 192, 193, 512) for K in (1, 15, 2048, 2049)
                      for L in (4, 8, 12, 250, 252, 256, 12288)] + [(43680, 16, 12288), (43681, 16, 12288)]
            for B, K, L in shapes:
                for ldx in (L, L + 1, L + 4):
                    for flags in range(4):
                        got, want = lib.vsom_bmu_cosine_form(B, K, L, ldx, flags), bmu_cosine_form(B, K, L, ldx, flags, mode)
                        if got != want:
                            bad.append((mode, B, K, L, ldx, flags, got, want))
            if mode != F32:
                assert lib.vsom_bmu_cosine_form(43680, 16, 12288, 12288, 3) == 2
                assert lib.vsom_bmu_cosine_form(43681, 16, 12288, 12288, 3) == 1
    finally:
        ops.set_gemm_mode(prev)
    assert not bad, (len(bad), bad[:8])
    assert lib.vsom_bmu_cosine_form(0, 16, 8, 8, 3) == -1


def test_describe_plan_grid_arithmetic(lib):
    """Workgroups = tiles x splits, the split count canonical (every split owns a k-tile of 32)."""
    got = describe(lib, 0, (300, 200, 64), 1)                       # 3 x 4 tiles of 128 x 64, one split
    assert got[5:] == (1, 12)
    got = describe(lib, 12, (512, 1600, 12288), 1)                  # BMU dots: 4 x 25 tiles, split over L
    assert got[6] == 100 * got[5] and -(-384 // -(-384 // got[5])) == got[5]
    got = describe(lib, 8, (70, 12, 24), 1)                         # generic dW: 3 k-tiles bound the splits
    assert got[5] <= 3 and got[6] == got[5]
    got = describe(lib, 14, (512, 1600, 12288), 3)                  # BMU planes: 2 x 9 tiles of 256 x 192, 256 // 18 = 14 splits
    assert got[4:] == (512, 14, 252)                                # ... of 28 k-tiles each


def test_describe_plan_rejects_bad_calls(lib):
    buf = ctypes.create_string_buffer(160)
    assert lib.vsom_describe_plan(99, 8, 8, 8, 1, buf, len(buf)) == -1
    assert lib.vsom_describe_plan(0, 0, 8, 8, 1, buf, len(buf)) == -1
    assert lib.vsom_describe_plan(0, 8, 8, 8, 1, buf, 8) == -1          # line does not fit
    assert lib.vsom_describe_plan(0, 8, 8, 8, 1, None, 0) == -1
    assert lib.vsom_describe_plan(13, 17, 2, 24, 1, buf, len(buf)) == -3   # head dim 24
