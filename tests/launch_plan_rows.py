"""The launch-plan table of DESIGN.md ("Which kernel runs") as data: one entry per row, at the smallest shape that selects
it.  tests/test_launch_plan_cpu.py pins vsom_describe_plan to these expectations; tests/test_launch_plan_gpu.py runs every
entry through its ops wrapper.  The expectations are written out from the table, not derived from the library."""
from collections import namedtuple

# include/vitsom_hip.h: VSOM_PLAN_*
(LINEAR_FWD, LINEAR_GELU_FWD, LINEAR_RELU_FWD, LINEAR_RESIDUAL_FWD, BWD_INPUT, BWD_INPUT_GELU, BWD_INPUT_T, BWD_INPUT_T_GELU,
 BWD_WEIGHT, BWD_INPUT_LN, SOM_BWD_GW, SOM_BWD_GX, BMU_COSINE_DOTS, ATTENTION_BWD, BMU_COSINE) = range(15)

F32, SPLIT, GRAD3 = 0, 1, 2                     # VSOM_GEMM_*
MODES = (F32, SPLIT, GRAD3)

# (engine, tile, planes, fast)
F32_128 = ("f32", "128x64", 0, 1)
F32_128_SLOW = ("f32", "128x64", 0, 0)
F32_64 = ("f32", "64x64", 0, 1)
F32_64_SLOW = ("f32", "64x64", 0, 0)
X6_64 = ("x6", "64x64", 3, 1)
X6_128 = ("x6", "128x64", 3, 1)
X6_128_P2 = ("x6", "128x64", 2, 1)
UNSUPPORTED = None                              # vsom_describe_plan returns VSOM_EUNSUPPORTED


def tn(tile, planes):
    return ("x6_tn", tile, planes, 1)


def ln(tile, planes):
    return ("x6_ln", tile, planes, 1)


TWO_LAUNCH, FUSED, SHARED = (("attn_" + n, "16x16", 0, 1) for n in ("two_launch", "fused", "shared"))
SHARED_BF16X3 = ("attn_shared_bf16x3", "16x16", 2, 1)
BMU_X3_SMALL, BMU_X3_BIG = ("bmu_x3", "128x128", 2, 1), ("bmu_x3", "256x192", 2, 1)
BMU_X3_PLANES = ("bmu_x3_planes", "256x192", 2, 1)

# row: label of the table row; op, shape: vsom_describe_plan's arguments (the entry point's own M, N, K); aligned: the
# flags (bit 0: aligned operands; bit 1, BMU_COSINE only: plane images are available); expect[gemm mode] = the outcome, or {hook value: outcome} where the family's hook matters (hook = "wgrad_tiles",
# "ln_tiles" or "attention_fused"); ld_pad: extra floats on the first operand's row stride in the GPU run
Row = namedtuple("Row", "row op shape aligned expect hook ld_pad", defaults=(None, 0))


def every(outcome):
    return {m: outcome for m in MODES}


def by_mode(f32, split, grad3):
    return {F32: f32, SPLIT: split, GRAD3: grad3}


PLAN_ROWS = [
    # ---- NT (both k-contiguous)
    Row("nt.slab", BMU_COSINE_DOTS, (70, 15, 256), 1, every(F32_128)),
    Row("nt.m<=64", LINEAR_FWD, (33, 10, 24), 1, by_mode(F32_128, X6_64, X6_64)),
    Row("nt.m<=64", LINEAR_GELU_FWD, (64, 16, 8), 1, by_mode(F32_128, X6_64, X6_64)),
    Row("nt.m<=64.p3", BWD_INPUT_T, (33, 24, 10), 1, by_mode(F32_128, X6_64, X6_64)),
    Row("nt.p3", BWD_INPUT_T, (70, 48, 50), 1, by_mode(F32_128, X6_128, X6_128_P2)),
    Row("nt.p3", BWD_INPUT_T_GELU, (65, 48, 50), 1, by_mode(F32_128, X6_128, X6_128_P2)),
    Row("nt.x6", LINEAR_FWD, (70, 50, 48), 1, by_mode(F32_128, X6_128, X6_128)),
    Row("nt.x6", LINEAR_GELU_FWD, (70, 50, 48), 1, by_mode(F32_128, X6_128, X6_128)),
    Row("nt.x6", LINEAR_RELU_FWD, (70, 50, 48), 1, by_mode(F32_128, X6_128, X6_128)),
    Row("nt.x6", LINEAR_RESIDUAL_FWD, (70, 50, 48), 1, by_mode(F32_128, X6_128, X6_128)),
    Row("nt.slow", LINEAR_FWD, (128, 128, 33), 1, every(F32_128_SLOW), ld_pad=3),          # K % 4 on a row stride of 36
    Row("nt.slow", LINEAR_FWD, (70, 50, 48), 0, every(F32_128_SLOW), ld_pad=1),            # row stride 49: unaligned
    # ---- A k-contiguous, B k-strided
    Row("nn.rowaxpy", SOM_BWD_GX, (70, 16, 48), 1, by_mode(F32_128, X6_128, X6_128_P2)),
    Row("nn.rowaxpy.slow", SOM_BWD_GX, (70, 15, 48), 1, every(F32_128_SLOW)),
    Row("nn.other", BWD_INPUT, (33, 10, 24), 1, every(F32_128_SLOW)),                      # N = 10 along k: K % 4
    Row("nn.other", BWD_INPUT, (70, 12, 8), 1, every(F32_128)),
    Row("nn.other", BWD_INPUT_GELU, (70, 12, 8), 1, every(F32_128)),
    # ---- both k-strided: the SOM's gW and the generic weight gradient
    Row("tn.64", SOM_BWD_GW, (70, 144, 48), 1, by_mode(F32_64, X6_64, X6_64)),             # 144 rows: 256 > 1.1 * 192
    Row("tn.128.p3", SOM_BWD_GW, (70, 256, 48), 1, by_mode(F32_128, X6_128, X6_128_P2)),
    Row("tn.64.slow", BWD_WEIGHT, (70, 10, 24), 1, every(F32_64_SLOW)),                    # 10 rows along the vector: N % 4
    Row("tn.64", BWD_WEIGHT, (70, 12, 24), 1, by_mode(F32_64, X6_64, X6_64)),
    Row("tn.128", BWD_WEIGHT, (70, 128, 24), 1, by_mode(F32_128, X6_128, X6_128)),         # slab epilogue: never two planes
    # ---- weight-gradient tiles
    Row("wgrad.192x64", BWD_WEIGHT, (256, 192, 64), 1, by_mode(F32_64, tn("192x64", 3), tn("192x64", 2))),
    Row("wgrad.96x96", BWD_WEIGHT, (256, 96, 96), 1, by_mode(F32_128, tn("96x96", 3), tn("96x96", 2))),
    Row("wgrad.192x192", BWD_WEIGHT, (256, 192, 192), 1,
        by_mode(F32_64, tn("192x64", 3), {0: tn("192x64", 2), 1: tn("192x192", 2), 2: tn("192x192", 2)}), "wgrad_tiles"),
    Row("wgrad.unaligned", BWD_WEIGHT, (256, 192, 64), 0, every(F32_64_SLOW), ld_pad=1),
    # ---- LayerNorm-fused input gradient: supported iff split engine, K in {192, 96}, >= 32 row tiles
    Row("ln.192", BWD_INPUT_LN, (2048, 64, 192), 1,
        by_mode(UNSUPPORTED, ln("64x192", 3), {0: ln("64x192", 2), 1: ln("192x192", 2)}), "ln_tiles"),
    Row("ln.96", BWD_INPUT_LN, (4096, 64, 96), 1, by_mode(UNSUPPORTED, ln("128x96", 3), ln("128x96", 2))),
    Row("ln.few_tiles", BWD_INPUT_LN, (2048 - 64, 64, 192), 1, every(UNSUPPORTED)),
    Row("ln.width", BWD_INPUT_LN, (4096, 64, 128), 1, every(UNSUPPORTED)),
    # ---- attention backward: shape = (N tokens, H, hd)
    Row("attn.shared", ATTENTION_BWD, (65, 2, 64), 1,
        by_mode({0: TWO_LAUNCH, 1: SHARED, 2: FUSED, 3: SHARED}, {0: TWO_LAUNCH, 1: SHARED, 2: FUSED, 3: SHARED},
                {0: TWO_LAUNCH, 1: SHARED_BF16X3, 2: FUSED, 3: SHARED}), "attention_fused"),
    Row("attn.shared.hd32", ATTENTION_BWD, (33, 2, 32), 1, every({0: TWO_LAUNCH, 1: SHARED, 2: FUSED, 3: SHARED}), "attention_fused"),
    # 64 (64 + 4) score floats > 65 (32 + 4) floats of LDS left by K / V
    Row("attn.fused", ATTENTION_BWD, (65, 2, 32), 1, every({0: TWO_LAUNCH, 1: FUSED, 2: FUSED, 3: FUSED}), "attention_fused"),
    Row("attn.two_launch.lds", ATTENTION_BWD, (197, 2, 64), 1, every({h: TWO_LAUNCH for h in range(4)}), "attention_fused"),
    Row("attn.two_launch.novec", ATTENTION_BWD, (17, 2, 8), 1, every({h: TWO_LAUNCH for h in range(4)}), "attention_fused"),
    # ---- cosine BMU pass: shape = (B, K, L); in VSOM_GEMM_F32 mode every row is the exact form
    Row("bmu.x3.small", BMU_COSINE, (70, 15, 256), 1, by_mode(F32_128, BMU_X3_SMALL, BMU_X3_SMALL)),
    Row("bmu.x3.big", BMU_COSINE, (192, 15, 256), 1, by_mode(F32_128, BMU_X3_BIG, BMU_X3_BIG)),
    Row("bmu.x3.planes", BMU_COSINE, (192, 15, 256), 3, by_mode(F32_128, BMU_X3_PLANES, BMU_X3_PLANES)),
    Row("bmu.x3.l%8", BMU_COSINE, (192, 15, 252), 3, by_mode(F32_128, BMU_X3_BIG, BMU_X3_BIG)),
    Row("bmu.exact.k", BMU_COSINE, (8, 2049, 8), 3, every(F32_128)),                        # 2049 > 256 * 8 prototypes
    Row("bmu.exact.stride", BMU_COSINE, (70, 15, 256), 0, every(F32_128_SLOW), ld_pad=1),   # row stride 257: unaligned
]

# every row of the table; test_launch_plan_cpu.py asserts that PLAN_ROWS hits each one
TABLE_ROWS = {
    "nt.slab", "nt.m<=64", "nt.m<=64.p3", "nt.p3", "nt.x6", "nt.slow",
    "nn.rowaxpy", "nn.rowaxpy.slow", "nn.other",
    "tn.64", "tn.64.slow", "tn.128", "tn.128.p3",
    "wgrad.192x64", "wgrad.96x96", "wgrad.192x192", "wgrad.unaligned",
    "ln.192", "ln.96", "ln.few_tiles", "ln.width",
    "attn.shared", "attn.shared.hd32", "attn.fused", "attn.two_launch.lds", "attn.two_launch.novec",
    "bmu.x3.small", "bmu.x3.big", "bmu.x3.planes", "bmu.x3.l%8", "bmu.exact.k", "bmu.exact.stride",
}

HOOK_VALUES = {"wgrad_tiles": (0, 1, 2), "ln_tiles": (0, 1), "attention_fused": (0, 1, 2, 3)}
HOOK_DEFAULTS = {"wgrad_tiles": 2, "ln_tiles": 1, "attention_fused": 1}
