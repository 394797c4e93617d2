"""The size-dependent launch regimes of the kernels outside the GEMM family, as data: one entry per regime, at the smallest
shape that selects it, with the sibling just below the threshold.  tests/test_launch_regimes_cpu.py pins every entry to the
host library's size queries and to the constants in the sources; tests/test_launch_regimes_gpu.py runs every entry against
fp64 by its module's own rule and, where an output depends on a row or an element alone, bit for bit against calls that stay
below the threshold.  The expectations are written out from the sources, not derived from the library.

Three patterns were looked for in every .hip file of vit_som_amd/csrc: a capped grid whose workgroups loop, a grid-stride
loop, and an even_split whose last piece can be short.

In the table:
  gmm.hip            E-step groups (GM_MAX_GROUPS x 32 rows), M-step slabs (GM_MAX_SLABS x 32 rows), the reduce pass's 4096 x
                     256 elements.
  kmeans.hip         assign groups (KM_MAX_GROUPS x 32 rows): the loop gmm.hip shares (row_tile.h); the centre pass's 4096 x
                     256 elements (km_shift_blocks).
  tsne.hip           the 64 segments of the step's Z sum.
  linear_probe.hip   row_plan (PROBE_MAX_BLOCKS), vec_plan for the L-BFGS vectors (LB_MAX_BLOCKS) and the fold
                     (FOLD_MAX_BLOCKS), probe_step_kernel's two grid-stride loops (2048 x 256 threads over theta and over Z).
  pca.hip            pca_plan: a short last split, a split count under its cap, a single split, for project and backproject.
  misc.hip           adamw_kernel, fill / scale_by / scaled_mul, l1_loss, l1_unpatchify, contingency.
  bmu_x3.hip         the flat part of planes_kernel<adamw> (vsom_adamw_step_planes).
  layernorm.hip      ln_bwd_blocks (512 x 16 rows), for the 16-byte kernel and for both widths of the element kernel.
  attention.hip      attn_probs_kernel (64 workgroups of 4 query rows per head).
  mapviz.hip         last_label.
  knn.hip            query_plan for vsom_knn_query: a column chunk of more than one 64-column tile, where the top-k lists are
                     carried from tile to tile and `exclude` applies; sil_clear_kernel (4096 x 256 words of the workspace).
  attention_q1.hip   rows_add_kernel (2048 x 256 threads).
  som_l1.hip         l1_splits: the L-chunks of the Manhattan distance pass over at most 16 splits, the last one short.

Looked at and left out:
  kmeans.hip         the colvar pass has a fixed 64 chunks; the counts, shift, relocate and k-means++ kernels are single
                     workgroups (or one per candidate) whose loops turn at every size the existing tests use.
  knn.hip            the SELF instantiation of the same tile loop (umap_knn, knn_ranks, the silhouette) takes several tiles
                     to a chunk at N = 20011 (test_umap_gpu.py) and at N = 4300 (test_silhouette_gpu.py::
                     test_many_column_chunks_equal_the_restatement, test_embedding_quality_gpu.py); no row is added for it.
  pca.hip            cs_plan's row splits (colstats) end in a short piece at nearly every size, those of test_pca_gpu.py's
                     KERNEL_CASES included (257 rows in 3 splits of 86); the PCA rows here run colstats again at their shapes.
  batch_som.hip      long segments (AV_LONG_SEGMENT) and the update's k-tile segments are crossed by test_batch_som_gpu.py.
  umap.hip, augment*.hip, mapquality.hip, som.hip, attention.hip's forward and backward, the attention_q1 kernels, bmu_x3.hip's distance pass,
  layernorm forward, cross entropy, misc.hip's patch and CLS kernels, transpose_many
                     one workgroup (or wave, or thread) per row, image, tile or edge block: the grid grows with the size and
                     no loop's trip count depends on a cap.  The GEMM-shaped passes among them (som.hip, bmu_x3.hip) are in
                     tests/launch_plan_rows.py.
  tsne.hip           the repulsion (one workgroup per 64 rows) and the affinities (one per row) have no cap; the repulsion's
                     column tiles are crossed at N = 3000 and 20011 by test_tsne_gpu.py.
  comm.hip, tape.hip no kernels of their own.
  GEMM family        tests/launch_plan_rows.py.
"""
import re
from collections import namedtuple

GMM_ESTEP = 0                                    # include/vitsom_hip.h: VSOM_GMM_ESTEP


def cdiv(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------------------------- constants in the sources
# file under vit_som_amd/csrc, [(regular expression with one group per integer, the integers as the table assumes them)],
# threshold(values) = the largest size the one-trip regime still takes
Const = namedtuple("Const", "file patterns threshold")

CONSTANTS = {
    "gmm.groups": Const("gmm.hip", [(r"constexpr int GM_MAX_GROUPS = (\d+);", (256,)), (r"constexpr int GM_THREADS = (\d+);", (512,)),
                                    (r"constexpr int GM_RB = (\d+);", (4,))], lambda g, t, rb: g * (t // 64) * rb),
    "gmm.slabs": Const("gmm.hip", [(r"constexpr int GM_MAX_SLABS = (\d+);", (256,)), (r"const long need = \(N \+ 31\) / (\d+);", (32,))],
                       lambda s, rows: s * rows),
    "gmm.reduce": Const("gmm.hip", [(r"if \(blocks > (\d+)\) blocks = (\d+);", (4096, 4096)), (r"constexpr int GM_MT = (\d+);", (256,))],
                        lambda a, b, mt: b * mt),
    "kmeans.groups": Const("kmeans.hip", [(r"constexpr int KM_MAX_GROUPS = (\d+);", (256,)), (r"constexpr int KM_THREADS = (\d+);", (512,)),
                                          (r"constexpr int KM_RB = (\d+);", (4,))], lambda g, t, rb: g * (t // 64) * rb),
    "kmeans.shift": Const("kmeans.hip", [(r"return b < (\d+) \? b : (\d+); \}", (4096, 4096)), (r"constexpr int KM_RED_THREADS = (\d+);", (256,))],
                          lambda a, cap, t: cap * t),
    "tsne.segments": Const("tsne.hip", [(r"const long seg = \(p\.n_z \+ (\d+)\) / (\d+);", (63, 64)), (r"constexpr int REP_ROWS = (\d+);", (64,))],
                           lambda a, segs, rows: segs * rows),
    "probe.rows": Const("linear_probe.hip", [(r"constexpr int PROBE_MAX_BLOCKS = (\d+);", (1024,))], lambda b: b * 16),   # C > 32: 4 slots x 4 rows
    "lbfgs.chunks": Const("linear_probe.hip", [(r"constexpr int LB_MAX_BLOCKS = (\d+);", (512,)), (r"constexpr int LB_CHUNK = (\d+);", (1024,))],
                          lambda b, c: b * c),
    "fold.chunks": Const("linear_probe.hip", [(r"constexpr int FOLD_MAX_BLOCKS = (\d+);", (512,)), (r"constexpr int LB_CHUNK = (\d+);", (1024,))],
                         lambda b, c: b * c),
    "pca.plan": Const("pca.hip", [(r"constexpr int PCA_TARGET_BLOCKS = (\d+);", (768,)), (r"constexpr int PCA_MAX_SPLITS = (\d+);", (64,)),
                                  (r"constexpr int PCA_BM = (\d+), PCA_BN = (\d+);", (128, 64))], None),
    "adamw.flat": Const("misc.hip", [(r"adamw_kernel, dim3\(grid_for\(n4, (\d+), (\d+)\)\)", (256, 8192))], lambda per, cap: per * cap * 4),
    "adamw.planes": Const("bmu_x3.hip", [(r"if \(nflat > (\d+)\) nflat = (\d+);", (8192, 8192)),
                                         (r"long nflat = \(q\.flat_n4 \+ (\d+)\) / (\d+);", (255, 256))], lambda a, cap, b, per: cap * per * 4),
    "fill": Const("misc.hip", [(r"\(fill_kernel, dim3\(grid_for\(n, (\d+), (\d+)\)\)", (1024, 4096))], lambda per, cap: per * cap),
    "scale_by": Const("misc.hip", [(r"\(scale_by_kernel, dim3\(grid_for\(n, (\d+), (\d+)\)\)", (1024, 4096))], lambda per, cap: per * cap),
    "scaled_mul": Const("misc.hip", [(r"\(scaled_mul_kernel, dim3\(grid_for\(n, (\d+), (\d+)\)\)", (1024, 4096))], lambda per, cap: per * cap),
    "l1.blocks": Const("misc.hip", [(r"long b = \(total \+ (\d+)\) / (\d+);\s*if \(b > (\d+)\) b = (\d+);", (1023, 1024, 2048, 2048))],
                       lambda a, per, b, cap: per * cap),
    "ln_bwd.blocks": Const("layernorm.hip", [(r"int b = cdiv\(rows, (\d+)\);\s*if \(b > (\d+)\) b = (\d+);", (16, 512, 512))],
                           lambda rows, a, cap: rows * cap),
    "sil.clear": Const("knn.hip", [(r"\(clear_blocks < (\d+) \? clear_blocks : (\d+)\)", (4096, 4096)),
                                   (r"const size_t clear_blocks = \(w\.clear_words \+ (\d+)\) / (\d+);", (255, 256))], lambda a, cap, b, per: cap * per),
    "knn.query": Const("knn.hip", [(r"constexpr int KNN_TARGET_BLOCKS = (\d+);", (2048,)), (r"constexpr int KNN_BM = (\d+);", (128,)),
                                   (r"constexpr int KNN_BN = (\d+);", (64,))], None),
    "probe.step": Const("linear_probe.hip", [(r"if \(grid > (\d+)\) grid = (\d+);", (2048, 2048)), (r"int grid = cdiv\(most, (\d+)\);", (256,))],
                        lambda a, cap, per: cap * per),
    "rows_add": Const("attention_q1.hip", [(r"\(n \+ 255\) / 256 < (\d+) \? \(n \+ (\d+)\) / (\d+) : (\d+)\)", (2048, 255, 256, 2048))],
                      lambda a, b, per, cap: cap * per),
    "l1.splits": Const("som_l1.hip", [(r"if \(s > (\d+)\) s = (\d+);", (16, 16)), (r"long s = \((\d+) \+ tiles - 1\) / tiles;", (1024,))], None),
    "attn.probs": Const("attention.hip", [(r"const int by = cdiv\(N, (\d+)\) < (\d+) \? cdiv\(N, (\d+)\) : (\d+);", (4, 64, 4, 64))],
                        lambda rows, a, b, cap: rows * cap),
    "contingency": Const("misc.hip", [(r"contingency_kernel, dim3\(vsom::grid_for\(n, (\d+), (\d+)\)\)", (256, 2048))], lambda per, cap: per * cap),
    "last_label": Const("mapviz.hip", [(r"last_label_kernel, dim3\(vsom::grid_1d\(n, (\d+), (\d+)\)\)", (256, 2048))], lambda per, cap: per * cap),
}


def read_constant(key, csrc):
    """The integers of CONSTANTS[key] as the source under `csrc` has them now."""
    import os
    c = CONSTANTS[key]
    src = open(os.path.join(csrc, c.file)).read()
    out = []
    for pattern, _ in c.patterns:
        found = re.findall(pattern, src)
        assert len(found) == 1, f"{c.file}: {pattern!r} matches {len(found)} times"
        out.extend(int(v) for v in (found[0] if isinstance(found[0], tuple) else (found[0],)))
    return tuple(out)


# ---------------------------------------------------------------------------------------------- the plans, restated
def even_split(n, want, granule=1):              # common.h
    per = cdiv(cdiv(n, want), granule) * granule
    return per, cdiv(n, per)


def row_steps(N, max_groups, group=32):
    """gm_groups / km_groups (no slab budget in play) + even_split -> (workgroups, rows of a workgroup, its steps, rows of the last
    workgroup, rows of that workgroup's last step)."""
    per, count = even_split(N, min(cdiv(N, group), max_groups))
    last = N - per * (count - 1)
    return count, per, cdiv(per, group), last, (per - 1) % group + 1


def gmm_slab_rows(N, D, K, max_slabs=256, rows=32, mt=256, budget=128 << 20):
    s = min(budget // (K * (2 * D + 1) * 8), cdiv(1024, cdiv(D, mt)), max_slabs, cdiv(N, rows))
    return even_split(N, max(s, 1))[0]


def probe_row_plan(N, C, max_blocks=1024):
    L = 2
    while L < C and L < 64:
        L <<= 1
    slots = 256 // L
    return even_split(N, max(min(cdiv(N, 4 * slots), max_blocks), 1), slots)        # rows of a block, blocks


def vec_plan(n, max_blocks, chunk=1024):
    chunks = max(cdiv(n, chunk), 1)
    return even_split(chunks, min(chunks, max_blocks))                               # chunks of a block, blocks


def pca_plan(N, D, l, which, target=768, max_splits=64, bm=128, bn=64):
    M, Nc, K = (l, D, N) if which else (N, l, D)
    tiles, ktiles = cdiv(M, bm) * cdiv(Nc, bn), cdiv(K, 32)
    per, splits = even_split(ktiles, max(min(target // tiles, max_splits, ktiles), 1))
    return dict(ktiles=ktiles, per=per, splits=splits, last=ktiles - per * (splits - 1))


def knn_query_plan(Nq, Nb, target=2048, bm=128, bn=64):
    rb, ct = cdiv(Nq, bm), cdiv(Nb, bn)
    chunks = max(min(cdiv(target, rb), ct), 1)
    return dict(rb=rb, ct=ct, chunks=chunks, most_tiles=max((c + 1) * ct // chunks - c * ct // chunks for c in range(chunks)))


def l1_splits(B, K, L, most=16, want=1024):
    tiles, nchunks = cdiv(B, 64) * cdiv(K, 64), cdiv(L, 32)
    per = cdiv(nchunks, max(min(cdiv(want, tiles), most, nchunks), 1))
    return dict(nchunks=nchunks, per=per, splits=cdiv(nchunks, per), last=nchunks - per * (cdiv(nchunks, per) - 1))


def kl_and_grad_torch(Pd, Y, exaggeration, dtype):
    """tsne_ref.kl_and_grad in torch on Pd's device: the fp64 reference of the t-SNE step rows (the dense N x N terms take
    seconds on the host at N = 4097) and, in float32, the plain-fp32 yardstick of test_tsne_gpu._grad_f32.
    test_launch_regimes_cpu.py holds the fp64 form to tsne_ref.kl_and_grad."""
    import torch
    import tsne_ref as R
    P = (Pd * float(exaggeration)).to(dtype)
    Y = Y.to(dtype)
    dx = Y[:, 0:1] - Y[:, 0][None, :]
    dy = Y[:, 1:2] - Y[:, 1][None, :]
    q = 1.0 / (1.0 + (dx * dx + dy * dy))
    q.fill_diagonal_(0.0)
    Z = q.sum()
    pq, q2 = P * q, q * q
    grad = 4.0 * torch.stack([(pq * dx).sum(1) - (q2 * dx).sum(1) / Z, (pq * dy).sum(1) - (q2 * dy).sum(1) / Z], dim=1)
    nz = P > 0
    kl = float((P[nz] * torch.log(P[nz].clamp_min(R.EPS) / (q[nz] / Z).clamp_min(R.EPS))).sum())
    return kl, grad.double().cpu().numpy()


# ---------------------------------------------------------------------------------------------- the table
# regime: the label; pair: the threshold the regime lies at (a "below" and at least one "past" row share it); module, entry;
# shape: the entry's own sizes; side: "below" or "past" the threshold of `const`; size: what is compared with that threshold;
# plan: what the sources give for this shape; query: (size query of the host library, arguments, value) or None where no query
# shows the split; covered_by: an existing test that already crosses the threshold at a workload size
Row = namedtuple("Row", "regime pair module entry shape side size const plan query covered_by", defaults=(None, None, None))


def _estep(regime, side, shape, **plan):
    N, D, K = shape
    return Row(regime, "gmm.estep", "gmm.hip", "vsom_gmm_estep", shape, side, N, "gmm.groups", plan,
               ("vsom_gmm_parts", (N, D, K, GMM_ESTEP), 256 * (2 + 32 * K)))     # sized for the cap: 256 groups on both sides


def _pca(regime, side, entry, shape, pair, **plan):
    N, D, l = shape
    which = int(entry == "vsom_pca_backproject")
    return Row(regime, pair, "pca.hip", entry, shape, side, None, "pca.plan", plan,
               ("vsom_pca_slabs", (N, D, l, which), plan["splits"] * (l * D if which else N * l)))


KMEANS_50000 = "test_kmeans_gpu.py::test_assign_update_against_oracle[50000-3072-10-False]"
KMEANS_200 = "test_kmeans_gpu.py::test_assign_update_against_oracle[1000-12288-200-False]"

ROWS = [
    # ---- gmm_estep_kernel: 256 workgroups of 32 rows; one more row and a workgroup takes a second step
    _estep("gmm.estep.one_step", "below", (8192, 8, 3), groups=256, rows_per=32, steps=1, last_step=32, chunks=1, dtiles=1, vec=4),
    _estep("gmm.estep.resident.vec", "past", (8193, 8, 3), groups=249, rows_per=33, steps=2, last_step=1, chunks=1, dtiles=1, vec=4),
    _estep("gmm.estep.resident.elem", "past", (16500, 7, 3), groups=254, rows_per=65, steps=3, last_step=1, chunks=1, dtiles=1, vec=1),
    _estep("gmm.estep.chunks", "past", (8200, 8, 9), groups=249, rows_per=33, steps=2, last_step=1, chunks=2, dtiles=1, vec=4),
    _estep("gmm.estep.dtiles", "past", (8200, 2100, 3), groups=249, rows_per=33, steps=2, last_step=1, chunks=1, dtiles=2, vec=4),
    # ---- gmm_mstep_kernel: 256 slabs of at least 32 rows
    Row("gmm.mstep.slab=32", "gmm.mstep", "gmm.hip", "vsom_gmm_mstep", (8192, 8, 3), "below", 8192, "gmm.slabs", dict(slab_rows=32),
        ("vsom_gmm_slab_rows", (8192, 8, 3), 32)),
    Row("gmm.mstep.slab>32", "gmm.mstep", "gmm.hip", "vsom_gmm_mstep", (8200, 8, 3), "past", 8200, "gmm.slabs", dict(slab_rows=33),
        ("vsom_gmm_slab_rows", (8200, 8, 3), 33)),
    # ---- gmm_reduce_kernel: 4096 x 256 threads, one element each, then the stride
    Row("gmm.reduce.one_trip", "gmm.reduce", "gmm.hip", "vsom_gmm_params", (64, 4096, 256), "below", 4096 * 256, "gmm.reduce",
        dict(slab_rows=32), ("vsom_gmm_slab_rows", (64, 4096, 256), 32)),
    Row("gmm.reduce.stride", "gmm.reduce", "gmm.hip", "vsom_gmm_params", (64, 4097, 256), "past", 4097 * 256, "gmm.reduce",
        dict(slab_rows=32), ("vsom_gmm_slab_rows", (64, 4097, 256), 32)),
    # ---- kmeans_assign_kernel: the same loop (row_tile.h); 29440 bytes = the sections of 256 groups at D = 8, k = 3
    Row("kmeans.assign.one_step", "kmeans.assign", "kmeans.hip", "vsom_kmeans_assign", (8192, 8, 3), "below", 8192, "kmeans.groups",
        dict(groups=256, rows_per=32, steps=1, last_step=32), ("vsom_kmeans_workspace_bytes", (8192, 8, 3), 29440)),
    Row("kmeans.assign.two_steps", "kmeans.assign", "kmeans.hip", "vsom_kmeans_assign", (8193, 8, 3), "past", 8193, "kmeans.groups",
        dict(groups=249, rows_per=33, steps=2, last_step=1), ("vsom_kmeans_workspace_bytes", (8193, 8, 3), 29440), KMEANS_50000),
    # ---- kmeans_centres_kernel: 4096 x 256 threads, one element of [k][D] each, then the stride (19 assign groups on both sides)
    Row("kmeans.update.one_trip", "kmeans.update", "kmeans.hip", "vsom_kmeans_update", (600, 4096, 256), "below", 256 * 4096, "kmeans.shift",
        None, ("vsom_kmeans_workspace_bytes", (600, 4096, 256), 19 * 256 * 16384 + 19456 + 256 + 256 * 16384 + 32768 + 256)),
    Row("kmeans.update.stride", "kmeans.update", "kmeans.hip", "vsom_kmeans_update", (600, 4096, 257), "past", 257 * 4096, "kmeans.shift",
        None, ("vsom_kmeans_workspace_bytes", (600, 4096, 257), 19 * 257 * 16384 + 19712 + 256 + 257 * 16384 + 32768 + 256), KMEANS_200),
    # ---- tsne_step_kernel: Z from 64 segments of zpart (one entry per 64 rows)
    Row("tsne.step.seg=1", "tsne.step", "tsne.hip", "vsom_tsne_step", (4096,), "below", 4096, "tsne.segments", dict(n_z=64, seg=1),
        ("vsom_tsne_repulsion_parts", (4096,), 64)),
    Row("tsne.step.seg=2", "tsne.step", "tsne.hip", "vsom_tsne_step", (4097,), "past", 4097, "tsne.segments", dict(n_z=65, seg=2),
        ("vsom_tsne_repulsion_parts", (4097,), 65)),
    # ---- linear probe, row_plan: 1024 blocks of 4 slots x 4 rows at C > 32
    Row("probe.rows.4_per_slot", "probe.rows", "linear_probe.hip", "vsom_probe_residual", (16384, 33), "below", 16384, "probe.rows",
        dict(rows_per=16, blocks=1024), ("vsom_probe_parts", (16384, 33), 1024 * 34)),
    Row("probe.rows.5_per_slot", "probe.rows", "linear_probe.hip", "vsom_probe_residual", (16400, 33), "past", 16400, "probe.rows",
        dict(rows_per=20, blocks=820), ("vsom_probe_parts", (16400, 33), 820 * 34)),
    Row("probe.rows.4_per_slot", "probe.rows", "linear_probe.hip", "vsom_probe_linesearch", (16384, 33), "below", 16384, "probe.rows",
        dict(rows_per=16, blocks=1024), ("vsom_probe_parts", (16384, 33), 1024 * 34)),
    Row("probe.rows.5_per_slot", "probe.rows", "linear_probe.hip", "vsom_probe_linesearch", (16400, 33), "past", 16400, "probe.rows",
        dict(rows_per=20, blocks=820), ("vsom_probe_parts", (16400, 33), 820 * 34)),
    # ---- linear probe, vec_plan: 512 blocks of one 1024-element chunk; 513 chunks give 257 blocks of 2, the last with 1
    Row("lbfgs.one_chunk", "lbfgs", "linear_probe.hip", "vsom_lbfgs_dots", (524288, 3), "below", 524288, "lbfgs.chunks",
        dict(chunks_per=1, blocks=512), ("vsom_lbfgs_parts", (524288, 3), 512 * 28)),
    Row("lbfgs.two_chunks", "lbfgs", "linear_probe.hip", "vsom_lbfgs_dots", (525313, 3), "past", 525313, "lbfgs.chunks",
        dict(chunks_per=2, blocks=257), ("vsom_lbfgs_parts", (525313, 3), 257 * 28)),
    Row("fold.one_chunk", "fold", "linear_probe.hip", "vsom_probe_fold", (43, 12192), "below", 43 * 12192, "fold.chunks",
        dict(chunks_per=1, blocks=512), ("vsom_probe_fold_parts", (43, 12192), 3 * 512)),
    Row("fold.two_chunks", "fold", "linear_probe.hip", "vsom_probe_fold", (43, 12288), "past", 43 * 12288, "fold.chunks",
        dict(chunks_per=2, blocks=258), ("vsom_probe_fold_parts", (43, 12288), 3 * 258)),
    # ---- pca_plan: k-tiles of 32 over min(768 / tiles, 64, k-tiles) splits
    _pca("pca.even_split", "below", "vsom_pca_project", (1536, 2048, 10), "pca.project.split", ktiles=64, per=1, splits=64, last=1),
    _pca("pca.short_last_split", "past", "vsom_pca_project", (1537, 2080, 10), "pca.project.split", ktiles=65, per=2, splits=33, last=1),
    _pca("pca.even_split", "below", "vsom_pca_backproject", (1536, 2048, 10), "pca.backproject.split", ktiles=48, per=2, splits=24, last=2),
    _pca("pca.short_last_split", "past", "vsom_pca_backproject", (1537, 2080, 10), "pca.backproject.split", ktiles=49, per=3, splits=17,
         last=1),
    _pca("pca.two_splits", "below", "vsom_pca_project", (49152, 64, 2), "pca.project.tiles", ktiles=2, per=1, splits=2, last=1),
    _pca("pca.single_split", "past", "vsom_pca_project", (49153, 64, 2), "pca.project.tiles", ktiles=2, per=2, splits=1, last=2),
    _pca("pca.single_split", "past", "vsom_pca_project", (49153, 8, 2), "pca.project.tiles", ktiles=1, per=1, splits=1, last=1),
    _pca("pca.splits_under_cap", "past", "vsom_pca_backproject", (49153, 8, 2), "pca.backproject.split", ktiles=1537, per=25, splits=62,
         last=12),
    # ---- grid-stride loops with nothing to query: the cap is read from the launch line
    Row("adamw.one_trip", "adamw.flat", "misc.hip", "vsom_adamw_step", (8388608,), "below", 8388608, "adamw.flat"),
    Row("adamw.stride", "adamw.flat", "misc.hip", "vsom_adamw_step", (8388608 + 768,), "past", 8388608 + 768, "adamw.flat"),
    # the arena outside a [70, 136] slice (9728 elements with its padding) at offset 768
    Row("adamw.one_trip", "adamw.planes", "bmu_x3.hip", "vsom_adamw_step_planes", (8388608 + 9728,), "below", 8388608, "adamw.planes"),
    Row("adamw.stride", "adamw.planes", "bmu_x3.hip", "vsom_adamw_step_planes", (8388608 + 768 + 9728,), "past", 8388608 + 768, "adamw.planes"),
    # fill, scale_by, scaled_mul: 4096 workgroups of 256 threads to 1024 elements, four trips up to the cap
    Row("fill.grid_uncapped", "fill", "misc.hip", "vsom_fill", (4194304,), "below", 4194304, "fill"),
    Row("fill.grid_capped", "fill", "misc.hip", "vsom_fill", (4194304 + 1027,), "past", 4194304 + 1027, "fill"),
    Row("fill.grid_uncapped", "scale_by", "misc.hip", "vsom_scale_by", (4194304,), "below", 4194304, "scale_by"),
    Row("fill.grid_capped", "scale_by", "misc.hip", "vsom_scale_by", (4194304 + 1027,), "past", 4194304 + 1027, "scale_by"),
    Row("fill.grid_uncapped", "scaled_mul", "misc.hip", "vsom_scaled_mul", (4194304,), "below", 4194304, "scaled_mul"),
    Row("fill.grid_capped", "scaled_mul", "misc.hip", "vsom_scaled_mul", (4194304 + 1027,), "past", 4194304 + 1027, "scaled_mul"),
    # ---- l1_blocks: 2048 workgroups of 256 threads to 1024 elements: four trips of the stride loop up to the cap, more past it
    # (both sides hold 2048 partials: 8192 bytes)
    Row("l1.grid_uncapped", "l1_loss", "misc.hip", "vsom_l1_loss", (2097152,), "below", 2097152, "l1.blocks", None,
        ("vsom_l1_loss_workspace_bytes", (2097152,), 8192)),
    Row("l1.grid_capped", "l1_loss", "misc.hip", "vsom_l1_loss", (2097152 + 1027,), "past", 2097152 + 1027, "l1.blocks", None,
        ("vsom_l1_loss_workspace_bytes", (2097152 + 1027,), 8192)),
    # (B, C, S, p): B x 65 tokens x 48 values
    Row("l1.grid_uncapped", "l1_unpatchify", "misc.hip", "vsom_l1_unpatchify", (672, 3, 32, 4), "below", 672 * 65 * 48, "l1.blocks", None,
        ("vsom_l1_unpatchify_workspace_bytes", (672, 3, 32, 4), 8192)),
    Row("l1.grid_capped", "l1_unpatchify", "misc.hip", "vsom_l1_unpatchify", (673, 3, 32, 4), "past", 673 * 65 * 48, "l1.blocks", None,
        ("vsom_l1_unpatchify_workspace_bytes", (673, 3, 32, 4), 8192)),
    # ---- ln_bwd_blocks: 512 workgroups of 16 rows; the partials are [512][2][cols] floats on both sides
    Row("ln_bwd.one_trip", "ln_bwd.16", "layernorm.hip", "vsom_layernorm_bwd", (8192, 16), "below", 8192, "ln_bwd.blocks", None,
        ("vsom_layernorm_bwd_workspace_bytes", (8192, 16), 512 * 2 * 16 * 4)),
    Row("ln_bwd.stride", "ln_bwd.16", "layernorm.hip", "vsom_layernorm_bwd", (8193 + 16, 16), "past", 8193 + 16, "ln_bwd.blocks", None,
        ("vsom_layernorm_bwd_workspace_bytes", (8193 + 16, 16), 512 * 2 * 16 * 4)),
    Row("ln_bwd.one_trip", "ln_bwd.192", "layernorm.hip", "vsom_layernorm_bwd", (8192, 192), "below", 8192, "ln_bwd.blocks", None,
        ("vsom_layernorm_bwd_workspace_bytes", (8192, 192), 512 * 2 * 192 * 4)),
    Row("ln_bwd.stride", "ln_bwd.192", "layernorm.hip", "vsom_layernorm_bwd", (8200, 192), "past", 8200, "ln_bwd.blocks", None,
        ("vsom_layernorm_bwd_workspace_bytes", (8200, 192), 512 * 2 * 192 * 4)),
    # ---- sil_clear_kernel: the words of S u64 [N][C], acc [C + 1] and ctrl (sections 256-aligned) over 4096 x 256 threads;
    # (N, n_clusters, D); the workspace adds sq f32 [N]
    Row("sil.clear.one_trip", "sil.clear", "knn.hip", "vsom_silhouette", (4300, 243, 8), "below", (8359424 + 2048 + 256) // 8, "sil.clear", None,
        ("vsom_silhouette_workspace_bytes", (4300, 243), 8359424 + 2048 + 256 + 17408)),
    Row("sil.clear.stride", "sil.clear", "knn.hip", "vsom_silhouette", (4300, 244, 8), "past", (8393728 + 2048 + 256) // 8, "sil.clear", None,
        ("vsom_silhouette_workspace_bytes", (4300, 244), 8393728 + 2048 + 256 + 17408)),
    # ---- vsom_knn_query, (Nq, Nb, D, k): chunks = min(ceil(2048 / row blocks), column tiles); 44 row blocks leave 47 chunks of
    # one tile, 45 leave 46 chunks, one of them with two tiles.  The workspace is sized by min(ct rb, 2047 + rb) row blocks
    Row("knn.query.one_tile", "knn.query", "knn.hip", "vsom_knn_query", (5632, 3000, 8, 10), "below", None, "knn.query",
        dict(rb=44, ct=47, chunks=47, most_tiles=1), ("vsom_knn_query_workspace_bytes", (5632, 3000, 10), 22528 + 12032 + 2 * 2068 * 5120)),
    Row("knn.query.two_tiles", "knn.query", "knn.hip", "vsom_knn_query", (5633, 3000, 8, 10), "past", None, "knn.query",
        dict(rb=45, ct=47, chunks=46, most_tiles=2), ("vsom_knn_query_workspace_bytes", (5633, 3000, 10), 22784 + 12032 + 2 * 2092 * 5120)),
    # ---- probe_step_kernel, (N, C, D): 2048 x 256 threads stride over the n = C D + C entries of theta and over the N C of Z
    Row("probe.step.one_trip", "probe.step", "linear_probe.hip", "vsom_probe_step", (16384, 32, 7), "below", 16384 * 32, "probe.step"),
    Row("probe.step.stride.z", "probe.step", "linear_probe.hip", "vsom_probe_step", (16400, 33, 7), "past", 16400 * 33, "probe.step"),
    Row("probe.step.stride.theta", "probe.step", "linear_probe.hip", "vsom_probe_step", (300, 43, 12288), "past", 43 * 12289, "probe.step"),
    # ---- rows_add_kernel, (rows, cols)
    Row("rows_add.one_trip", "rows_add", "attention_q1.hip", "vsom_rows_add", (2048, 256), "below", 2048 * 256, "rows_add"),
    Row("rows_add.stride", "rows_add", "attention_q1.hip", "vsom_rows_add", (2049, 256), "past", 2049 * 256, "rows_add"),
    # ---- l1_dist_kernel, (B, K, L): 24 chunks of 32 columns are 12 splits of 2; 25 are 12 of 2 and one of 1
    Row("l1.splits.even", "l1.splits", "som_l1.hip", "vsom_bmu_manhattan_fwd", (33, 12, 768), "below", None, "l1.splits",
        dict(nchunks=24, per=2, splits=12, last=2), ("vsom_bmu_manhattan_workspace_bytes", (33, 12, 768), 12 * 33 * 12 * 4)),
    Row("l1.splits.short_last", "l1.splits", "som_l1.hip", "vsom_bmu_manhattan_fwd", (33, 12, 784), "past", None, "l1.splits",
        dict(nchunks=25, per=2, splits=13, last=1), ("vsom_bmu_manhattan_workspace_bytes", (33, 12, 784), 13 * 33 * 12 * 4)),
    # ---- layernorm_bwd_kernel<4> (cols not a multiple of 4) and <16> (cols > 256): the same 512 x 16 rows
    Row("ln_bwd.one_trip", "ln_bwd.18", "layernorm.hip", "vsom_layernorm_bwd", (8192, 18), "below", 8192, "ln_bwd.blocks", None,
        ("vsom_layernorm_bwd_workspace_bytes", (8192, 18), 512 * 2 * 18 * 4)),
    Row("ln_bwd.stride", "ln_bwd.18", "layernorm.hip", "vsom_layernorm_bwd", (8200, 18), "past", 8200, "ln_bwd.blocks", None,
        ("vsom_layernorm_bwd_workspace_bytes", (8200, 18), 512 * 2 * 18 * 4)),
    Row("ln_bwd.one_trip", "ln_bwd.260", "layernorm.hip", "vsom_layernorm_bwd", (8192, 260), "below", 8192, "ln_bwd.blocks", None,
        ("vsom_layernorm_bwd_workspace_bytes", (8192, 260), 512 * 2 * 260 * 4)),
    Row("ln_bwd.stride", "ln_bwd.260", "layernorm.hip", "vsom_layernorm_bwd", (8200, 260), "past", 8200, "ln_bwd.blocks", None,
        ("vsom_layernorm_bwd_workspace_bytes", (8200, 260), 512 * 2 * 260 * 4)),
    # ---- attn_probs_kernel, (B, N, H, hd): 64 workgroups of 4 query rows to a head, then the stride
    Row("attn.probs.one_trip", "attn.probs", "attention.hip", "vsom_attention_probs", (1, 256, 2, 16), "below", 256, "attn.probs"),
    Row("attn.probs.stride", "attn.probs", "attention.hip", "vsom_attention_probs", (1, 257, 2, 16), "past", 257, "attn.probs"),
    # ---- integer atomics behind a grid-stride loop
    Row("pairs.one_trip", "contingency", "misc.hip", "vsom_contingency", (524288,), "below", 524288, "contingency"),
    Row("pairs.stride", "contingency", "misc.hip", "vsom_contingency", (524288 + 300,), "past", 524288 + 300, "contingency"),
    Row("pairs.one_trip", "last_label", "mapviz.hip", "vsom_last_label", (524288,), "below", 524288, "last_label"),
    Row("pairs.stride", "last_label", "mapviz.hip", "vsom_last_label", (524288 + 300,), "past", 524288 + 300, "last_label", None, None,
        "test_mapviz_gpu.py::test_last_label_against_the_reference_loop"),
]

# every regime of the table; test_launch_regimes_cpu.py asserts that ROWS hits each one
REGIMES = {
    "gmm.estep.one_step", "gmm.estep.resident.vec", "gmm.estep.resident.elem", "gmm.estep.chunks", "gmm.estep.dtiles",
    "gmm.mstep.slab=32", "gmm.mstep.slab>32", "gmm.reduce.one_trip", "gmm.reduce.stride",
    "kmeans.assign.one_step", "kmeans.assign.two_steps", "kmeans.update.one_trip", "kmeans.update.stride", "tsne.step.seg=1", "tsne.step.seg=2",
    "probe.rows.4_per_slot", "probe.rows.5_per_slot", "lbfgs.one_chunk", "lbfgs.two_chunks", "fold.one_chunk", "fold.two_chunks",
    "pca.even_split", "pca.short_last_split", "pca.two_splits", "pca.single_split", "pca.splits_under_cap",
    "adamw.one_trip", "adamw.stride", "fill.grid_uncapped", "fill.grid_capped", "l1.grid_uncapped", "l1.grid_capped", "ln_bwd.one_trip", "ln_bwd.stride",
    "pairs.one_trip", "pairs.stride", "sil.clear.one_trip", "sil.clear.stride", "knn.query.one_tile", "knn.query.two_tiles",
    "probe.step.one_trip", "probe.step.stride.z", "probe.step.stride.theta", "rows_add.one_trip", "rows_add.stride",
    "l1.splits.even", "l1.splits.short_last", "attn.probs.one_trip", "attn.probs.stride",
}

# what a workgroup's loop carries from one step to the next: a refused row in a second step must be counted and must leave
# every other row alone.  (shape of an E-step row above, the two bad rows): row 197 is the one-row second step of workgroup 5
# and 3332 that of workgroup 100; 235 lies in the second step of workgroup 3 (rows 195..259) and 16482 in the second step of
# the last workgroup (rows 16445..16499)
ESTEP_BAD_ROWS = [((8193, 8, 3), (197, 3332)), ((16500, 7, 3), (235, 16482))]

SLICE_ROWS = 8192                                # k-means and GMM: the rows of a call that stays in the one-step regime
MIN_SHARE = 0.9                                  # a check that leaves rows out keeps at least this share of them


def rows_of(entry):
    return [r for r in ROWS if r.entry == entry]


def row_id(r):
    return f"{r.entry[5:]}-{'x'.join(map(str, r.shape))}"
