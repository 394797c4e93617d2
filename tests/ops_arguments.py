"""The argument contract of the evaluation wrappers of vit_som_amd/ops.py (from the `evaluation` banner to the RCCL
section), as a table: for every wrapper one valid call at the smallest shapes that satisfy its own relations, and for
every tensor argument its kind.  test_ops_arguments_cpu.py and test_ops_arguments_gpu.py read it.

Kinds (the three checks of ops.py): MATRIX, a float32 row matrix with any row stride; DENSE, a contiguous tensor of an exact
shape; BUFFER, a contiguous tensor of at least so many elements.  Per argument further:

  optional   None is a valid value (the wrapper's docstring says so); `together` names the arguments that must be None with it;
  sized      the wrapper knows how large the argument has to be, so one row or one element less is refused.  False for
             an argument that sets a size itself (X sets N and D: a row less is another valid call) and for a buffer
             whose element count goes to the entry, which sizes it by a query of its own and refuses a short one before
             it launches (the k-means and UMAP workspaces, zpart, part, the ragged scratch).  A sized BUFFER is built at
             exactly its minimum here;
  dtype      None: any dtype passes (the k-means workspace).

Nothing here computes: every tensor is zeros, which is also what the two wrappers that look at values before the launch
need (knn_ranks' index range, som_batch_accumulate's sort)."""
import ctypes
import math
from dataclasses import dataclass, field

import torch

from vit_som_amd import _lib, ops

MATRIX, DENSE, BUFFER = "matrix", "dense", "buffer"
F32, F64, I32, I64, U8 = torch.float32, torch.float64, torch.int32, torch.int64, torch.uint8
WRONG = {F32: F64, F64: F32, I64: I32, I32: I64, U8: I32}          # the dtype each is mistaken for


@dataclass
class Arg:
    kind: str
    dtype: object = F32
    optional: bool = False
    sized: bool = True
    together: tuple = ()


def mat(**kw):
    return Arg(MATRIX, F32, **kw)


def dense(dtype=F32, **kw):
    return Arg(DENSE, dtype, **kw)


def buf(dtype, **kw):
    return Arg(BUFFER, dtype, **kw)


@dataclass
class Row:
    name: str                      # the wrapper, with a suffix in brackets for a second form of its call
    entry: str                     # the C entry the valid call reaches, once
    make: object                   # make(device) -> the keyword arguments of the valid call
    args: dict                     # tensor argument -> Arg
    reads_back: bool = False       # reads a status word after the launch: under the stub nobody wrote it
    fn: object = field(init=False)

    def __post_init__(self):
        self.fn = getattr(ops, self.name.split("[")[0])


class StubLib:
    """Stands in for ops.lib: an entry that returns a status (c_int) is recorded and answered with 0 without being
    called; the size queries (c_size_t / c_long) go to the real library."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        restype, _ = _lib.SIGNATURES[name]
        if restype is not ctypes.c_int:
            return getattr(_lib.lib, name)

        def entry(*args):
            self.calls.append(name)
            return 0
        return entry


# Wrappers of the range that take no tensor whose address reaches the library: host arithmetic and allocators.
EXEMPT = {"augment_ragged_scratch_bytes", "kmeans_workspace_bytes", "umap_neg_sample", "umap_transform_workspace",
          "umap_transform_state", "silhouette_workspace", "pca_slabs", "probe_parts", "lbfgs_state", "tsne_repulsion_parts",
          "tsne_step_parts", "gmm_parts", "gmm_slab_rows", "gmm_scratch"}

N, D, K, C, NQ, KNN = 7, 5, 3, 3, 4, 3       # rows, columns, clusters / units, classes, queries, neighbours
B, CH, S = 2, 3, 8                           # the data pipeline: batch, channels, side
M_, NV = 2, 6                                # L-BFGS: memory, vector length
NNZ = 6


def _z(dev):
    return lambda dtype, *shape: torch.zeros(*shape, dtype=dtype, device=dev)


def _crop():
    return dict(scale=(0.08, 1.0), log_ratio=(math.log(0.75), math.log(4 / 3)), scale2=None, log_ratio2=None, flip_p=0.5,
                erase_p=0.0, seed=1, epoch=0)


def _batch(z):
    return dict(index=z(I64, B), out=z(F32, B, CH, S, S), mean=z(F32, CH), std=z(F32, CH), seed=1, epoch=0, out_u8=z(U8, B, CH, S, S))


_BATCH = dict(index=dense(I64, sized=False), out=buf(F32), mean=dense(), std=dense(), out_u8=buf(U8, optional=True))
_STATE = int(_lib.lib.vsom_lbfgs_state_doubles(M_))
_DOTS = 3 * (2 * M_ + 3) + 1
_WS = dict(ws=buf(None, sized=False))


def _rows():
    r = []

    def row(name, entry, make, reads_back=False, **args):
        r.append(Row(name, entry, make, args, reads_back))

    # ---- evaluation counters, mosaic, map statistics, U-matrix
    row("contingency", "vsom_contingency",
        lambda d, z=_z: dict(a=z(d)(I64, N), b=z(d)(I64, N), table=z(d)(I64, K, 2), bad=z(d)(I32, 1)),
        a=buf(I64, sized=False), b=dense(I64), table=dense(I64, sized=False), bad=dense(I32))
    row("argmax_rows", "vsom_argmax_rows", lambda d, z=_z: dict(x=z(d)(F32, N, D), out=z(d)(I64, N)),
        x=mat(sized=False), out=dense(I64))
    row("proto_mosaic", "vsom_proto_mosaic",
        lambda d, z=_z: dict(pred=z(d)(F32, 2 * 5, 2 * 2 * CH), n=4, p=2, C=CH, k0=0, map_size=(1, 2), images=z(d)(F32, 2, CH, 4, 4),
                             canvas=z(d)(U8, 4, 9, 3), gap=1),
        pred=dense(), images=dense(optional=True), canvas=dense(U8, optional=True))
    row("last_label", "vsom_last_label",
        lambda d, z=_z: dict(bmu=z(d)(I64, N), label=z(d)(I64, N), first_ordinal=0, cells=z(d)(I64, K), bad=z(d)(I32, 1)),
        bmu=buf(I64, sized=False), label=dense(I64), cells=buf(I64, sized=False), bad=dense(I32))
    row("map_stats", "vsom_map_stats",
        lambda d, z=_z: dict(dist=z(d)(F32, N, K), bmu=z(d)(I64, N), grid_positions=z(d)(F32, K, 2), adj_r2=1.0, first_ordinal=0,
                             hits=z(d)(I64, K), qe_fix=z(d)(I64, K), te=z(d)(I64, 1), nearest=z(d)(I64, K), bad=z(d)(I32, 1),
                             second=z(d)(I64, N)),
        dist=dense(sized=False), bmu=dense(I64), grid_positions=dense(), hits=dense(I64), qe_fix=dense(I64), te=dense(I64),
        nearest=dense(I64), bad=dense(I32), second=dense(I64, optional=True))
    row("umatrix", "vsom_umatrix", lambda d, z=_z: dict(W=z(d)(F32, K, D), grid_positions=z(d)(F32, K, 2), adj_r2=1.0, distance=0),
        reads_back=True, W=dense(sized=False), grid_positions=dense())

    # ---- both data pipelines
    row("augment_plan", "vsom_augment_plan",
        lambda d, z=_z: dict(index=z(d)(I64, B), params=z(d)(I32, B, ops.AUGMENT_PARAMS), N=4, H=S, S=S, **_crop()),
        index=dense(I64, sized=False), params=buf(I32))
    row("augment_batch", "vsom_augment_batch",
        lambda d, z=_z: dict(src=z(d)(U8, 4, CH, S, S), params=z(d)(I32, B, ops.AUGMENT_PARAMS), S=S, R=S, off=0, **_batch(z(d))),
        src=dense(U8, sized=False), params=buf(I32, optional=True), **_BATCH)
    row("randaug_plan", "vsom_randaug_plan",
        lambda d, z=_z: dict(index=z(d)(I64, B), ra=z(d)(I32, B, ops.RANDAUG_PARAMS), N=4, S=S, randaug_n=2, autoaugment=False,
                             flip1_p=0.5, fill_tv=(0, 0, 0), fill_timm=(1, 2, 3), seed=1, epoch=0),
        index=dense(I64, sized=False), ra=buf(I32))
    row("augment_batch_ra", "vsom_augment_batch_ra",
        lambda d, z=_z: dict(src=z(d)(U8, 4, CH, S, S), params=z(d)(I32, B, ops.AUGMENT_PARAMS), ra=z(d)(I32, B, ops.RANDAUG_PARAMS),
                             S=S, **_batch(z(d))),
        src=dense(U8, sized=False), params=buf(I32), ra=buf(I32), **_BATCH)
    row("augment_plan_ragged", "vsom_augment_plan_ragged",
        lambda d, z=_z: dict(index=z(d)(I64, B), shapes=z(d)(I32, 4, 2), params=z(d)(I32, B, ops.AUGMENT_PARAMS), S=S, **_crop()),
        index=dense(I64, sized=False), shapes=dense(I32, sized=False), params=buf(I32))
    row("augment_batch_ragged", "vsom_augment_batch_ragged",
        lambda d, z=_z: dict(data=z(d)(U8, 100), offsets=z(d)(I64, 4), shapes=z(d)(I32, 4, 2), C=CH, max_h=S, max_w=S,
                             params=z(d)(I32, B, ops.AUGMENT_PARAMS), S=S, R=S, scratch=z(d)(U8, 64), **_batch(z(d))),
        data=dense(U8, sized=False), offsets=dense(I64, sized=False), shapes=dense(I32), params=buf(I32, optional=True),
        scratch=buf(U8, sized=False), **_BATCH)          # with params the scratch is needed

    # ---- k-means
    row("kmeans_assign", "vsom_kmeans_assign",
        lambda d, z=_z: dict(X=z(d)(F32, N, D), centers=z(d)(F32, K, D), labels=z(d)(I64, N), prev_labels=z(d)(I64, N),
                             mind=z(d)(F32, N), ws=z(d)(U8, 64)),
        X=mat(sized=False), centers=dense(sized=False), labels=dense(I64), prev_labels=dense(I64), mind=dense(), **_WS)
    row("kmeans_update", "vsom_kmeans_update",
        lambda d, z=_z: dict(centers_old=z(d)(F32, K, D), centers_new=z(d)(F32, K, D), N=N, mind=z(d)(F32, N), counts=z(d)(I64, K),
                             status=z(d)(F64, 4), ws=z(d)(U8, 64)),
        centers_old=dense(sized=False), centers_new=dense(), mind=dense(), counts=dense(I64), status=dense(F64), **_WS)
    row("kmeans_relocate", "vsom_kmeans_relocate",
        lambda d, z=_z: dict(X=z(d)(F32, N, D), labels=z(d)(I64, N), moves=z(d)(I64, 1, 2), centers_old=z(d)(F32, K, D),
                             centers_new=z(d)(F32, K, D), counts=z(d)(I64, K), status=z(d)(F64, 4), ws=z(d)(U8, 64)),
        X=mat(sized=False), labels=dense(I64), moves=dense(I64, sized=False), centers_old=dense(sized=False), centers_new=dense(),
        counts=dense(I64), status=dense(F64), **_WS)
    row("kmeanspp_dist", "vsom_kmeanspp_dist",
        lambda d, z=_z: dict(X=z(d)(F32, N, D), candidates=z(d)(I64, 2), closest=z(d)(F32, N), dist=z(d)(F32, 2, N), pots=z(d)(F64, 2)),
        X=mat(sized=False), candidates=buf(I64, sized=False), closest=dense(optional=True), dist=dense(), pots=buf(F64))
    row("kmeans_colvar", "vsom_kmeans_colvar", lambda d, z=_z: dict(X=z(d)(F32, N, D), k=K, out=z(d)(F64, 1), ws=z(d)(U8, 64)),
        X=mat(sized=False), out=dense(F64), **_WS)

    # ---- UMAP
    row("umap_knn", "vsom_umap_knn",
        lambda d, z=_z: dict(X=z(d)(F32, N, D), k=KNN, metric=0, knn_idx=z(d)(I64, N, KNN), knn_dist=z(d)(F32, N, KNN)),
        X=mat(sized=False), knn_idx=dense(I64), knn_dist=dense())
    row("umap_epoch", "vsom_umap_epoch",
        lambda d, z=_z: dict(indptr=z(d)(I64, N + 1), indices=z(d)(I64, NNZ), eps=z(d)(F64, NNZ), next_s=z(d)(F64, NNZ),
                             eps_neg=z(d)(F64, NNZ), next_neg=z(d)(F64, NNZ), Y_in=z(d)(F32, N, 2), Y_out=z(d)(F32, N, 2), a=1.0, b=1.0,
                             gamma=1.0, alpha=1.0, epoch=0, seed=1),
        indptr=dense(I64), indices=buf(I64, sized=False), eps=dense(F64), next_s=dense(F64), eps_neg=dense(F64), next_neg=dense(F64),
        Y_in=dense(sized=False), Y_out=dense())
    row("umap_transform_layout", "vsom_umap_transform_layout",
        lambda d, z=_z: dict(knn_idx=z(d)(I64, NQ, KNN), weights=z(d)(F64, NQ, KNN), eps=z(d)(F64, NQ, KNN), Y_train=z(d)(F32, N, 2),
                             Y=z(d)(F32, NQ, 2), a=1.0, b=1.0, gamma=1.0, initial_alpha=0.25, n_epochs=10, epoch_begin=0, epoch_end=10,
                             negative_sample_rate=5, seed=1, status=z(d)(I32, 1), ws=z(d)(U8, 1024)),
        knn_idx=dense(I64, sized=False), weights=dense(F64), eps=dense(F64), Y_train=dense(sized=False), Y=dense(), status=dense(I32),
        ws=buf(U8, sized=False))

    # ---- kNN, ranks, silhouette, vote
    row("knn_query", "vsom_knn_query",
        lambda d, z=_z: dict(Q=z(d)(F32, NQ, D), X=z(d)(F32, N, D), k=KNN, metric=0, idx=z(d)(I64, NQ, KNN), dist=z(d)(F32, NQ, KNN),
                             exclude=z(d)(I64, NQ)),
        Q=mat(sized=False), X=mat(sized=False), idx=dense(I64), dist=dense(), exclude=dense(I64, optional=True))
    row("knn_ranks", "vsom_knn_ranks",
        lambda d, z=_z: dict(A=z(d)(F32, N, D), nbr=z(d)(I64, N, KNN), metric=0, less=z(d)(I32, N, KNN), tied=z(d)(I32, N, KNN)),
        A=mat(sized=False), nbr=dense(I64), less=dense(I32), tied=dense(I32))
    row("silhouette", "vsom_silhouette",
        lambda d, z=_z: dict(X=z(d)(F32, N, D), labels=z(d)(I64, N), metric=0, n_clusters=K,
                             ws=z(d)(U8, int(_lib.lib.vsom_silhouette_workspace_bytes(N, K)))),
        reads_back=True, X=mat(sized=False), labels=dense(I64), ws=buf(U8, optional=True))
    row("knn_vote", "vsom_knn_vote",
        lambda d, z=_z: dict(idx=z(d)(I64, NQ, KNN), dist=z(d)(F32, NQ, KNN), bank_labels=z(d)(I64, N), n_classes=C, weights=0,
                             temperature=0.07, pred=z(d)(I64, NQ), status=z(d)(I32, 2), scores=z(d)(F64, NQ, C)),
        idx=dense(I64, sized=False), dist=dense(), bank_labels=buf(I64, sized=False), pred=dense(I64), status=dense(I32),
        scores=dense(F64, optional=True))

    # ---- PCA
    row("pca_colstats", "vsom_pca_colstats", lambda d, z=_z: dict(X=z(d)(F32, N, D), mean=z(d)(F32, D), var=z(d)(F64, D)),
        X=mat(sized=False), mean=dense(optional=True), var=dense(F64, optional=True))
    row("pca_project", "vsom_pca_project",
        lambda d, z=_z: dict(X=z(d)(F32, N, D), mean=z(d)(F32, D), B=z(d)(F32, K, D), scale=z(d)(F32, K), Y=z(d)(F32, N, K)),
        X=mat(sized=False), mean=dense(optional=True), B=mat(sized=False), scale=dense(optional=True), Y=mat())
    row("pca_backproject", "vsom_pca_backproject",
        lambda d, z=_z: dict(Y=z(d)(F32, N, K), X=z(d)(F32, N, D), mean=z(d)(F32, D), Zt=z(d)(F32, K, D)),
        Y=mat(), X=mat(sized=False), mean=dense(optional=True), Zt=mat())
    row("pca_gram", "vsom_pca_gram",
        lambda d, z=_z: dict(Zt=z(d)(F32, K, D), G=z(d)(F64, K, K), B=z(d)(F32, K, D), H=z(d)(F64, K, K)),
        Zt=mat(sized=False), G=dense(F64), B=mat(optional=True, together=("H",)), H=dense(F64, optional=True, together=("B",)))
    row("pca_rotate", "vsom_pca_rotate", lambda d, z=_z: dict(T=z(d)(F64, 2, K), Zt=z(d)(F32, K, D), Bout=z(d)(F32, 2, D)),
        T=dense(F64, sized=False), Zt=mat(sized=False), Bout=mat())
    row("pca_reconstruct", "vsom_pca_reconstruct",
        lambda d, z=_z: dict(Y=z(d)(F32, NQ, K), scale=z(d)(F32, K), B=z(d)(F32, K, D), mean=z(d)(F32, D), Xout=z(d)(F32, NQ, D)),
        Y=mat(sized=False), scale=dense(optional=True), B=mat(), mean=dense(optional=True), Xout=mat())

    # ---- batch SOM
    def accumulate(d, z=_z):
        return dict(X=z(d)(F32, N, D), bmu=z(d)(I64, N), sums=z(d)(F64, K, D), counts=z(d)(I64, K), inv_norm=z(d)(F32, N))

    acc = dict(X=mat(sized=False), bmu=dense(I64), sums=dense(F64), counts=dense(I64, sized=False), inv_norm=dense(optional=True))
    row("som_batch_accumulate", "vsom_som_batch_accumulate", lambda d, z=_z: dict(bad=z(d)(I32, 1), **accumulate(d)),
        bad=dense(I32, optional=True), **acc)
    row("som_batch_accumulate[bad=None]", "vsom_som_batch_accumulate", accumulate, reads_back=True, **acc)
    row("som_batch_update", "vsom_som_batch_update",
        lambda d, z=_z: dict(sums=z(d)(F64, K, D), counts=z(d)(I64, K), grid_positions=z(d)(F32, K, 2), sigma=1.0, W_out=z(d)(F32, K, D)),
        sums=dense(F64), counts=dense(I64, sized=False), grid_positions=dense(), W_out=mat())

    # ---- linear probe and L-BFGS
    nt = C * D + C
    row("probe_fold", "vsom_probe_fold",
        lambda d, z=_z: dict(A=z(d)(F64, C, D), invstd=z(d)(F64, D), B=z(d)(F32, C, D), W=z(d)(F64, C, D), pen=z(d)(F64, 3)),
        A=dense(F64, sized=False), invstd=dense(F64), B=mat(), W=dense(F64, optional=True, together=("pen",)),
        pen=dense(F64, optional=True, together=("W",)))
    row("probe_residual", "vsom_probe_residual",
        lambda d, z=_z: dict(Z=z(d)(F32, N, C), b=z(d)(F64, C), y=z(d)(I64, N), R=z(d)(F32, N, C), loss=z(d)(F64, 1), gb=z(d)(F64, C),
                             status=z(d)(I32, 1), pred=z(d)(I64, N), prob=z(d)(F64, N, C)),
        Z=mat(sized=False), b=dense(F64, optional=True), y=dense(I64), R=mat(), loss=dense(F64), gb=dense(F64), status=dense(I32),
        pred=dense(I64, optional=True), prob=dense(F64, optional=True))
    row("probe_linesearch", "vsom_probe_linesearch",
        lambda d, z=_z: dict(Z=z(d)(F32, N, C), Zp=z(d)(F32, N, C), b=z(d)(F64, C), pb=z(d)(F64, C), y=z(d)(I64, N), alpha0=z(d)(F64, 1),
                             nsteps=4, phi=z(d)(F64, 4)),
        Z=mat(sized=False), Zp=mat(), b=dense(F64, optional=True, together=("pb",)), pb=dense(F64, optional=True, together=("b",)),
        y=dense(I64), alpha0=dense(F64), phi=dense(F64))
    row("probe_step", "vsom_probe_step",
        lambda d, z=_z: dict(phi=z(d)(F64, 4), alpha0=z(d)(F64, 1), f0=z(d)(F64, 1), pen=z(d)(F64, 3), gtp=z(d)(F64, 1), lam=0.1, c1=1e-4,
                             Z=z(d)(F32, N, C), Zp=z(d)(F32, N, C), theta=z(d)(F64, nt), p=z(d)(F64, nt), s_new=z(d)(F64, nt),
                             rec=z(d)(F64, ops.LBFGS_RECORD)),
        phi=buf(F64, sized=False), alpha0=dense(F64), f0=dense(F64), pen=dense(F64), gtp=dense(F64), Z=mat(sized=False), Zp=mat(),
        theta=buf(F64, sized=False), p=dense(F64), s_new=dense(F64), rec=buf(F64))
    row("probe_gradient", "vsom_probe_gradient",            # theta holds an intercept: gb is needed
        lambda d, z=_z: dict(Zt=z(d)(F32, C, D), invstd=z(d)(F64, D), theta=z(d)(F64, nt), gb=z(d)(F64, C), N=N, lam=0.1, g=z(d)(F64, nt),
                             g_prev=z(d)(F64, nt), y_new=z(d)(F64, nt)),
        Zt=mat(sized=False), invstd=dense(F64), theta=buf(F64), gb=dense(F64), g=dense(F64),
        g_prev=dense(F64, optional=True, together=("y_new",)), y_new=dense(F64, optional=True, together=("g_prev",)))

    def lbfgs(d, z=_z):
        return dict(S=z(d)(F64, M_, NV), Y=z(d)(F64, M_, NV), g=z(d)(F64, NV), s_new=z(d)(F64, NV), y_new=z(d)(F64, NV),
                    state=z(d)(F64, _STATE))

    row("lbfgs_dots", "vsom_lbfgs_dots", lambda d, z=_z: dict(dots=z(d)(F64, _DOTS), **lbfgs(d)),
        S=dense(F64, sized=False), Y=dense(F64), g=dense(F64), s_new=dense(F64, optional=True, together=("y_new",)),
        y_new=dense(F64, optional=True, together=("s_new",)), state=dense(F64), dots=dense(F64))
    row("lbfgs_coeff", "vsom_lbfgs_coeff", lambda d, z=_z: dict(dots=z(d)(F64, _DOTS), m=M_, has_new=False, state=z(d)(F64, _STATE)),
        dots=dense(F64), state=dense(F64))
    row("lbfgs_combine", "vsom_lbfgs_combine", lambda d, z=_z: dict(p=z(d)(F64, NV), **lbfgs(d)),
        S=dense(F64, sized=False), Y=dense(F64), g=dense(F64), s_new=dense(F64), y_new=dense(F64), state=dense(F64), p=dense(F64))

    # ---- t-SNE
    row("tsne_affinities", "vsom_tsne_affinities",
        lambda d, z=_z: dict(knn_dist=z(d)(F32, N, KNN + 1), perplexity=2.0, P=z(d)(F64, N, KNN), beta=z(d)(F64, N), status=z(d)(I32, 1),
                             knn_idx=z(d)(I64, N, KNN + 1), first=1, square=True),
        knn_dist=mat(sized=False), P=dense(F64), beta=dense(F64), status=dense(I32), knn_idx=dense(I64, optional=True))
    row("tsne_repulsion", "vsom_tsne_repulsion",
        lambda d, z=_z: dict(Y=z(d)(F32, N, 2), rep=z(d)(F64, N, 2), sumq=z(d)(F64, N), zpart=z(d)(F64, 1)),
        Y=dense(sized=False), rep=dense(F64), sumq=dense(F64), zpart=buf(F64, sized=False))
    row("tsne_step", "vsom_tsne_step",
        lambda d, z=_z: dict(indptr=z(d)(I64, N + 1), indices=z(d)(I64, NNZ), data=z(d)(F64, NNZ), Y_in=z(d)(F32, N, 2), Y_out=z(d)(F32, N, 2),
                             update=z(d)(F32, N, 2), gains=z(d)(F32, N, 2), rep=z(d)(F64, N, 2), zpart=z(d)(F64, 1), exaggeration=12.0,
                             momentum=0.5, learning_rate=200.0, part=z(d)(F64, 2), record=False),
        indptr=dense(I64), indices=buf(I64, sized=False), data=dense(F64), Y_in=dense(sized=False), Y_out=dense(), update=dense(),
        gains=dense(), rep=dense(F64), zpart=buf(F64, sized=False), part=buf(F64, sized=False))

    # ---- Gaussian mixtures
    row("gmm_estep", "vsom_gmm_estep",
        lambda d, z=_z: dict(X=z(d)(F32, N, D), means=z(d)(F32, K, D), prec=z(d)(F32, K, D), logc=z(d)(F64, K), resp=z(d)(F32, N, K),
                             log_prob_norm=z(d)(F64, N), labels=z(d)(I64, N), estat=z(d)(F64, 2), part=z(d)(F64, 64)),
        X=mat(sized=False), means=dense(sized=False), prec=dense(), logc=dense(F64), resp=mat(optional=True), log_prob_norm=dense(F64),
        labels=dense(I64, optional=True), estat=dense(F64), part=buf(F64, optional=True, sized=False))
    row("gmm_mstep", "vsom_gmm_mstep",
        lambda d, z=_z: dict(X=z(d)(F32, N, D), resp=z(d)(F32, N, K), means_old=z(d)(F32, K, D), part=z(d)(F64, 64)),
        X=mat(sized=False), resp=mat(), means_old=dense(sized=False), part=buf(F64, sized=False))
    row("gmm_params", "vsom_gmm_params",
        lambda d, z=_z: dict(part=z(d)(F64, 64), N=N, means_old=z(d)(F32, K, D), reg_covar=1e-6, spherical=False, n_norm=0, estat=z(d)(F64, 2),
                             means=z(d)(F32, K, D), cov=z(d)(F64, K, D), prec=z(d)(F32, K, D), weights=z(d)(F64, K), logc=z(d)(F64, K),
                             record=z(d)(F64, ops.GMM_RECORD)),
        part=buf(F64, sized=False), means_old=dense(sized=False), estat=dense(F64, optional=True), means=dense(), cov=dense(F64),
        prec=dense(), weights=dense(F64), logc=dense(F64), record=dense(F64))
    row("gmm_set_params", "vsom_gmm_set_params",
        lambda d, z=_z: dict(weights=z(d)(F64, K), cov=z(d)(F64, K, D), D=D, spherical=False, prec=z(d)(F32, K, D), logc=z(d)(F64, K),
                             record=z(d)(F64, ops.GMM_RECORD), part=z(d)(F64, 64)),
        weights=dense(F64, sized=False), cov=dense(F64), prec=dense(), logc=dense(F64), record=dense(F64),
        part=buf(F64, optional=True, sized=False))
    return r


ROWS = _rows()


def in_scope_range(source):
    """(first, last) line numbers of the range of ops.py the table covers."""
    lines = source.split("\n")
    first = next(i for i, text in enumerate(lines, 1) if text.startswith("# ----") and text.endswith(" evaluation"))
    last = next(i for i, text in enumerate(lines, 1) if text.startswith("# ----") and "data-parallel exchange (RCCL)" in text)
    return first, last
