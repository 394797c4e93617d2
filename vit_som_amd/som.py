"""SOMLayer (models/som_layer.py:8-152) on the HIP kernels, with the autograd functions of its distances and loss."""
from dataclasses import dataclass
from typing import Dict, Optional

import numpy as np
import torch
import torch.nn as nn

from . import ops
from ._base import _Acts, _Base
from ._lib import Event, on_stream
from .tuning import hooks


class _SomDistancesFn(torch.autograd.Function):
    """SOMLayer.forward under autograd (som_layer.py:83-89, 111-125): distances differentiable w.r.t. the input rows
    and the prototypes; the BMU indices are returned alongside (non-differentiable, argmin)."""

    @staticmethod
    def forward(ctx, x, W, layer):
        with torch.no_grad():
            s = layer._buffers_for(x.shape[0], x.device)
            layer._distances_into(x, s)
            dist, bmu = s.dist.clone(), s.bmu.clone()
            ctx.save_for_backward(x, W, dist, s.inx.clone(), s.inw.clone())
        ctx.mode = layer._dist_mode
        ctx.mark_non_differentiable(bmu)
        return dist, bmu

    @staticmethod
    def backward(ctx, g_dist, _g_bmu):
        x, W, dist, inx, inw = ctx.saved_tensors
        B, K = dist.shape
        with torch.no_grad():
            f = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dist.device)   # noqa: E731
            coef, row_dot, col_dot, tmp = f(B, K), f(B), f(K), f(1)
            # backward coefficients of sum(g * dist): the upstream gradient plays the role of the weights
            ops.som_weighted_loss(dist, g_dist.float().contiguous(), tmp, inv_nx=inx, inv_nw=inw, grad_scale=1.0, coef=coef,
                                  row_dot=row_dot, col_dot=col_dot, distance=ctx.mode)
            gW, gX = torch.empty_like(W), torch.empty_like(x)
            if ctx.mode == ops.DIST_MANHATTAN:
                ops.som_bwd_manhattan(x, W, coef, gW, gX, accumulate_gx=False)
            else:
                ops.som_bwd(x, W, coef, row_dot, col_dot, gW, gX, accumulate_gx=False)
        return gX, gW, None


class _SomLossFn(torch.autograd.Function):
    """mean(weights * distances) (som_layer.py:137-142) with gradients to both arguments."""

    @staticmethod
    def forward(ctx, weights, distances):
        ctx.save_for_backward(weights, distances)
        tmp = torch.empty(1, dtype=torch.float32, device=distances.device)
        ops.som_weighted_loss(distances, weights, tmp)
        out = torch.empty((), dtype=torch.float32, device=distances.device)
        ops.scaled_mul(out.view(1), tmp, factor=1.0 / distances.numel())
        return out

    @staticmethod
    def backward(ctx, gout):
        weights, distances = ctx.saved_tensors
        g = gout.detach().reshape(1).float().contiguous()
        inv = 1.0 / distances.numel()
        gw = ops.scaled_mul(torch.empty_like(weights), distances, scale_dev=g, factor=inv) if ctx.needs_input_grad[0] else None
        gd = ops.scaled_mul(torch.empty_like(distances), weights, scale_dev=g, factor=inv) if ctx.needs_input_grad[1] else None
        return gw, gd


@dataclass
class BatchSOMReport:
    """Host values of one SOMLayer.fit_batch run over T epochs (bmu stays on the device)."""
    sigma: np.ndarray                    # float64 [T]: the radius of every epoch
    quantization_error: np.ndarray       # float64 [T]: mean BMU distance (the layer's distance) BEFORE each update
    final_quantization_error: float      # the same after the last update
    moved: np.ndarray                    # int64 [T]: rows whose BMU differs from the previous epoch's (all rows in the first)
    hits: np.ndarray                     # int64 [K]: rows per unit in the final search
    dead_units: int                      # units no row hit in the final search
    bmu: torch.Tensor                    # int64 [N] on the device: the final search


# ------------------------------------------------------------------------------------ SOM layer
class SOMLayer(_Base):
    """models/som_layer.py:8-152 on the HIP kernels (cosine / euclidean / manhattan distance; square /
    hexa topology; clients: ViTSOM and DESOM)."""

    def __init__(self, config):
        super().__init__()
        hp = config["hyperparameters"]
        self.model_arch = hp["model_arch"]
        som_hp, data_hp = hp["som"], config["data"]
        vit_hp = hp["vit"] if self.model_arch == "vit_som" else None
        self.total_epochs, self.batch_size = hp["total_epochs"], hp["batch_size"]
        self.map_size = som_hp["map_size"]
        self.Tmax, self.Tmin = som_hp["Tmax"], som_hp["Tmin"]
        self.topology, self.distance_fcn = som_hp["topology"], som_hp["distance_fcn"]
        self.n_prototypes = int(np.prod(self.map_size))
        modes = {"cosine": ops.DIST_COSINE, "euclidean": ops.DIST_EUCLIDEAN, "manhattan": ops.DIST_MANHATTAN}
        if self.distance_fcn not in modes:                              # som_layer.py:111-125 raises the same way
            raise ValueError(f"Unsupported distance function: {self.distance_fcn}")
        self._dist_mode = modes[self.distance_fcn]
        if self.model_arch == "vit_som":                                       # som_layer.py:35-40
            self.use_reduced = som_hp["use_reduced"]
            latent_dim = vit_hp["emb_dim"]
            if not self.use_reduced:
                latent_dim *= (data_hp["input_size"] // vit_hp["patch_size"]) ** 2
        else:                                                                  # DESOM: the autoencoder's code
            self.use_reduced = False
            latent_dim = hp["ae"]["encoder_dims"][-1]
        self.latent_dim = latent_dim
        self.current_temperature = self.Tmax
        proto = torch.rand(self.n_prototypes, latent_dim)                      # som_layer.py:44-56
        if self.distance_fcn == "cosine":
            proto = torch.nn.functional.normalize(proto, p=2, dim=1)
        self.prototypes = nn.Parameter(proto)
        self.create_grid_positions()
        self._world_size = 1
        self._n_train: Optional[int] = None
        self._bufs: Dict[int, _Acts] = {}
        # pre-split plane image of the prototypes for the BMU contraction (ops.bmu_planes_*): valid while its stamp
        # equals _w_stamp().  FusedAdamW rewrites it in the pass that updates the prototypes; anything else that
        # changes them is seen through torch's version counter, the storage address or _raw_updates.
        self._wplanes: Optional[torch.Tensor] = None
        self._wplanes_stamp = None
        self._raw_updates = 0           # updates of the prototypes that bypass torch (raw-pointer kernels)
        self._planes_used = False       # a forward took the planes path: the optimizer keeps the image current
        self._planes_rows = 0           # ... with this many sample rows
        self._w_ready_ev = None         # the event of _w_planes_async (a dedicated one: its wait comes a whole encoder later)

    # ---- plane image of the prototypes ---------------------------------------------------
    def _w_stamp(self):
        W = self.prototypes
        return (W.data_ptr(), W._version, self._raw_updates, tuple(W.shape))

    def invalidate_planes(self):
        """Call after changing the prototypes behind torch's back (writes through ``.data`` or a raw pointer)."""
        self._wplanes_stamp = None

    def _bmu_form(self, B: int, ldx: Optional[int] = None, aligned: bool = True) -> int:
        """Which form of the cosine BMU pass runs for B sample rows of stride `ldx` floats (default: dense rows): ops.BMU_EXACT,
        BMU_X3 or BMU_X3_PLANES.  The rule is the library's launch plan ("Which kernel runs"); this is the one place
        of the package that asks it."""
        K, L = self.prototypes.shape
        return ops.lib.vsom_bmu_cosine_form(B, K, L, L if ldx is None else ldx, int(aligned) | (2 if hooks.bmu_planes else 0))

    def _planes_shape_ok(self, B: int) -> bool:
        """Would a batch of B dense, aligned rows take the planes form?"""
        return self._dist_mode == ops.DIST_COSINE and self.prototypes.is_cuda and self._bmu_form(B) == ops.BMU_X3_PLANES

    def _w_planes_buffer(self) -> torch.Tensor:
        """The prototypes' plane buffer, allocated here (and nowhere else) when there is none or it is on another device or of
        another size.  A new buffer describes nothing yet."""
        W = self.prototypes
        if self._wplanes is None or self._wplanes.device != W.device or self._wplanes.numel() != ops.lib.vsom_bmu_planes_bytes(*W.shape):
            self._wplanes = ops.bmu_planes_alloc(W.shape[0], W.shape[1], W.device)
            self._wplanes_stamp = None
        return self._wplanes

    def _w_planes(self) -> torch.Tensor:
        """The prototypes' plane buffer, re-split here if it does not describe them any more."""
        planes = self._w_planes_buffer()
        if self._wplanes_stamp != self._w_stamp():
            ops.bmu_planes_from(self.prototypes.detach(), planes)
            self._wplanes_stamp = self._w_stamp()
        return planes

    def _w_planes_async(self, side_stream, force: bool):
        """Bring the prototypes' image up to date on `side_stream`, behind everything the launch stream holds so far
        (the optimizer step that wrote the prototypes, the last contraction that read the image) -- when it is stale,
        or always with `force` (a recorded training step must contain the launch whatever the state it was recorded
        in).  Returns the event the consumer has to wait for, or None when nothing was launched.  The event is the layer's
        own: the consumer waits a whole encoder later, by which time a pooled event could have been recorded again."""
        planes = self._w_planes_buffer()
        if not force and self._wplanes_stamp == self._w_stamp():
            return None
        Event.pooled().record().wait(side_stream)
        with on_stream(side_stream):
            ops.bmu_planes_from(self.prototypes.detach(), planes)
        self._wplanes_stamp = self._w_stamp()
        if self._w_ready_ev is None:
            self._w_ready_ev = Event()
        return self._w_ready_ev.record(side_stream)

    def _load_from_state_dict(self, *args, **kwargs):
        super()._load_from_state_dict(*args, **kwargs)
        self.invalidate_planes()

    def create_grid_positions(self):                                   # som_layer.py:60-81
        if self.topology == "square":
            gy, gx = torch.meshgrid(torch.arange(self.map_size[0]), torch.arange(self.map_size[1]), indexing="ij")
            positions = torch.stack([gy, gx], dim=-1).view(-1, 2).float()
        elif self.topology == "hexa":
            rows, cols = self.map_size
            positions = torch.zeros(self.n_prototypes, 2)
            for i in range(self.n_prototypes):
                row, col = i // cols, i % cols
                positions[i, 0] = col + (0.5 if row % 2 == 1 else 0.0)
                positions[i, 1] = row * np.sqrt(3) / 2
        else:
            raise ValueError(f"Unsupported topology: {self.topology}")
        self.register_buffer("grid_positions", positions)

    # ---- initialisation from data ---------------------------------------------------------
    def pca_grid_coordinates(self) -> torch.Tensor:
        """(u, v) in [-1, 1] per unit, float64 [K, 2], for the linear initialisation: the two grid_positions coordinates,
        each axis rescaled to [-1, 1] (0 on an axis of one line), the axis with the larger extent first -- it carries the
        first principal component.  Covers the hexagonal topology: its positions are plain plane coordinates too."""
        pos = self.grid_positions.detach().double().cpu()
        lo, hi = pos.min(dim=0).values, pos.max(dim=0).values
        extent = hi - lo
        uv = torch.where(extent > 0, 2.0 * (pos - lo) / torch.where(extent > 0, extent, torch.ones_like(extent)) - 1.0,
                         torch.zeros_like(pos))
        return uv if extent[0] >= extent[1] else uv.flip(1)

    @torch.no_grad()
    def init_prototypes(self, latents, method="pca", span=2.0, seed=0):
        """Start the map from data instead of torch.rand (som_layer.py:44-56), which at a large latent width puts every
        prototype in a corner of the positive orthant, far from the data.
        method="pca": Kohonen's linear initialisation (SOM Toolbox som_lininit, MiniSom pca_weights_init): the grid spread
        over the plane of the first two principal components of `latents` [N, D] (a device tensor; pca.py),
        W = mean + span (u sqrt(lambda_1) c_1 + v sqrt(lambda_2) c_2) with (u, v) = pca_grid_coordinates().
        method="sample": latents[RandomState(seed).choice(N, K, replace=N < K)].
        With the cosine distance the rows are L2-normalised afterwards, as the random start is.  The existing Parameter is
        written in place.  Returns the fitted PCA (None for "sample")."""
        W = self.prototypes
        X = latents.flatten(start_dim=1) if latents.dim() > 2 else latents
        if X.dim() != 2 or X.shape[1] != W.shape[1]:
            raise ValueError(f"init_prototypes: latents must be [N, {W.shape[1]}], got {tuple(latents.shape)}")
        X = X.detach().to(device=W.device, dtype=torch.float32)
        if X.stride(-1) != 1:
            X = X.contiguous()
        K, D = W.shape
        fitted = None
        if method == "pca":
            from .pca import PCA
            fitted = PCA(n_components=2, random_state=seed).fit(X)
            uv = (self.pca_grid_coordinates() * float(span)).to(device=W.device, dtype=torch.float32).contiguous()
            new = torch.empty(K, D, dtype=torch.float32, device=W.device)
            ops.pca_reconstruct(uv, fitted.explained_variance_.sqrt().float(), fitted.components_, fitted.mean_, new)
        elif method == "sample":
            N = X.shape[0]
            idx = np.random.RandomState(seed).choice(N, K, replace=N < K)
            new = X[torch.from_numpy(idx).to(W.device)]
        else:
            raise ValueError(f"init_prototypes: unknown method {method!r} (pca or sample)")
        if self.distance_fcn == "cosine":
            new = torch.nn.functional.normalize(new, p=2, dim=1)
        W.copy_(new)
        self.invalidate_planes()
        return fitted

    # ---- Kohonen's batch map ----------------------------------------------------------------
    def batch_sigma_schedule(self, epochs, sigma=None) -> np.ndarray:
        """The radii of fit_batch, float64 [epochs].  None: the layer's own schedule Tmax (Tmin / Tmax)^(t / (T - 1)) (Tmax
        when T = 1); a float: constant; a pair (hi, lo): the same geometric schedule between the two; a sequence of length
        `epochs`: the radii themselves (for two epochs the two readings of a pair agree)."""
        T = int(epochs)
        if T < 1:
            raise ValueError(f"fit_batch: epochs must be >= 1, got {epochs}")
        if sigma is None:
            sigma = (float(self.Tmax), float(self.Tmin))
        if isinstance(sigma, (int, float, np.integer, np.floating)):
            s = np.full(T, float(sigma), dtype=np.float64)
        else:
            seq = [float(v) for v in sigma]
            if len(seq) == T:
                s = np.asarray(seq, dtype=np.float64)
            elif len(seq) == 2:
                hi, lo = seq
                if not (hi > 0 and lo > 0):
                    raise ValueError(f"fit_batch: radii must be positive and finite, got {sigma!r}")
                s = hi * (lo / hi) ** (np.arange(T, dtype=np.float64) / (T - 1)) if T > 1 else np.full(1, hi, dtype=np.float64)
            else:
                raise ValueError(f"fit_batch: sigma must be None, a number, a pair (hi, lo) or {T} radii, got {len(seq)} values")
        if not (np.all(np.isfinite(s)) and np.all(s > 0)):
            raise ValueError(f"fit_batch: radii must be positive and finite, got {s.tolist()}")
        return s

    def _bmu_search(self, X, bmu_out, chunk):
        """BMU of every row of X into bmu_out [N], in chunks of rows through _distances_into; -> the sum of the BMU
        distances as a float64 device scalar."""
        total = torch.zeros((), dtype=torch.float64, device=X.device)
        for i0 in range(0, X.shape[0], chunk):
            xc = X[i0:i0 + chunk]
            s = self._buffers_for(xc.shape[0], xc.device)
            self._distances_into(xc, s)
            bmu_out[i0:i0 + xc.shape[0]].copy_(s.bmu)
            total += s.dist.gather(1, s.bmu.view(-1, 1)).sum(dtype=torch.float64)
        return total

    @torch.no_grad()
    def fit_batch(self, latents, epochs=10, sigma=None, chunk=8192) -> "BatchSOMReport":
        """Train the map on `latents` [N, D] (a device tensor) with Kohonen's batch rule (SOM Toolbox som_batchtrain,
        somoclu): no learning rate, no optimizer state, one pass over the data per epoch.  Per epoch at radius sigma_t
        (batch_sigma_schedule): the BMU of every row under the layer's own distance (the existing search, `chunk` rows
        at a time), the per-unit sums and hit counts (ops.som_batch_accumulate; the rows times 1 / |row| for the cosine
        distance), then every prototype as the neighbourhood-weighted mean of the sums (ops.som_batch_update; L2-normalised
        for the cosine distance).  The prototypes are written in place; one more search follows the last update.
        The manhattan distance is refused: its batch rule is a weighted median, not a mean.  Nothing N- or D-sized goes to
        the host: the report's scalars are read once, at the end.  The searches run in a buffer set of their own ([chunk, K]
        distances), dropped on return: the layer's training and validation buffers are neither evicted nor grown."""
        W = self.prototypes
        if self._dist_mode == ops.DIST_MANHATTAN:
            raise NotImplementedError("fit_batch: the batch rule of the manhattan distance is a weighted median, not the weighted "
                                      "mean implemented here; use the cosine or the euclidean distance")
        X = latents.flatten(start_dim=1) if latents.dim() > 2 else latents
        if X.dim() != 2 or X.shape[1] != W.shape[1]:
            raise ValueError(f"fit_batch: latents must be [N, {W.shape[1]}], got {tuple(latents.shape)}")
        if X.shape[0] < 1:
            raise ValueError("fit_batch: latents is empty")
        if int(chunk) < 1:
            raise ValueError(f"fit_batch: chunk must be >= 1, got {chunk}")
        radii = self.batch_sigma_schedule(epochs, sigma)
        X = X.detach().to(device=W.device, dtype=torch.float32)
        if X.stride(-1) != 1:
            X = X.contiguous()
        N, (K, D), T, dev = X.shape[0], W.shape, len(radii), W.device
        cosine = self._dist_mode == ops.DIST_COSINE
        inv_norm = ops.row_inv_norm(X, torch.empty(N, dtype=torch.float32, device=dev)) if cosine else None
        pos = self.grid_positions.to(device=dev, dtype=torch.float32).contiguous()
        sums = torch.empty(K, D, dtype=torch.float64, device=dev)
        counts = torch.empty(K, dtype=torch.int64, device=dev)
        bad = torch.zeros(1, dtype=torch.int32, device=dev)
        bmu, prev = torch.empty(N, dtype=torch.int64, device=dev), torch.full((N,), -1, dtype=torch.int64, device=dev)
        stats = torch.zeros(T + 1, 2, dtype=torch.float64, device=dev)          # per epoch: sum of BMU distances, rows moved
        kept, self._bufs = self._bufs, {}
        try:
            for t in range(T):
                stats[t, 0] = self._bmu_search(X, bmu, int(chunk))
                stats[t, 1] = (bmu != prev).sum()
                ops.som_batch_accumulate(X, bmu, sums, counts, inv_norm=inv_norm, bad=bad)
                ops.som_batch_update(sums, counts, pos, float(radii[t]), W.data, normalize=cosine)
                self.invalidate_planes()
                bmu, prev = prev, bmu
            stats[T, 0] = self._bmu_search(X, bmu, int(chunk))
        finally:
            self._bufs = kept
        hits = torch.bincount(bmu, minlength=K)
        host = stats.cpu().numpy()
        if int(bad.item()):
            raise RuntimeError(f"fit_batch: the BMU search returned {int(bad.item())} units outside the map")
        hits = hits.cpu().numpy().astype(np.int64)
        return BatchSOMReport(sigma=radii, quantization_error=host[:T, 0] / N, final_quantization_error=float(host[T, 0] / N),
                              moved=host[:T, 1].astype(np.int64), hits=hits, dead_units=int((hits == 0).sum()), bmu=bmu)

    def adjacency_radius2(self) -> float:
        """Two units are grid neighbours when their grid_positions lie within this squared distance: square lattice
        distances^2 are 1, 2, 4, ... (2.25 takes the 8 around a cell), hexagonal ones 1, 3, ... (1.5 takes the 6)."""
        return {"square": 2.25, "hexa": 1.5}[self.topology]

    def grid_connectivity(self) -> torch.Tensor:
        """bool [K, K] on the prototypes' device: unit u touches unit v on the grid (grid_positions within
        adjacency_radius2(), the 8 around a cell of a square map, the 6 of a hexagonal one); symmetric, empty diagonal.  What
        AgglomerativeClustering(connectivity=...) takes to keep every cluster of units one region of the map."""
        pos = self.grid_positions.to(self.prototypes.device).double()
        d2 = ((pos[:, None, :] - pos[None, :, :]) ** 2).sum(dim=-1)
        near = d2 <= self.adjacency_radius2()
        near.fill_diagonal_(False)
        return near

    def _buffers_for(self, B: int, device) -> _Acts:
        s = self._bufs.get(B)
        if s is not None and s.device == device:
            return s
        K = self.n_prototypes
        f = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=device)   # noqa: E731
        s = _Acts()
        s.device = device
        s.inx, s.inw = f(B), f(K)
        s.dist, s.bmu = f(B, K), torch.empty(B, dtype=torch.int64, device=device)
        s.reranked = torch.zeros(1, dtype=torch.int32, device=device)      # rows whose BMU needed the exact re-rank (cumulative)
        s.coef, s.row_dot, s.col_dot = f(B, K), f(B), f(K)
        s.loss_sum = f(1)
        # like the ViT's activation buffers: at most two batch sizes stay allocated (training and validation batches alternate)
        self._bufs = dict(list(self._bufs.items())[-1:] + [(B, s)])
        return s

    # reference API -----------------------------------------------------------------------
    @torch.no_grad()
    def compute_distances(self, x):                                    # som_layer.py:111-125
        if x.dim() > 2:
            x = x.flatten(start_dim=1)
        s = self._buffers_for(x.shape[0], x.device)
        self._distances_into(x, s)
        return s.dist.clone()

    def _distances_into(self, x2d, s: _Acts):
        if self._dist_mode == ops.DIST_COSINE:
            W = self.prototypes
            form = self._bmu_form(x2d.shape[0], x2d.stride(0), x2d.data_ptr() % 16 == 0 and W.data_ptr() % 16 == 0)
            if form == ops.BMU_X3_PLANES:
                # norms + reduced-precision contraction + exact re-rank in one pass over X and W, on pre-split operands: the
                # prototypes' image is kept by the optimizer, the samples' written here
                self._planes_used, self._planes_rows = True, x2d.shape[0]
                if getattr(s, "xplanes", None) is None:
                    s.xplanes = ops.bmu_planes_alloc(x2d.shape[0], x2d.shape[1], x2d.device)
                wplanes = self._w_planes()
                ops.bmu_planes_from(x2d, s.xplanes)
                ops.bmu_cosine_x3_planes_fwd(x2d, W, s.xplanes, wplanes, s.dist, s.bmu, s.inx, s.inw, s.reranked)
            elif form == ops.BMU_X3:                # the same pass with the split inside the contraction
                ops.bmu_cosine_x3_fwd(x2d, W, s.dist, s.bmu, s.inx, s.inw, s.reranked)
            else:
                ops.row_inv_norm(x2d, s.inx)
                ops.row_inv_norm(W, s.inw)
                ops.bmu_cosine_fwd(x2d, W, s.inx, s.inw, s.dist, s.bmu)
        elif self._dist_mode == ops.DIST_MANHATTAN:
            ops.bmu_manhattan_fwd(x2d, self.prototypes, s.dist, s.bmu)
        else:                                   # euclidean: inx / inw hold the squared norms
            ops.row_sqnorm(x2d, s.inx)
            ops.row_sqnorm(self.prototypes, s.inw)
            ops.bmu_euclid_fwd(x2d, self.prototypes, s.inx, s.inw, s.dist, s.bmu)

    def forward(self, x):                                              # som_layer.py:83-89
        """-> (distances [B,K], bmu_indices [B] int64).  With autograd enabled the distances are differentiable
        w.r.t. `x` and the prototypes (``_SomDistancesFn``); the fused training step does not go through here."""
        if x.dim() > 2:
            x = x.flatten(start_dim=1)
        x = x.float()
        if x.stride(-1) != 1:
            x = x.contiguous()
        if torch.is_grad_enabled() and (x.requires_grad or self.prototypes.requires_grad):
            return _SomDistancesFn.apply(x, self.prototypes, self)
        with torch.no_grad():
            s = self._buffers_for(x.shape[0], x.device)
            self._distances_into(x, s)
            return s.dist.clone(), s.bmu.clone()

    def total_iterations(self) -> float:
        n = self._n_train
        if n is None:
            tr = getattr(self, "_trainer_ref", None)
            if tr is None:
                raise RuntimeError("SOMLayer: call ViTSOM.set_schedule(n_train, estimated_stepping_batches) "
                                   "or attach a trainer before training_step")
            n = len(tr.train_dataloader.dataset)
        # single-process semantics on the GLOBAL batch (the reference divides by the per-rank
        # batch size only, som_layer.py:131 -- SURVEY.md section 5, defect (b))
        return (n / (self.batch_size * self._world_size)) * self.total_epochs

    def update_temperature(self, iteration):                           # som_layer.py:127-132
        it = float(iteration)
        self.current_temperature = self.Tmax * (self.Tmin / self.Tmax) ** (it / (self.total_iterations() - 1))

    def index_to_position(self, indices):                              # som_layer.py:134-135
        return torch.stack((indices // self.map_size[1], indices % self.map_size[1]), dim=1).float()

    @torch.no_grad()
    def compute_weights(self, bmu_indices):                            # som_layer.py:144-152
        B, K = bmu_indices.shape[0], self.n_prototypes
        dev = bmu_indices.device
        h = torch.empty(B, K, dtype=torch.float32, device=dev)
        zero_d = torch.zeros(B, K, dtype=torch.float32, device=dev)
        tmp = torch.empty(1, dtype=torch.float32, device=dev)
        ops.som_neigh_loss(zero_d, bmu_indices.contiguous(), self.grid_positions, float(self.current_temperature), tmp, h=h,
                           distance=self._dist_mode)
        return h

    def som_loss(self, weights, distances):                            # som_layer.py:137-142
        """mean(weights * distances) for ANY weights tensor, differentiable in both arguments."""
        if weights.shape != distances.shape:
            raise ValueError(f"som_loss: weights {tuple(weights.shape)} and distances {tuple(distances.shape)} differ")
        return _SomLossFn.apply(weights.float().contiguous(), distances.float().contiguous())
