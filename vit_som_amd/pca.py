"""Principal component analysis on the device (sklearn.decomposition.PCA's interface; no counterpart in the reference).

The data never leaves the device: the steps that touch X [N, D] are HIP kernels (csrc/pca.hip), the host keeps the
[l, l] decisions in fp64 numpy.  Only [l, l] matrices cross, twice per pass.  A fit is bitwise reproducible.

The algorithm is block subspace iteration on the covariance operator with a Rayleigh-Ritz step each pass.  The basis is
kept as ROWS: B is [l, D] float32, like sklearn's ``components_``.  l = min(n_components + n_oversamples, N, D) <= 256.

1. Column statistics (vsom_pca_colstats).  mean[D]: the column mean, summed in fp64 in a fixed order and rounded once to
   f32.  var[D] (fp64) = sum (x - mean)^2 / (N - 1) with that rounded mean, in a second sweep.
2. Start.  B <- the rows of np.random.RandomState(seed).standard_normal((l, D)) as float32, orthonormalised (step 5
   without a rotation).
3. One pass.  Y = (X - mean) B^T [N, l] (vsom_pca_project); Zt = Y^T (X - mean) [l, D] (vsom_pca_backproject); then
   H = B Zt^T and G = Zt Zt^T, both [l, l] in fp64 on the device (vsom_pca_gram).  The mean is subtracted from each X
   tile as it is loaded, never algebraically afterwards: the column means of latents are large against their spread and
   X B^T - 1 (mean^T B^T) cancels in f32.
4. Host, fp64 (`ritz`).  theta, S = eigh((H + H^T) / 2), theta descending.  The residual estimate of Ritz pair i is
   sqrt(max(s_i^T G s_i - theta_i^2, 0)) / theta_0.
5. Orthonormalise with the Ritz rotation folded in (`orthonormalising_transform`).  G' = S^T G S; d = sqrt(diag G') (a
   zero row keeps d = 1); w, V = eigh(G' / d d^T); T = V diag(w)^-1/2 V^T diag(1/d) S^T; B <- T Zt on the device
   (vsom_pca_rotate: fp64 accumulation, one rounding).  Then once more on the new B itself (a second Gram, no rotation),
   which brings the rows to orthonormality at the f32 level.  Directions with w <= 2^-40 max w are dropped (an exactly
   zero row of Zt), and T = diag(w)^-1/2 V^T diag(1/d) S^T over the directions kept then has fewer rows;
   ``basis_width_`` is the width that is left.
   T is the SYMMETRIC inverse square root on purpose.  diag(w)^-1/2 V^T alone orthonormalises as well, but V of a
   near-identity matrix is an arbitrary rotation: it mixes the leading direction into every row of the new basis, each
   column of the next Y then carries f32 rounding relative to the LARGEST singular value, and the direction of a small
   component comes out a hundred times worse (1 - |cos| 5e-7 ... 1e-6 against <= 7e-9 on the tests' k = 24 fixture in the
   numpy restatement).  With V ... V^T the rows stay with their Ritz vectors.
   The rotation matters: the Gram matrix squares the range of the spectrum, and without rotating first the drop
   threshold eats real directions on spectra that span six decades.  The rows of S^T Zt are nearly orthogonal, so the
   scaled Gram matrix is near the identity.
   Where G' is formed matters too.  The rows of S^T Zt span more than eight decades once the trailing directions hold
   nothing but the f32 rounding of Zt (a low-noise set: lengths 1e-6 next to 300), and S^T G S on the host then
   cancels below the fp64 rounding of G itself: its small block is noise, the scaled Gram matrix gets negative
   eigenvalues and a direction is dropped that should not be.  So the rotation is applied on the DEVICE first,
   R = S^T Zt (vsom_pca_rotate; one rounding to f32, relative to each row's own length), and G' = R R^T is a Gram
   matrix of its own (vsom_pca_gram): every entry is then accurate relative to d_i d_j.  T without its S^T then
   acts on R.  `orthonormalising_transform(G, S)` keeps the one-step host form for sets without that range.
6. Steps 3-5 run n_iter times, then steps 3-4 once more.  components_ = (S^T B)[:k], explained_variance_ =
   theta[:k] / (N - 1), explained_variance_ratio_ = explained_variance_ / sum(var), singular_values_ = sqrt(theta[:k]),
   noise_variance_ by sklearn's formula from sum(var), residuals_[:k], n_iter_.  Sign rule of sklearn >= 1.5
   (svd_flip(u_based_decision=False)): the entry of largest magnitude of each component is positive.
   There is no early stop: the number of passes is fixed and passes are cheap.  A requested component whose residual
   exceeds ``tol`` draws a warning.  The estimate's floor is about 1e-4, the square root of the basis' f32
   orthonormality error.

Accuracy: the iteration works on the covariance operator in f32, so eigenvalues are accurate relative to the LARGEST one,
|lambda_i - lambda_i(fp64)| / lambda_1, not each to itself, and a direction to about that error over its eigenvalue gap
(DESIGN.md section 4).
"""
import warnings

import numpy as np
import torch

from . import ops

MAX_WIDTH = ops.PCA_MAX_WIDTH
DROP = 2.0 ** -40
_RECONSTRUCT_ROWS = 262140                    # vsom_pca_reconstruct: rows per call


class NotFittedError(ValueError, AttributeError):
    """transform / inverse_transform before fit (sklearn.exceptions.NotFittedError has the same two bases)."""


# ------------------------------------------------------------------------------------ host side, fp64 numpy
def ritz(H, G):
    """Step 4 -> (theta [l] descending, S [l, l] with the Ritz vectors as columns, residual estimates [l])."""
    H, G = np.asarray(H, np.float64), np.asarray(G, np.float64)
    theta, S = np.linalg.eigh((H + H.T) / 2)
    theta, S = theta[::-1].copy(), S[:, ::-1].copy()
    q = np.einsum("ji,jk,ki->i", S, G, S)
    top = theta[0] if theta[0] > 0 else 1.0
    return theta, S, np.sqrt(np.maximum(q - theta * theta, 0.0)) / top


def orthonormalising_transform(G, S=None):
    """Step 5 -> T [l_out, l]: with G = Zt Zt^T the rows of T Zt are orthonormal, each close to the matching row of S^T Zt
    (the symmetric inverse square root of the scaled Gram matrix).  When directions of that matrix have w <= 2^-40 max w
    they are dropped and T = diag(w)^-1/2 V^T diag(1/d) S^T over the others has l_out < l rows."""
    G = np.asarray(G, np.float64)
    l = G.shape[0]
    S = np.eye(l) if S is None else np.asarray(S, np.float64)
    Gp = S.T @ G @ S
    Gp = (Gp + Gp.T) / 2
    d = np.sqrt(np.maximum(np.diag(Gp), 0.0))
    d[d == 0] = 1.0
    w, V = np.linalg.eigh(Gp / np.outer(d, d))
    w, V = w[::-1], V[:, ::-1]
    keep = w > DROP * w[0]
    if keep.all():                                   # the symmetric inverse square root: rows stay with their Ritz vectors
        return np.ascontiguousarray((V / np.sqrt(w)) @ V.T @ (S / d).T)
    w, V = w[keep], V[:, keep]
    return np.ascontiguousarray((V / np.sqrt(w)).T @ (S / d).T)


def sign_rule(components):
    """sklearn >= 1.5's svd_flip(u_based_decision=False), in place: the entry of largest magnitude of each row becomes
    positive (a zero row stays).  One [k, D] reduction where the tensor lives."""
    idx = components.abs().argmax(dim=1, keepdim=True)
    sign = torch.sign(components.gather(1, idx))
    sign[sign == 0] = 1
    components.mul_(sign)
    return components


# ------------------------------------------------------------------------------------ the estimator
class PCA:
    """sklearn.decomposition.PCA on device tensors: fit / fit_transform / transform / inverse_transform.  Fitted:
    components_ f32 [k, D], mean_ f32 [D], explained_variance_ / explained_variance_ratio_ / singular_values_ /
    residuals_ f64 [k] (device tensors), noise_variance_, n_iter_, basis_width_, n_samples_, n_features_in_."""

    def __init__(self, n_components=2, whiten=False, n_iter=10, n_oversamples=8, random_state=0, tol=1e-3):
        self.n_components, self.whiten = n_components, bool(whiten)
        self.n_iter, self.n_oversamples = int(n_iter), int(n_oversamples)
        self.random_state, self.tol = random_state, float(tol)

    # ---- helpers
    @staticmethod
    def _rows(X, name="X"):
        if not isinstance(X, torch.Tensor) or X.dim() != 2:
            raise ValueError(f"PCA: {name} must be a 2-D tensor")
        ops._f32(X, name)
        return X

    def _fitted(self):
        if not hasattr(self, "components_"):
            raise NotFittedError("This PCA instance is not fitted yet. Call 'fit' with appropriate arguments before using this "
                                 "estimator.")

    @staticmethod
    def _grams(Zt, B=None):
        """(G, H) on the host in one copy; H is None without B."""
        l, dev = Zt.shape[0], Zt.device
        GH = torch.empty(2 if B is not None else 1, l, l, dtype=torch.float64, device=dev)
        ops.pca_gram(Zt, GH[0], B, GH[1] if B is not None else None)
        GH = GH.cpu().numpy()
        return GH[0], (GH[1] if B is not None else None)

    @staticmethod
    def _orthonormalise(Zt, G, S, a, b):
        """Step 5 on the rows of Zt; a and b are two buffers of Zt's shape, neither of them Zt.  G = Zt Zt^T is used when
        there is no rotation S.  -> (the orthonormal basis, cut to the width that is left; the other buffer)."""
        dev = Zt.device
        rotate = lambda T, src, dst: ops.pca_rotate(torch.from_numpy(np.ascontiguousarray(T)).to(dev), src, dst[:T.shape[0]])  # noqa: E731
        if S is not None:
            Zt = rotate(S.T, Zt, a)                       # R = S^T Zt, then its own Gram matrix
            G, _ = PCA._grams(Zt)
            a, b = b, a
        Q = rotate(orthonormalising_transform(G), Zt, a)
        Q2 = rotate(orthonormalising_transform(PCA._grams(Q)[0]), Q, b)
        return Q2, a

    # ---- sklearn's interface
    def fit(self, X):
        if not isinstance(X, torch.Tensor) or X.dim() != 2:
            raise ValueError("PCA: X must be a 2-D tensor")
        N, D = X.shape
        k = self.n_components
        if not isinstance(k, (int, np.integer)) or not 1 <= k <= min(N, D):
            raise ValueError(f"n_components={k!r} must be between 1 and min(n_samples, n_features)={min(N, D)!r} with "
                             f"svd_solver='subspace_iteration'")
        X = self._rows(X)
        if N < 2:
            raise ValueError("PCA: at least two samples are needed")
        if self.n_iter < 0 or self.n_oversamples < 0:
            raise ValueError("PCA: n_iter and n_oversamples must not be negative")
        k = int(k)
        l = min(k + self.n_oversamples, N, D)
        if l > MAX_WIDTH:
            raise ValueError(f"PCA: n_components + n_oversamples = {k + self.n_oversamples} > {MAX_WIDTH}, the widest basis "
                             f"the kernels take")
        dev = X.device
        mean, var = ops.pca_colstats(X)
        f = lambda: torch.empty(l, D, dtype=torch.float32, device=dev)      # noqa: E731
        start = np.random.RandomState(self.random_state).standard_normal((l, D)).astype(np.float32)
        Zt, tmp, B = torch.from_numpy(start).to(dev), f(), f()
        B, tmp = self._orthonormalise(Zt, self._grams(Zt)[0], None, tmp, B)
        # Y with a row pitch that is a multiple of four floats: backproject then takes 16-byte loads of it
        Ybuf = torch.empty(N, (l + 3) // 4 * 4, dtype=torch.float32, device=dev)

        def one_pass(B):
            w = B.shape[0]
            Y, Z = Ybuf[:, :w], Zt[:w]
            ops.pca_project(X, mean, B, None, Y)
            ops.pca_backproject(Y, X, mean, Z)
            G, H = self._grams(Z, B)
            return Z, G, ritz(H, G)

        for _ in range(self.n_iter):
            Z, G, (theta, S, res) = one_pass(B)
            # B is read by nothing once the Gram matrices are on the host: it serves as one of the two buffers
            B, tmp = self._orthonormalise(Z, G, S, tmp, B)
        Z, G, (theta, S, res) = one_pass(B)
        width = B.shape[0]
        kk = min(k, width)

        comps = torch.zeros(k, D, dtype=torch.float32, device=dev)
        ops.pca_rotate(torch.from_numpy(np.ascontiguousarray(S.T[:kk])).to(dev), B, comps[:kk])
        sign_rule(comps)
        lam = np.zeros(k)
        lam[:kk] = np.maximum(theta[:kk], 0.0)
        resid = np.zeros(k)
        resid[:kk] = res[:kk]
        total = float(var.sum())
        ev = lam / (N - 1)
        f64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)      # noqa: E731
        self.components_, self.mean_ = comps, mean
        self.explained_variance_ = f64(ev)
        self.explained_variance_ratio_ = f64(ev / total if total > 0 else np.zeros(k))
        self.singular_values_ = f64(np.sqrt(lam))
        self.residuals_ = f64(resid)
        self.total_variance_ = total
        self.noise_variance_ = (total - float(ev.sum())) / (min(N, D) - k) if k < min(N, D) else 0.0
        self.n_iter_, self.basis_width_ = self.n_iter, width
        self.n_components_, self.n_samples_, self.n_features_in_ = k, N, D
        scale = np.maximum(np.sqrt(ev), np.finfo(np.float64).eps)
        self._scale = torch.from_numpy(scale.astype(np.float32)).to(dev)
        self._inv_scale = torch.from_numpy((1.0 / scale).astype(np.float32)).to(dev)
        if width < k:
            warnings.warn(f"PCA: the data span only {width} directions, the last {k - width} components are zero")
        worst = float(resid.max())
        if worst > self.tol:
            warnings.warn(f"PCA: the residual estimate of a requested component is {worst:.2e} > tol = {self.tol:.1e} after "
                          f"{self.n_iter} passes; raise n_iter or n_oversamples")
        return self

    def transform(self, X):
        """(X - mean_) components_^T, divided by sqrt(explained_variance_) with whiten: f32 [N, k]."""
        self._fitted()
        X = self._rows(X)
        if X.shape[1] != self.n_features_in_:
            raise ValueError(f"X has {X.shape[1]} features, but PCA is expecting {self.n_features_in_} features as input.")
        N = X.shape[0]
        if N == 0:
            return X.new_empty(0, self.n_components_)
        rows = torch.cat([X, X]) if N == 1 else X           # the kernels take two rows at least
        Y = torch.empty(rows.shape[0], self.n_components_, dtype=torch.float32, device=X.device)
        ops.pca_project(rows, self.mean_, self.components_, self._inv_scale if self.whiten else None, Y)
        return Y[:N]

    def fit_transform(self, X):
        return self.fit(X).transform(X)

    def inverse_transform(self, Y):
        """Y (scaled back with whiten) components_ + mean_: f32 [M, D]."""
        self._fitted()
        Y = self._rows(Y, "Y")
        if Y.shape[1] != self.n_components_:
            raise ValueError(f"Y has {Y.shape[1]} components, but PCA has {self.n_components_}")
        M, D = Y.shape[0], self.n_features_in_
        out = torch.empty(M, D, dtype=torch.float32, device=Y.device)
        for r0 in range(0, M, _RECONSTRUCT_ROWS):
            r1 = min(M, r0 + _RECONSTRUCT_ROWS)
            ops.pca_reconstruct(Y[r0:r1], self._scale if self.whiten else None, self.components_, self.mean_, out[r0:r1])
        return out
