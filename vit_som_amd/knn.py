"""k-nearest-neighbour classifier on the device, for evaluate_knn: how much class information do the latents carry?

Every test sample is classified by a weighted vote of its k nearest training samples; nothing is trained.  Naming follows
sklearn.neighbors.KNeighborsClassifier (as KMeans and UMAP follow theirs).  Both steps that touch the data are HIP
kernels (knn.hip): `vsom_knn_query` finds the exact neighbours of the queries in a bank chunk on the f32 matrix cores and
folds them into the lists it is given, `vsom_knn_vote` turns the lists into fp64 class scores and predictions.

Two ways to give the bank:
  fit(X, y)                       keeps references to a bank that fits on the device in one piece;
  partial_fit_query(Q), then      fixes the query set first and folds bank chunks into its lists, so the bank never has
  update(X_chunk, y_chunk) ...    to exist in one piece (only its labels are kept).
The lists order neighbours by (distance, bank ordinal) and every pair's distance is computed in one fixed order, so the
streamed lists equal the one-piece lists bit for bit, whatever the chunking.

weights: "uniform" (1), "distance" (sklearn's 1 / d; neighbours at distance 0 take the whole vote) or "softmax"
(exp(-d / temperature) up to a common factor per query -- the kernel shifts by the query's smallest distance, so the
scores cannot underflow together: with metric="cosine" the DINO-style exp(sim / T) vote).  Vote ties go to the lowest
class.  Distances: "cosine" (1 - cos, clamped at 0) or "euclidean", as UMAP's kNN defines them.  A row with a NaN, an
infinity or an overflowing squared norm has no distance to anything: as a bank row it is in no list, as a query it gets
an empty list, the prediction -1, and is counted in the vote's status[1].
"""
import torch

from . import ops

METRICS = {"euclidean": ops.DIST_EUCLIDEAN, "cosine": ops.DIST_COSINE}
WEIGHTS = {"uniform": ops.KNN_UNIFORM, "distance": ops.KNN_DISTANCE, "softmax": ops.KNN_SOFTMAX}


def _is_int(v):
    return isinstance(v, int) and not isinstance(v, bool)


def _check_x(X, name):
    if not (isinstance(X, torch.Tensor) and X.dim() == 2):
        raise ValueError(f"KNNClassifier: {name} must be a float32 [N, D] tensor on the GPU")
    if X.dtype != torch.float32:
        raise ValueError(f"KNNClassifier: {name} must be float32, got {X.dtype}")
    if not X.is_cuda:
        raise ValueError(f"KNNClassifier: {name} must be on the GPU (there is no CPU path)")
    if X.shape[0] < 1 or X.shape[1] < 1:
        raise ValueError(f"KNNClassifier: {name} is empty")
    if not X.is_contiguous():
        raise ValueError(f"KNNClassifier: {name} must be contiguous")
    return X


def _check_y(y, n, device, name="y"):
    if not isinstance(y, torch.Tensor) or y.dim() != 1 or y.numel() != n:
        raise ValueError(f"KNNClassifier: {name} must be a 1-D tensor of {n} labels")
    if y.dtype.is_floating_point or y.dtype == torch.bool:
        raise ValueError(f"KNNClassifier: {name} must hold integer class labels, got {y.dtype}")
    return y.to(device=device, dtype=torch.int64).contiguous()


class KNNClassifier:
    def __init__(self, n_neighbors=20, weights="uniform", metric="cosine", temperature=0.07, n_classes=None):
        self.n_neighbors = n_neighbors
        self.weights = weights
        self.metric = metric
        self.temperature = temperature
        self.n_classes = n_classes
        self._X = self._y = None                    # fit(): the bank
        self._Q = None                              # partial_fit_query(): the fixed queries and their lists
        self._idx = self._dist = None
        self._labels, self._seen = [], 0
        self.refused_ = 0                           # neighbours the last vote refused (label outside [0, n_classes))

    def _validate(self):
        if not _is_int(self.n_neighbors) or self.n_neighbors < 1:
            raise ValueError(f"KNNClassifier: n_neighbors must be a positive integer, got {self.n_neighbors!r}")
        if self.n_neighbors > ops.KNN_MAX_K:
            raise ValueError(f"KNNClassifier: n_neighbors={self.n_neighbors} exceeds the kernel's limit of {ops.KNN_MAX_K}")
        if not isinstance(self.weights, str) or self.weights not in WEIGHTS:
            raise ValueError(f"KNNClassifier: weights must be one of {sorted(WEIGHTS)}, got {self.weights!r}")
        if not isinstance(self.metric, str) or self.metric not in METRICS:
            raise ValueError(f"KNNClassifier: metric must be one of {sorted(METRICS)}, got {self.metric!r}")
        if self.weights == "softmax" and not self.temperature > 0:
            raise ValueError(f"KNNClassifier: temperature must be positive, got {self.temperature!r}")
        if self.n_classes is not None:
            if not _is_int(self.n_classes) or self.n_classes < 1:
                raise ValueError(f"KNNClassifier: n_classes must be None or a positive integer, got {self.n_classes!r}")
            if self.n_classes > ops.KNN_MAX_CLASSES:
                raise ValueError(f"KNNClassifier: n_classes={self.n_classes} exceeds the vote kernel's limit of {ops.KNN_MAX_CLASSES}")

    # ------------------------------------------------------------------ the bank in one piece
    def fit(self, X, y):
        """Keep device references to the bank X [N, D] and its labels y [N] (not copies: do not overwrite them)."""
        self._validate()
        X = _check_x(X, "X")
        self._X, self._y = X, _check_y(y, X.shape[0], X.device)
        return self

    def _lists(self, n, device):
        k = self.n_neighbors
        return (torch.empty(n, k, dtype=torch.int64, device=device), torch.empty(n, k, dtype=torch.float32, device=device))

    def _need_bank(self, who):
        if self._X is None:
            raise ValueError(f"KNNClassifier.{who}: call fit(X, y) first")
        if self.n_neighbors > self._X.shape[0]:
            raise ValueError(f"KNNClassifier.{who}: n_neighbors={self.n_neighbors} exceeds the bank's {self._X.shape[0]} rows")

    def kneighbors(self, Q=None, return_distance=True):
        """-> (dist f32 [Nq, k], idx int64 [Nq, k]) (sklearn's order), or idx alone: the k nearest bank rows of every
        query, ascending by (distance, index).  Q=None: the bank's own rows, each excluded from its own list
        (leave-one-out; needs n_neighbors < N).  After partial_fit_query / update and without a fitted bank, Q=None
        returns the streamed lists."""
        self._validate()
        if Q is None and self._X is None and self._Q is not None:
            idx, dist = self._idx, self._dist
            return (dist, idx) if return_distance else idx
        self._need_bank("kneighbors")
        X = self._X
        exclude = None
        if Q is None:
            if self.n_neighbors >= X.shape[0]:
                raise ValueError(f"KNNClassifier.kneighbors: leave-one-out needs n_neighbors < {X.shape[0]} bank rows")
            Q, exclude = X, torch.arange(X.shape[0], dtype=torch.int64, device=X.device)
        else:
            Q = _check_x(Q, "Q")
            if Q.shape[1] != X.shape[1]:
                raise ValueError(f"KNNClassifier.kneighbors: Q has {Q.shape[1]} columns, the bank {X.shape[1]}")
        idx, dist = self._lists(Q.shape[0], X.device)
        ops.knn_query(Q, X, self.n_neighbors, METRICS[self.metric], idx, dist, exclude=exclude)
        return (dist, idx) if return_distance else idx

    # ------------------------------------------------------------------ the bank in pieces
    def partial_fit_query(self, Q):
        """Fix the query set (a device reference) and empty its lists; update() then folds bank chunks into them."""
        self._validate()
        self._Q = _check_x(Q, "Q")
        self._idx, self._dist = self._lists(Q.shape[0], Q.device)
        self._labels, self._seen = [], 0
        return self

    def update(self, X_chunk, y_chunk):
        """Fold one bank chunk (rows seen so far are its ordinals' base) into the query lists; the labels are copied, the
        rows are not kept.  No host synchronisation."""
        if self._Q is None:
            raise ValueError("KNNClassifier.update: call partial_fit_query(Q) first")
        X = _check_x(X_chunk, "X_chunk")
        if X.shape[1] != self._Q.shape[1]:
            raise ValueError(f"KNNClassifier.update: the chunk has {X.shape[1]} columns, the queries {self._Q.shape[1]}")
        y = _check_y(y_chunk, X.shape[0], X.device, "y_chunk")
        ops.knn_query(self._Q, X, self.n_neighbors, METRICS[self.metric], self._idx, self._dist, index_base=self._seen,
                      accumulate=self._seen > 0)
        self._labels.append(y.clone())
        self._seen += X.shape[0]
        return self

    # ------------------------------------------------------------------ the vote
    def _vote(self, idx, dist, labels, want_scores):
        n_classes = self.n_classes
        if n_classes is None:
            n_classes = int(labels.max()) + 1 if labels.numel() else 1
            if n_classes > ops.KNN_MAX_CLASSES:
                raise ValueError(f"KNNClassifier: the labels reach {n_classes - 1}: more than the vote kernel's {ops.KNN_MAX_CLASSES} classes")
        dev = idx.device
        pred = torch.empty(idx.shape[0], dtype=torch.int64, device=dev)
        scores = torch.empty(idx.shape[0], n_classes, dtype=torch.float64, device=dev) if want_scores else None
        self._status = torch.zeros(2, dtype=torch.int32, device=dev)
        ops.knn_vote(idx, dist, labels, n_classes, WEIGHTS[self.weights], self.temperature, pred, self._status, scores)
        return pred, scores

    def _predict(self, Q, want_scores):
        self._validate()
        if Q is None:
            if self._Q is None or not self._labels:
                raise ValueError("KNNClassifier.predict: no queries given and no streamed lists (partial_fit_query / update)")
            if self.n_neighbors > self._seen:
                raise ValueError(f"KNNClassifier.predict: n_neighbors={self.n_neighbors} exceeds the bank's {self._seen} rows")
            return self._vote(self._idx, self._dist, torch.cat(self._labels), want_scores)
        self._need_bank("predict")
        dist, idx = self.kneighbors(_check_x(Q, "Q"))
        return self._vote(idx, dist, self._y, want_scores)

    def predict(self, Q=None):
        """-> int64 [Nq] device tensor of predicted classes (Q=None: for the streamed queries).  A query without a
        countable neighbour gets -1.  Does not synchronise; `refused()` reads how many neighbours the vote refused."""
        return self._predict(Q, False)[0]

    def predict_scores(self, Q=None):
        """-> fp64 [Nq, n_classes] device tensor of the class scores (the summed vote weights)."""
        return self._predict(Q, True)[1]

    def refused(self):
        """Neighbours of the last vote whose label fell outside [0, n_classes) (one host read)."""
        self.refused_ = int(self._status[0])
        return self.refused_

    def score(self, Q, y):
        """Mean accuracy of predict(Q) against y (a host float)."""
        pred = self.predict(Q)
        y = _check_y(y, pred.numel(), pred.device)
        if self.refused():
            raise ValueError(f"KNNClassifier.score: {self.refused_} neighbour labels fell outside [0, n_classes)")
        return float((pred == y).double().mean())
