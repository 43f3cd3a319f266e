"""Surprise adequacy: DSA, LSA, MDSA, MLSA + multimodal wrappers and
surprise coverage.

Capability parity with reference src/core/surprise.py (behavioural contracts
cited per class), re-designed for MI355X: every hot loop is a pairwise
distance problem routed through ops.* (the MFMA pairwise-sqdist kernel with
min/argmin or logsumexp epilogues on device; torch fallback on CPU). Fits
that are tiny (covariances, Cholesky, GMM EM over <=300 features) happen in
float64 on the host for scipy-grade stability, then push whitened fp32
operands to the device.
"""

import abc
import os
import warnings
from typing import Callable, Dict, Iterable, List, Optional, Tuple, Union

import numpy as np
import torch

from .. import ops
from .bitmap import BitProfile
from .kde import StableGaussianKDE
from .kmeans import (
    kmeans_fit,
    kmeans_fit_many,
    kmeans_predict,
    silhouette_score,
    silhouette_scores_many,
)

Activations = Union[List, np.ndarray, torch.Tensor]
Predictions = Union[List, np.ndarray, torch.Tensor]
Discriminator = Callable[[torch.Tensor, Optional[torch.Tensor]], torch.Tensor]

# Strict mode: inputs routed to a mode/class unseen at fit time RAISE (the
# reference's behaviour, surprise.py:308-315) instead of scoring +inf with a
# warning. Off by default; parity-validation runs flip it on to detect the
# divergence instead of absorbing it.
_STRICT_MODES = os.environ.get("TIP_STRICT_MODES") == "1"


def set_strict_modes(flag: bool) -> bool:
    """Toggle strict unseen-mode handling; returns the previous value."""
    global _STRICT_MODES
    prev = _STRICT_MODES
    _STRICT_MODES = bool(flag)
    return prev


# ---------------------------------------------------------------------------
# Input normalisation helpers
# ---------------------------------------------------------------------------


def _flatten_layers(layers: Activations) -> torch.Tensor:
    """Flatten per-sample activations to [N, D] (list of layers concatenated).

    Mirrors reference surprise.py:168-177.
    """
    if isinstance(layers, torch.Tensor):
        return layers.reshape(layers.shape[0], -1) if layers.dim() != 2 else layers
    if isinstance(layers, np.ndarray):
        t = torch.from_numpy(np.ascontiguousarray(layers))
        return t.reshape(t.shape[0], -1)
    parts = []
    for l in layers:
        t = l if isinstance(l, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(l))
        parts.append(t.reshape(t.shape[0], -1))
    return torch.cat(parts, dim=1)


def _class_predictions(predictions: Predictions) -> torch.Tensor:
    """1-D integer class predictions (reference surprise.py:136-165)."""
    if isinstance(predictions, torch.Tensor):
        p = predictions
    else:
        p = torch.as_tensor(np.asarray(predictions))
    assert p.dim() == 1, (
        "Class predictions must be one-dimensional (use argmax over softmax)"
    )
    if not p.dtype in (torch.int64, torch.int32, torch.int16, torch.uint8):
        pl = p.long()
        assert torch.allclose(p.double(), pl.double(), atol=1e-5), (
            "Predictions must be integers"
        )
        p = pl
    assert bool((p >= 0).all()), "Class predictions must be >= 0"
    return p.long()


def _subsample_arrays(
    subsampling: Union[int, float], arrays: Tuple[torch.Tensor, ...], seed: int
) -> Tuple[torch.Tensor, ...]:
    """Common-index subsampling (reference surprise.py:62-87; numpy
    RandomState for index parity)."""
    n = arrays[0].shape[0]
    assert all(a.shape[0] == n for a in arrays)
    if subsampling == 1.0:
        return arrays
    if isinstance(subsampling, int) and subsampling > 0:
        num = min(subsampling, n)
    elif 0 < subsampling < 1:
        num = int(subsampling * n)
    else:
        raise ValueError(
            "subsampling must be a float in (0,1) or a positive int"
        )
    rng = np.random.RandomState(seed)
    idx = torch.from_numpy(rng.choice(np.arange(n), num, replace=False))
    return tuple(a[idx.to(a.device)] for a in arrays)


def _subsample_array(subsampling, array, seed):
    return _subsample_arrays(subsampling, (array,), seed)[0]


# ---------------------------------------------------------------------------
# Surprise coverage
# ---------------------------------------------------------------------------


class SurpriseCoverageMapper:
    """Maps SA values to bucket-membership coverage profiles.

    Half-open buckets over linspace(0, upper_bound, sections+1); a value equal
    to the upper bound sets no bit (reference surprise.py:186-209). Profiles
    are packed bitmaps.
    """

    def __init__(self, sections: int, upper_bound: float, overflow_bucket: bool = False):
        self.sections = int(sections)
        self.upper_bound = float(upper_bound)
        num = sections if overflow_bucket else sections + 1
        thr = torch.linspace(0.0, self.upper_bound, num, dtype=torch.float64)
        if overflow_bucket:
            thr = torch.cat([thr, torch.tensor([float("inf")], dtype=torch.float64)])
        self.thresholds = thr

    def get_coverage_profile(self, surprise_values) -> BitProfile:
        v = surprise_values
        if not isinstance(v, torch.Tensor):
            v = torch.as_tensor(np.asarray(v))
        words = ops.bucketize_profile(v, self.thresholds.to(v.device if v.is_cuda else "cpu"))
        return BitProfile(words, self.sections)


# ---------------------------------------------------------------------------
# SA hierarchy
# ---------------------------------------------------------------------------


class SA(abc.ABC):
    """Abstract surprise-adequacy scorer."""

    @abc.abstractmethod
    def __call__(
        self, activations: Activations, predictions: Predictions, num_threads: int = 1
    ) -> torch.Tensor:
        """Surprise adequacy per sample (1-D tensor)."""


def _by_class_discriminator(activations, predictions):
    return _class_predictions(predictions)


KMEANS_MODES = ("looped", "batched")


def resolve_kmeans_mode(kmeans_mode: str) -> str:
    """The k-means discovery mode in force: ``TIP_KMEANS_MODE`` overrides the
    argument; anything but ``"looped"`` or ``"batched"`` raises ValueError."""
    kmeans_mode = os.environ.get("TIP_KMEANS_MODE", kmeans_mode)
    if kmeans_mode not in KMEANS_MODES:
        raise ValueError(
            f"kmeans_mode must be 'looped' or 'batched', got {kmeans_mode!r}"
        )
    return kmeans_mode


class _KmeansDiscriminator:
    """Chooses k in potential_k by silhouette on (subsampled) training data
    and assigns new samples to the nearest center
    (reference surprise.py:102-133; sklearn replaced by the device-capable
    core.kmeans Lloyd/silhouette built on the pairwise kernel).

    ``kmeans_mode="looped"`` (the default) fits and scores one k after the
    other. ``"batched"`` runs every restart of every k in lockstep
    (``kmeans_fit_many``) and scores all k from one pass over the distances
    (``silhouette_scores_many``); the selection rule is the same: k
    ascending, a strictly greater silhouette wins. ``TIP_KMEANS_MODE``
    overrides the argument."""

    def __init__(
        self,
        training_data: Activations,
        potential_k: Iterable[int],
        subsampling: Union[int, float] = 1.0,
        subsampling_seed: int = 0,
        n_init: int = 10,
        max_iter: int = 300,
        kmeans_mode: str = "looped",
    ):
        self.kmeans_mode = resolve_kmeans_mode(kmeans_mode)
        data = _flatten_layers(training_data).float()
        data = _subsample_array(subsampling, data, seed=subsampling_seed)
        self.best_score = -float("inf")
        self.best_k = None
        self.best_centers = None
        if self.kmeans_mode == "batched":
            ks = list(potential_k)
            fits = kmeans_fit_many(
                data, ks, n_init=n_init, max_iter=max_iter, seed=subsampling_seed
            )
            scores = silhouette_scores_many(data, [fits[k][1] for k in ks])
            for k, score in zip(ks, scores):
                if score > self.best_score:
                    self.best_score = score
                    self.best_k = k
                    self.best_centers = fits[k][0]
            return
        for k in potential_k:
            centers, labels, _ = kmeans_fit(
                data, k, n_init=n_init, max_iter=max_iter, seed=subsampling_seed
            )
            score = silhouette_score(data, labels)
            if score > self.best_score:
                self.best_score = score
                self.best_k = k
                self.best_centers = centers

    def __call__(self, activations, predictions=None):
        x = _flatten_layers(activations).float()
        return kmeans_predict(x.to(self.best_centers.device), self.best_centers).cpu()


class MultiModalSA(SA):
    """Routes samples to per-mode SA instances via a discriminator
    (reference surprise.py:226-371)."""

    def __init__(self, discriminator: Discriminator, modal_sa: Dict[int, SA]):
        self.discriminator = discriminator
        self.modal_sa = modal_sa

    @staticmethod
    def build_by_class(activations, predictions, sa_constructor) -> "MultiModalSA":
        return MultiModalSA.build(
            activations, predictions, _by_class_discriminator, sa_constructor
        )

    @staticmethod
    def build_with_kmeans(
        activations,
        predictions,
        sa_constructor,
        potential_k: Iterable[int],
        n_init: int = 10,
        max_iter: int = 300,
        subsampling: Union[int, float] = 1.0,
        subsampling_seed: int = 0,
        kmeans_mode: str = "looped",
    ) -> "MultiModalSA":
        disc = _KmeansDiscriminator(
            training_data=activations,
            potential_k=potential_k,
            n_init=n_init,
            max_iter=max_iter,
            subsampling=subsampling,
            subsampling_seed=subsampling_seed,
            kmeans_mode=kmeans_mode,
        )
        return MultiModalSA.build(activations, predictions, disc, sa_constructor)

    @staticmethod
    def build(activations, predictions, discriminator, sa_constructor) -> "MultiModalSA":
        acts = _flatten_layers(activations)
        preds = None if predictions is None else _class_predictions(predictions)
        modal_idx = discriminator(acts, preds)
        if not isinstance(modal_idx, torch.Tensor):
            modal_idx = torch.as_tensor(np.asarray(modal_idx))
        modal_idx = modal_idx.cpu()
        sas: Dict[int, SA] = {}
        for modal_id in torch.unique(modal_idx).tolist():
            sel = modal_idx == modal_id
            a = acts[sel.to(acts.device)]
            p = None if preds is None else preds[sel.to(preds.device)]
            sas[int(modal_id)] = sa_constructor(a, p)
        return MultiModalSA(discriminator, sas)

    def fuse(self, device=None) -> "GroupedGaussianSA":
        """Opt-in single-launch form of a Gaussian multimodal SA.

        Allowed when every mode is an :class:`MDSA` or every mode is an
        :class:`MLSA` (TypeError otherwise). The per-mode tables are stacked
        once and every call scores all modes through
        ``ops.grouped_gaussian_scores``: no Python loop over modes and, on
        the GPU, no copy of the mode ids to the host. ``__call__`` of this
        object is unchanged.
        """
        return GroupedGaussianSA(self, device=device)

    def __call__(self, activations, predictions=None, num_threads: int = 1):
        acts = _flatten_layers(activations)
        preds = None if predictions is None else _class_predictions(predictions)
        modal_idx = self.discriminator(acts, preds)
        if not isinstance(modal_idx, torch.Tensor):
            modal_idx = torch.as_tensor(np.asarray(modal_idx))
        modal_idx = modal_idx.cpu()
        assert modal_idx.shape[0] == acts.shape[0], "discriminator length mismatch"
        if modal_idx.shape[0] == 0:
            return torch.empty(0)
        if acts.is_cuda:
            # device-resident result: no per-mode host sync
            res = torch.full(
                (modal_idx.shape[0],), -float("inf"),
                dtype=torch.float32, device=acts.device,
            )
        else:
            res = torch.full(
                (modal_idx.shape[0],), -float("inf"), dtype=torch.float64
            )
        for modal_id in torch.unique(modal_idx).tolist():
            try:
                sa = self.modal_sa[int(modal_id)]
            except KeyError:
                # Sample routed to a mode that never occurred in the fitting
                # data (e.g. a predicted class absent from the training
                # predictions). The reference raises here
                # (surprise.py:308-315); we treat such inputs as maximally
                # surprising instead, consistent with DSA's handling —
                # unless strict mode is on (set_strict_modes / TIP_STRICT_MODES).
                if _STRICT_MODES:
                    raise ValueError(
                        f"No modal found for modal id {modal_id} "
                        f"(reference raises here)"
                    )
                warnings.warn(
                    f"No modal found for modal id {modal_id}; scoring those "
                    f"inputs as maximally surprising (+inf).",
                    UserWarning,
                )
                sel = modal_idx == modal_id
                res[sel.to(res.device)] = float("inf")
                continue
            sel = modal_idx == modal_id
            a = acts[sel.to(acts.device)]
            p = None if preds is None else preds[sel.to(preds.device)]
            vals = sa(a, p)
            if res.is_cuda:
                res[sel.to(res.device)] = vals.float().to(res.device)
            else:
                res[sel] = vals.double().cpu()
        return res


class MDSA(SA):
    """Mahalanobis-distance surprise adequacy (reference surprise.py:374-393).

    Fit: float64 ML covariance + pseudo-inverse precision — ON DEVICE when
    the activations live there (K3: the D x D covariance is one fp64 GEMM,
    the pseudo-inverse one rocSOLVER eigh; the CPU-sklearn fit was 45 s of
    a full-scale run). Score: (x-mu) P (x-mu)^T row-dot GEMM.
    """

    def __init__(self, activations: Activations, device=None):
        acts_in = _flatten_layers(activations)
        fit_dev = acts_in.device if acts_in.is_cuda else torch.device("cpu")
        acts = acts_in.to(fit_dev, torch.float64)
        mean = acts.mean(dim=0)
        centered = acts - mean
        # sklearn EmpiricalCovariance: ML estimate (divide by N)
        cov = centered.t() @ centered / acts.shape[0]
        precision = torch.linalg.pinv(cov, hermitian=True)
        self.mean = mean.cpu()
        self.precision = precision.cpu()
        self.device = device if device is not None else (
            fit_dev if fit_dev.type == "cuda" else None
        )
        if self.device is not None and str(self.device) != "cpu":
            self._mean_dev = mean.float().to(self.device)
            self._prec_dev = precision.float().to(self.device)

    def __call__(self, activations, predictions=None, num_threads=None):
        acts = _flatten_layers(activations)
        if acts.is_cuda or (self.device is not None and str(self.device) != "cpu"):
            dev = acts.device if acts.is_cuda else self.device
            x = acts.float().to(dev)
            m = getattr(self, "_mean_dev", self.mean.float().to(dev))
            p = getattr(self, "_prec_dev", self.precision.float().to(dev))
            d = x - m
            return ((d @ p) * d).sum(dim=1)
        d = acts.double() - self.mean
        return ((d @ self.precision) * d).sum(dim=1)


class LSA(SA):
    """Likelihood-based surprise adequacy: -log KDE density
    (reference surprise.py:396-495).

    Keeps the reference's variance-based feature selection (top
    ``max_features`` by variance) and the drop-feature retry ladder on
    non-positive-definite covariances.
    """

    def __init__(
        self,
        activations: Activations,
        var_threshold: Optional[float] = None,
        max_features: Optional[Union[int, float]] = 300,
        device=None,
        shard_train: bool = False,
    ):
        # fit stays on the activations' device (K2/K19: variance selection,
        # covariance, jitter ladder and Cholesky are all device-capable)
        from ..parallel.dist import get_world_size

        # train-axis sharding: the KDE fit happens on the full
        # (replicated) class data — identical on every rank — but evaluation
        # sums the kernel over this rank's whitened-train row shard only,
        # merging partial logsumexps across ranks.
        self.shard_train = bool(shard_train) and get_world_size() > 1
        acts = _flatten_layers(activations).double()
        assert var_threshold is None or max_features is None, (
            "var_threshold and max_features cannot both be specified"
        )
        self.removed_neurons: List[int] = []
        if var_threshold is not None and var_threshold > 0:
            var = acts.var(dim=0, unbiased=True)
            self.removed_neurons = torch.nonzero(var < var_threshold).flatten().tolist()
        if max_features is not None:
            if max_features < 1:
                num_features = int(min(max_features * acts.shape[1], acts.shape[1]))
            else:
                num_features = int(min(max_features, acts.shape[1]))
            var = acts.var(dim=0, unbiased=True).cpu().numpy()
            dropped = np.argsort(var, kind="stable")[:-num_features]
            self.removed_neurons = [int(x) for x in dropped]
        self.device = device
        self.kde = self._create_kde(acts)

    def _create_kde(self, acts: torch.Tensor):
        cleaned = self._remove_unused_columns(acts)
        if cleaned.shape[1] == 0:
            warnings.warn(
                "Feature removal dropped all ATs; this LSA instance will "
                "always return density 0",
                UserWarning,
            )
            return None
        if cleaned.shape[0] < 2:
            # scipy's gaussian_kde (and the reference) would crash outright
            # on a singleton class; degrade to the prepare-failed behaviour
            warnings.warn(
                "LSA fit with < 2 samples; reporting density 0 for this mode",
                UserWarning,
            )
            return None
        try:
            return StableGaussianKDE(cleaned)
        except (np.linalg.LinAlgError, ValueError) as e:
            msg = str(e)
            if "leading minor of the array is not positive definite" in msg:
                import re

                problematic_row = int(re.findall(r"\d+", msg)[0]) - 1
                original = np.delete(np.arange(acts.shape[1]), self.removed_neurons)
                problematic_index = int(original[problematic_row])
                warnings.warn(
                    f"Dropping AT {problematic_index}, as leading to numerical error.",
                    UserWarning,
                )
                self.removed_neurons.append(problematic_index)
                return self._create_kde(acts)
            raise

    def _remove_unused_columns(self, acts: torch.Tensor) -> torch.Tensor:
        if self.removed_neurons:
            keep = np.delete(np.arange(acts.shape[1]), self.removed_neurons)
            return acts.index_select(
                1, torch.from_numpy(keep).to(acts.device)
            )
        return acts

    def __call__(self, activations, predictions=None, num_threads=0):
        acts = _flatten_layers(activations)
        if acts.is_cuda and self.kde is not None and not self.kde.prepare_failed:
            # device fast path: column-select + whiten-GEMM + MFMA KDE kernel,
            # no host round-trip
            if self.removed_neurons:
                keep = torch.from_numpy(
                    np.delete(np.arange(acts.shape[1]), self.removed_neurons)
                ).to(acts.device)
                acts = acts.index_select(1, keep)
            return -self.kde.log_density_device(
                acts.float().contiguous(), shard_train=self.shard_train
            )
        dev = acts.device if acts.is_cuda else self.device
        acts = self._remove_unused_columns(acts.double().cpu())
        if self.kde is None:
            return torch.zeros(acts.shape[0], dtype=torch.float64)
        logd = self.kde.log_density(acts, device=dev, shard_train=self.shard_train)
        return -logd


class MLSA(SA):
    """Multimodal likelihood SA: -log GMM likelihood
    (reference surprise.py:498-520).

    CPU inputs fit with sklearn's EM (reference parity, the test oracle);
    device inputs fit with a torch EM on the GPU (K4 — the CPU GMM fit was
    84 s of a full-scale run, the device EM is seconds). Scoring is torch
    either way. The two fits converge to (possibly) different local optima,
    as any EM with different initialisation does.
    """

    REG_COVAR = 1e-6  # sklearn's default covariance regulariser

    def __init__(self, activations: Activations, num_components: int = 2, device=None):
        acts_t = _flatten_layers(activations)
        self.device = device
        if acts_t.is_cuda:
            self._fit_device(acts_t.double(), num_components)
            self._sync_fit()
            return
        from sklearn.mixture import GaussianMixture

        acts = acts_t.double().cpu().numpy()
        self.gmm = GaussianMixture(n_components=num_components)
        self.gmm.fit(acts)
        self.means = torch.from_numpy(self.gmm.means_)  # [k, d]
        # precision cholesky P with Sigma^-1 = P P^T
        self.prec_chol = torch.from_numpy(self.gmm.precisions_cholesky_)
        self.log_weights = torch.from_numpy(np.log(self.gmm.weights_))
        self._sync_fit()

    def _sync_fit(self):
        """Broadcast the fit from rank 0 so every rank scores with identical
        parameters: EM init is the one nondeterministic fit in the SA family
        (sklearn seeds from the process RNG; the device EM's kmeans init is
        seeded but EM converges to a local optimum either way). Part of the
        "broadcast statistics at setup" collective set."""
        from ..parallel.dist import is_initialized

        if not is_initialized():
            return
        import torch.distributed as dist

        from ..parallel.dist import _staging_device

        for t in (self.means, self.prec_chol, self.log_weights):
            staged, home = _staging_device(t)
            dist.broadcast(staged, src=0)
            if home is not None:
                t.copy_(staged.to(home))

    def _fit_device(self, x: torch.Tensor, k: int, iters: int = 60, tol: float = 1e-3):
        """Full-covariance EM in fp64 on the device (kmeans init)."""
        n, d = x.shape
        centers, labels, _ = kmeans_fit(x.float(), k, n_init=1, max_iter=20, seed=0)
        means = torch.stack(
            [
                x[labels == c].mean(dim=0) if bool((labels == c).any()) else x[c % n]
                for c in range(k)
            ]
        )
        weights = torch.full((k,), 1.0 / k, dtype=torch.float64, device=x.device)
        covs = []
        eye = torch.eye(d, dtype=torch.float64, device=x.device)
        for c in range(k):
            sel = labels == c
            xc = (x[sel] if bool(sel.any()) else x) - means[c]
            covs.append(xc.t() @ xc / max(int(sel.sum()), 1) + self.REG_COVAR * eye)
        covs = torch.stack(covs)
        prev_ll = None
        for _ in range(iters):
            # E-step: per-component log N(x; mu, Sigma) via Cholesky solves
            log_prob = torch.empty(n, k, dtype=torch.float64, device=x.device)
            chols = torch.linalg.cholesky(covs)
            for c in range(k):
                xc = (x - means[c]).t()
                y = torch.linalg.solve_triangular(chols[c], xc, upper=False)
                logdet = torch.log(torch.diagonal(chols[c])).sum()
                log_prob[:, c] = (
                    -0.5 * (y * y).sum(dim=0)
                    - logdet
                    - 0.5 * d * np.log(2 * np.pi)
                    + torch.log(weights[c])
                )
            norm = torch.logsumexp(log_prob, dim=1)
            ll = float(norm.mean())
            resp = torch.exp(log_prob - norm.unsqueeze(1))
            # M-step
            nk = resp.sum(dim=0).clamp_min(1e-10)
            means = (resp.t() @ x) / nk.unsqueeze(1)
            for c in range(k):
                xc = x - means[c]
                covs[c] = (xc * resp[:, c : c + 1]).t() @ xc / nk[c] + self.REG_COVAR * eye
            weights = nk / n
            if prev_ll is not None and abs(ll - prev_ll) < tol:
                break
            prev_ll = ll
        chols = torch.linalg.cholesky(covs)
        # precision cholesky P = L^-T (Sigma^-1 = P P^T)
        eye_b = eye.unsqueeze(0).expand(k, d, d)
        self.prec_chol = torch.linalg.solve_triangular(
            chols.transpose(1, 2), eye_b, upper=True
        )
        self.means = means
        self.log_weights = torch.log(weights)

    def _score_samples(self, x: torch.Tensor) -> torch.Tensor:
        k, d = self.means.shape[0], self.means.shape[1]
        log_probs = torch.empty(x.shape[0], k, dtype=x.dtype, device=x.device)
        for j in range(k):
            p = self.prec_chol[j].to(x.device, x.dtype)
            mu = self.means[j].to(x.device, x.dtype)
            y = (x - mu) @ p
            logdet = torch.log(torch.diagonal(p)).sum()
            log_probs[:, j] = (
                logdet
                - 0.5 * d * np.log(2 * np.pi)
                - 0.5 * (y * y).sum(dim=1)
                + self.log_weights[j].to(x.device, x.dtype)
            )
        return torch.logsumexp(log_probs, dim=1)

    def __call__(self, activations, predictions=None, num_threads=0):
        acts = _flatten_layers(activations)
        if acts.is_cuda:
            return -self._score_samples(acts.float())
        return -self._score_samples(acts.double())


class DSA(SA):
    """Distance-based surprise adequacy (reference surprise.py:523-651).

    dsa(x) = d_a / d_b where d_a = distance from x to its nearest same-class
    training AT ``a``, and d_b = distance from ``a`` (two-hop, per the
    reference's refinement) to the nearest training AT of another class.

    The reference slices work into 10-row "badges" on a 5-thread pool to
    bound numpy's N x M x D broadcast; here each class is one fused
    pairwise-distance + row-min/argmin kernel launch on the device.

    ``shard_train=True`` shards the train-AT axis across the ranks of an
    initialised torch.distributed group: every rank keeps
    only its contiguous row-shard of each class, scores the (replicated)
    inputs against the shard, and the per-rank partial (min, argmin) merge
    with a deterministic rank-ordered reduction, so 1-GPU and N-GPU scores
    are identical. The two-hop b-table is fit sharded too (each rank
    computes the rows of its shard) and then all-gathered, since scoring
    needs b-table entries of whichever global row wins the merge.
    """

    def __init__(
        self,
        activations: Activations,
        predictions: Predictions,
        badge_size: int = 10,
        subsampling: Union[int, float] = 1.0,
        subsampling_seed: int = 0,
        device=None,
        shard_train: bool = False,
    ):
        acts = _flatten_layers(activations)
        preds = _class_predictions(predictions)
        acts, preds = _subsample_arrays(subsampling, (acts, preds), subsampling_seed)
        self.device = device
        if device is not None and str(device) != "cpu":
            acts = acts.float().to(device)
            preds = preds.to(device)
        self.train_activations = acts
        self.train_predictions = preds
        self.num_classes = int(preds.max().item()) + 1
        self.badge_size = badge_size  # kept for API parity; kernels batch freely
        from ..parallel.dist import get_world_size

        self.shard_train = bool(shard_train) and get_world_size() > 1
        self._class_cache = None  # device path: per-class (same_ats, b_table)

    def _build_class_cache(self):
        """Per class c: (same-class ATs contiguous, b_table, same_norm,
        shard_offset) where b_table[i] = distance from same-class AT i to its
        nearest OTHER-class training AT.

        dist_b depends only on which training AT is closest to the input
        (two-hop), so it is a fixed function of the training set: we
        precompute it once at fit time (part of the SA "setup" timing
        bucket) and the per-input path becomes hop-1 + a gather.

        With ``shard_train`` the stored same-class ATs are this rank's row
        shard (offset recorded) while the b-table stays global: the b-table
        rows of the local shard are computed here (1/world of the fit work)
        and all-gathered.
        """
        from ..parallel import sharded as shd
        from ..parallel.dist import allgather_rows

        cache = {}
        for label in range(self.num_classes):
            same_sel = self.train_predictions == label
            same = self.train_activations[same_sel].contiguous()
            if same.shape[0] == 0:
                cache[label] = (None, None, None, 0)
                continue
            other = self.train_activations[~same_sel].contiguous()
            if self.shard_train:
                n_same = same.shape[0]
                local, off = shd.shard_rows(same)
                if other.shape[0] == 0:
                    # single-class training set: an all-inf b-table keeps the
                    # global indexing consistent across ranks and yields
                    # dsa = dist/inf = 0 ("no contrast"), like the dense path
                    b_table = torch.full(
                        (n_same,), float("inf"),
                        dtype=same.dtype, device=same.device,
                    )
                    cache[label] = (local, b_table, self._rownorm(local), off)
                    continue
                if local.shape[0] > 0:
                    bt_local, _ = ops.rowmin_l2(local, other)
                else:
                    bt_local = torch.empty(
                        0, dtype=same.dtype, device=same.device
                    )
                b_table = allgather_rows(bt_local, n_same)
                cache[label] = (local, b_table, self._rownorm(local), off)
                continue
            if other.shape[0] == 0:
                cache[label] = (same, None, self._rownorm(same), 0)
                continue
            b_table, _ = ops.rowmin_l2(same, other)
            cache[label] = (same, b_table, self._rownorm(same), 0)
        self._class_cache = cache

    @staticmethod
    def _rownorm(t: torch.Tensor):
        """Cached ||row||^2 for the GPU kernels (None on CPU/empty)."""
        if not t.is_cuda or t.shape[0] == 0:
            return None
        return (t.float() * t.float()).sum(dim=1).contiguous()

    def __call__(self, activations, predictions, num_threads=None):
        target_ats = _flatten_layers(activations)
        target_pred = _class_predictions(predictions)
        dev = self.train_activations.device
        target_ats = target_ats.to(dev, self.train_activations.dtype)
        target_pred = target_pred.to(dev)
        if target_ats.is_cuda:
            # grouped fast path: one segmented kernel launch for all classes
            fused = self._grouped_call(target_ats, target_pred)
            if fused is not None:
                return fused
        dsa = torch.empty(target_pred.shape[0], dtype=target_ats.dtype, device=dev)
        if self._class_cache is None:
            self._build_class_cache()
        # single host sync: which classes are present and how many of each
        counts = torch.bincount(
            target_pred, minlength=self.num_classes
        ).cpu().tolist()
        for label in range(self.num_classes, len(counts)):
            if counts[label]:
                # predicted class never seen in training predictions:
                # maximally surprising (the reference would crash here)
                if _STRICT_MODES:
                    raise ValueError(
                        f"Predicted class {label} was never predicted on the "
                        f"training set (reference raises here)"
                    )
                dsa[target_pred == label] = float("inf")
        if self.shard_train:
            from ..parallel import sharded as shd
        for label in range(self.num_classes):
            if counts[label] == 0:
                continue
            sel = target_pred == label
            same, b_table, same_norm, off = self._class_cache[label]
            if same is None:
                dsa[sel] = float("inf")
                continue
            samples = target_ats[sel]
            if b_table is None:
                dsa[sel] = 0.0  # single-class training set: no contrast
                continue
            if self.shard_train:
                dist_a, closest_idx = shd.sharded_rowmin_l2(
                    samples, same, off, same_norm
                )
            else:
                dist_a, closest_idx = ops.rowmin_l2(samples, same, same_norm)
            dsa[sel] = dist_a / b_table[closest_idx]
        return dsa

    def _grouped_call(self, target_ats, target_pred):
        """Single-launch DSA via the grouped segmented kernel (GPU only).

        Returns None when inapplicable (labels outside the fitted range);
        numerics equal the per-class path (same kernels, same tie rules)."""
        try:
            from ..engine.serving import FusedPrioritizer
        except ImportError:  # pragma: no cover
            return None
        if bool((target_pred >= self.num_classes).any()):
            return None
        fp = getattr(self, "_fused_prio", None)
        if fp is None:
            try:
                fp = FusedPrioritizer(self, None, target_ats.device)
            except Exception:  # noqa: BLE001 - fall back to per-class loop
                return None
            self._fused_prio = fp
        dsa, _ = fp(target_ats.float(), target_pred)
        return dsa


class GroupedGaussianSA(SA):
    """All modes of a Gaussian :class:`MultiModalSA` scored in one op call
    (``MultiModalSA.fuse``): pc-MDSA / pc-MMDSA (every mode an MDSA) as
    Mahalanobis forms, pc-MLSA (every mode an MLSA) as mixture NLLs.

    The tables are stacked once from the fp64 fits: MDSA contributes its mean
    and precision, MLSA its means, ``M = P P^T`` and ``logc = log w +
    sum(log diag P) - D/2 log 2 pi`` per component, all formed in fp64. On a
    GPU device they are cast to fp32 (the kernel's dtype); on the CPU they
    stay fp64, so the fused CPU result equals the per-mode loop to rounding.
    Mode ids are compacted to groups ``0..G-1`` through a lookup tensor on
    the device; an id without a fitted mode maps to group -1 and scores
    ``+inf``.

    ``check_unseen`` keeps the per-mode semantics for such ids (UserWarning,
    or ValueError in strict mode). The check is one device reduction whose
    result is read on the host; with ``check_unseen=False`` a GPU call makes
    no device-to-host copy at all (unseen ids still score ``+inf``).
    """

    def __init__(self, multimodal: "MultiModalSA", device=None, check_unseen: bool = True):
        sas = multimodal.modal_sa
        kinds = {type(sa) for sa in sas.values()}
        if not sas or kinds not in ({MDSA}, {MLSA}):
            raise TypeError(
                "fuse() needs every mode to be an MDSA or every mode to be "
                f"an MLSA, got {sorted(k.__name__ for k in kinds)}"
            )
        self.is_mixture = kinds == {MLSA}
        self.discriminator = multimodal.discriminator
        self.by_class = self.discriminator is _by_class_discriminator
        self.check_unseen = bool(check_unseen)
        modes = sorted(int(m) for m in sas)
        if modes[0] < 0:
            raise ValueError("mode ids must be >= 0")
        if device is None:
            first = getattr(sas[modes[0]], "device", None)
            device = first if first is not None else "cpu"
        self.device = torch.device(device)
        on_gpu = self.device.type == "cuda"

        means, mats, logc, off = [], [], [], [0]
        for m in modes:
            sa = sas[m]
            if self.is_mixture:
                mu = sa.means.detach().cpu().double()
                p = sa.prec_chol.detach().cpu().double()
                d = mu.shape[1]
                means.append(mu)
                mats.append(p @ p.transpose(1, 2))
                logc.append(
                    sa.log_weights.detach().cpu().double()
                    + torch.log(torch.diagonal(p, dim1=1, dim2=2)).sum(dim=1)
                    - 0.5 * d * np.log(2 * np.pi)
                )
                off.append(off[-1] + mu.shape[0])
            else:
                prec = sa.precision.detach().cpu().double()
                means.append(sa.mean.detach().cpu().double().unsqueeze(0))
                # pinv(hermitian=True) is symmetric up to rounding; the
                # kernel reads rows as columns, so make it exact
                mats.append((0.5 * (prec + prec.t())).unsqueeze(0))
                off.append(off[-1] + 1)
        dt = torch.float32 if on_gpu else torch.float64
        self.means = torch.cat(means).to(self.device, dt).contiguous()
        self.mats = torch.cat(mats).to(self.device, dt).contiguous()
        self.logc = (
            torch.cat(logc).to(self.device, dt).contiguous()
            if self.is_mixture
            else None
        )
        self.comp_off = torch.tensor(off, dtype=torch.int32)  # host table
        self.num_groups = len(modes)
        lookup = torch.full((modes[-1] + 1,), -1, dtype=torch.int64)
        lookup[torch.tensor(modes)] = torch.arange(len(modes))
        self.lookup = lookup.to(self.device)
        #: mode id == group id, so a plan made from the ids is a plan of the
        #: groups (the serving path reuses its class plan then)
        self.identity_groups = modes == list(range(len(modes)))
        self._tables = None

    def tables(self, device=None):
        """Validated fp32 device tables of the HIP path (built on first use)."""
        device = torch.device(self.device if device is None else device)
        if self._tables is None or self._tables.device != device:
            from ..ops import hip_ops

            self._tables = hip_ops.GaussianTables(
                self.comp_off, self.means.float(), self.mats.float(),
                None if self.logc is None else self.logc.float(), device,
            )
        return self._tables

    def mode_ids(self, x: torch.Tensor, predictions) -> torch.Tensor:
        """Mode id per row, on ``x``'s device."""
        if self.by_class:
            if x.is_cuda:
                p = predictions
                if not isinstance(p, torch.Tensor):
                    p = torch.as_tensor(np.asarray(p))
                assert p.dim() == 1, "Class predictions must be one-dimensional"
                return p.to(x.device).long()
            return _class_predictions(predictions).to(x.device)
        if isinstance(self.discriminator, _KmeansDiscriminator):
            centers = self.discriminator.best_centers
            return kmeans_predict(x.float(), centers.to(x.device)).long()
        ids = self.discriminator(x, predictions)
        if not isinstance(ids, torch.Tensor):
            ids = torch.as_tensor(np.asarray(ids))
        return ids.to(x.device).long()

    def groups_of(self, ids: torch.Tensor) -> torch.Tensor:
        """Group per mode id (-1 for ids without a fitted mode)."""
        if self.lookup.device != ids.device:
            self.lookup = self.lookup.to(ids.device)  # once per device
        n_ids = self.lookup.shape[0]
        inside = (ids >= 0) & (ids < n_ids)
        return torch.where(
            inside, self.lookup[ids.clamp(0, n_ids - 1)], torch.full_like(ids, -1)
        )

    def _check_unseen(self, ids, group):
        if not self.check_unseen or not bool((group < 0).any()):
            return
        missing = torch.unique(ids[group < 0]).tolist()
        if _STRICT_MODES:
            raise ValueError(
                f"No modal found for modal id {missing[0]} (reference raises here)"
            )
        for modal_id in missing:
            warnings.warn(
                f"No modal found for modal id {modal_id}; scoring those "
                f"inputs as maximally surprising (+inf).",
                UserWarning,
            )

    def __call__(self, activations, predictions=None, num_threads: int = 1):
        acts = _flatten_layers(activations)
        if acts.shape[0] == 0:
            return torch.empty(0)
        if self.device.type == "cuda" or acts.is_cuda:
            dev = acts.device if acts.is_cuda else self.device
            x = acts.to(dev)
            if x.dtype != torch.bfloat16:
                x = x.float()
        else:
            x = acts.double()
        ids = self.mode_ids(x, predictions)
        assert ids.shape[0] == x.shape[0], "discriminator length mismatch"
        group = self.groups_of(ids)
        self._check_unseen(ids, group)
        if ops._route(x) is ops.fallback:
            return ops.fallback.grouped_gaussian_scores(
                x.to(self.mats.dtype), group, self.comp_off,
                self.means.to(x.device), self.mats.to(x.device),
                None if self.logc is None else self.logc.to(x.device),
            )
        from ..ops import hip_ops

        return hip_ops.grouped_gaussian_scores_tables(
            x, group, self.tables(x.device)
        )
