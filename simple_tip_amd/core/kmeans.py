"""KMeans (Lloyd, kmeans++ init) and silhouette score on torch tensors.

Replaces sklearn's KMeans/silhouette_score used by the reference's
``_KmeansDiscriminator`` (src/core/surprise.py:102-133). Both the Lloyd
assignment step and the silhouette score are pairwise-distance problems, so
on MI355X they run on the same MFMA pairwise-sqdist kernel as DSA/KDE
(ops.pairwise_sqdist / ops.rowmin_l2).

Determinism: on CPU every function here is deterministic for a given seed,
and so is the batched path (``kmeans_fit_many`` / ``silhouette_scores_many``)
on the GPU, whose sums have a fixed order. ``kmeans_fit`` on the GPU updates
its centres with ``index_add_``, i.e. float atomic adds, so its centres can
differ from run to run in the last bits.
"""

from typing import Dict, List, Sequence, Tuple

import torch

from .. import ops


def _kmeanspp_init(x: torch.Tensor, k: int, gen: torch.Generator) -> torch.Tensor:
    n = x.shape[0]
    centers = torch.empty(k, x.shape[1], dtype=x.dtype, device=x.device)
    first = int(torch.randint(n, (1,), generator=gen).item())
    centers[0] = x[first]
    d2 = ops.pairwise_sqdist(x, centers[0:1]).squeeze(1).clamp_min_(0)
    for i in range(1, k):
        probs = d2 / d2.sum().clamp_min(1e-30)
        idx = int(torch.multinomial(probs.cpu(), 1, generator=gen).item())
        centers[i] = x[idx]
        nd = ops.pairwise_sqdist(x, centers[i : i + 1]).squeeze(1).clamp_min_(0)
        d2 = torch.minimum(d2, nd)
    return centers


def kmeans_fit(
    x: torch.Tensor,
    k: int,
    n_init: int = 10,
    max_iter: int = 300,
    seed: int = 0,
    tol: float = 1e-4,
) -> Tuple[torch.Tensor, torch.Tensor, float]:
    """Fit k centers; returns (centers, labels, inertia). Best of n_init."""
    gen = torch.Generator().manual_seed(seed)
    best = None
    for _ in range(n_init):
        centers = _kmeanspp_init(x, k, gen)
        for _ in range(max_iter):
            d, labels = ops.rowmin_l2(x, centers)
            new_centers = torch.zeros_like(centers)
            counts = torch.zeros(k, dtype=x.dtype, device=x.device)
            new_centers.index_add_(0, labels, x)
            counts.index_add_(0, labels, torch.ones_like(d))
            empty = counts == 0
            counts = counts.clamp_min(1.0)
            new_centers /= counts.unsqueeze(1)
            # keep empty clusters where they were (sklearn reseeds; rare)
            new_centers[empty] = centers[empty]
            shift = (new_centers - centers).pow(2).sum()
            centers = new_centers
            if float(shift) <= tol:
                break
        d, labels = ops.rowmin_l2(x, centers)
        inertia = float((d * d).sum())
        if best is None or inertia < best[2]:
            best = (centers, labels, inertia)
    return best


def kmeans_predict(x: torch.Tensor, centers: torch.Tensor) -> torch.Tensor:
    """Assign each row of x to its nearest center."""
    _, labels = ops.rowmin_l2(x, centers)
    return labels


def silhouette_score(x: torch.Tensor, labels: torch.Tensor, chunk: int = 2048) -> float:
    """Mean silhouette coefficient over all samples.

    s(i) = (b(i) - a(i)) / max(a(i), b(i)) with a = mean intra-cluster
    distance (excluding self), b = min mean distance to another cluster.
    Computed chunked so the N x N distance matrix never materialises.
    """
    labels = labels.to(x.device)
    k = int(labels.max().item()) + 1
    n = x.shape[0]
    onehot = torch.zeros(n, k, dtype=x.dtype, device=x.device)
    onehot[torch.arange(n, device=x.device), labels] = 1.0
    counts = onehot.sum(dim=0)  # [k]
    s_vals = torch.empty(n, dtype=x.dtype, device=x.device)
    for s0 in range(0, n, chunk):
        xc = x[s0 : s0 + chunk]
        d = ops.pairwise_sqdist(xc, x).clamp_min_(0).sqrt_()  # [c, N]
        sums = d @ onehot  # [c, k] sum of distances to each cluster
        own = labels[s0 : s0 + chunk]
        own_counts = counts[own]
        a = sums[torch.arange(xc.shape[0], device=x.device), own] / (
            own_counts - 1
        ).clamp_min(1.0)
        mean_to = sums / counts.clamp_min(1.0)
        # empty clusters (kmeans_fit can retain a center nobody claims) must
        # not offer b=0 to every sample — sklearn raises on such labelings;
        # masking them to +inf drops them from the min
        mean_to[:, counts == 0] = float("inf")
        mean_to[torch.arange(xc.shape[0], device=x.device), own] = float("inf")
        b = mean_to.min(dim=1).values
        s = (b - a) / torch.maximum(a, b)
        # singleton clusters have s = 0 by convention
        s = torch.where(own_counts > 1, s, torch.zeros_like(s))
        s_vals[s0 : s0 + chunk] = s
    return float(s_vals.mean())


#: Lloyd iterations between two read-backs of the problems still moving
_ACTIVE_POLL = 8


def kmeans_fit_many(
    x: torch.Tensor,
    ks: Sequence[int],
    n_init: int = 10,
    max_iter: int = 300,
    seed: int = 0,
    tol: float = 1e-4,
    stats: dict = None,
) -> Dict[int, Tuple[torch.Tensor, torch.Tensor, float]]:
    """``{k: (centers, labels, inertia)}``, each what
    ``kmeans_fit(x, k, n_init, max_iter, seed, tol)`` returns.

    For each k the ``n_init`` k-means++ seeds are drawn up front from a
    fresh generator (the stream ``kmeans_fit`` sees: Lloyd never touches
    it); then all ``len(ks) * n_init`` problems iterate in lockstep through
    ``ops.lloyd_assign_many`` / ``ops.lloyd_update_many``. The set of
    problems still moving is read back every ``_ACTIVE_POLL`` iterations
    only; a converged problem is left untouched by further updates, so the
    late read changes no result. On CPU the results equal ``kmeans_fit``'s
    exactly; on the GPU they are reproducible from run to run. ``stats``
    (optional dict) receives ``lloyd_iterations``, the updates run.
    """
    ks = [int(k) for k in ks]
    x = x.float().contiguous()
    inits = []
    for k in ks:
        gen = torch.Generator().manual_seed(seed)
        inits += [_kmeanspp_init(x, k, gen) for _ in range(n_init)]
    seg_host = [0]
    for c in inits:
        seg_host.append(seg_host[-1] + c.shape[0])
    centers = torch.cat(inits, dim=0).contiguous()
    seg = torch.tensor(seg_host, dtype=torch.int32, device=x.device)
    active = torch.ones(len(inits), dtype=torch.int32, device=x.device)
    xnorm = ops.row_sqnorms(x)
    # on the host the read is free, and an early stop saves whole assigns
    poll = _ACTIVE_POLL if x.is_cuda else 1
    iters = 0
    while iters < max_iter:
        labels, _ = ops.lloyd_assign_many(x, centers, seg, seg_host, xnorm)
        ops.lloyd_update_many(x, labels, centers, seg, active, tol, seg_host)
        iters += 1
        if iters % poll == 0 and not bool(active.any()):
            break
    if stats is not None:
        stats["lloyd_iterations"] = iters
    labels, mind = ops.lloyd_assign_many(x, centers, seg, seg_host, xnorm)
    # per problem the expression of kmeans_fit; one read-back for all
    inertias = torch.stack(
        [(mind[p] * mind[p]).sum() for p in range(len(inits))]
    ).tolist()
    out = {}
    for i, k in enumerate(ks):
        best = None
        for p in range(i * n_init, (i + 1) * n_init):
            if best is None or inertias[p] < inertias[best]:
                best = p
        out[k] = (
            centers[seg_host[best] : seg_host[best + 1]].clone(),
            labels[best].long(),
            inertias[best],
        )
    return out


def silhouette_scores_many(
    x: torch.Tensor, labels_list: Sequence[torch.Tensor]
) -> List[float]:
    """``[silhouette_score(x, labels) for labels in labels_list]`` from one
    ``ops.silhouette_cluster_sums`` call: the distances are computed once for
    all labelings, the per-row arithmetic of :func:`silhouette_score` is then
    applied to the [N, C] cluster sums."""
    x = x.float().contiguous()
    n = x.shape[0]
    lab = torch.stack([l.to(x.device).long() for l in labels_list])  # [P, N]
    ks = (lab.max(dim=1).values + 1).tolist()
    seg_host = [0]
    for k in ks:
        seg_host.append(seg_host[-1] + int(k))
    seg = torch.tensor(seg_host, dtype=torch.int32, device=x.device)
    sums_all = ops.silhouette_cluster_sums(
        x, lab.to(torch.int32).contiguous(), seg, seg_host
    )
    rows = torch.arange(n, device=x.device)
    means = []
    for p, k in enumerate(ks):
        own = lab[p]
        sums = sums_all[:, seg_host[p] : seg_host[p + 1]]
        onehot = torch.zeros(n, int(k), dtype=x.dtype, device=x.device)
        onehot[rows, own] = 1.0
        counts = onehot.sum(dim=0)
        own_counts = counts[own]
        a = sums[rows, own] / (own_counts - 1).clamp_min(1.0)
        mean_to = sums / counts.clamp_min(1.0)
        # as silhouette_score: empty clusters and the own one leave the min
        mean_to = mean_to.masked_fill((counts == 0).unsqueeze(0), float("inf"))
        mean_to[rows, own] = float("inf")
        b = mean_to.min(dim=1).values
        s = (b - a) / torch.maximum(a, b)
        s = torch.where(own_counts > 1, s, torch.zeros_like(s))
        means.append(s.mean())
    return [float(v) for v in torch.stack(means).tolist()]
