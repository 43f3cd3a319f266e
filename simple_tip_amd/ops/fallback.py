"""Pure torch/numpy reference implementations of every TIP hot-path op.

These serve two purposes:
1. The CPU execution path (this container has no GPU; CI runs here).
2. The numeric oracle the HIP/CDNA4 kernels are tested against
   (tests/test_gpu_*.py compare device results to these).

Bit layout contract (shared with the HIP kernels in simple_tip_amd/ops/hip):
profiles are packed little-endian into 64-bit words — bit ``j`` of word ``w``
of a row is profile column ``w*64 + j``. For multi-section metrics
(KMNC sections, NBC sides) the column index is ``neuron * S + s``, matching
the reference's row-major ``(N, K, S)`` flattening
(reference: src/core/neuron_coverage.py:82-94, 118-128).
"""

from typing import Dict, List, NamedTuple, Tuple

import numpy as np
import torch

# ---------------------------------------------------------------------------
# Bitmap packing / popcount
# ---------------------------------------------------------------------------

_POPCOUNT_U8 = np.array(
    [bin(i).count("1") for i in range(256)], dtype=np.int64
)


def pack_bits(profile: torch.Tensor) -> torch.Tensor:
    """Pack a bool tensor [N, K] into int64 words [N, ceil(K/64)] (LSB-first)."""
    assert profile.dtype == torch.bool and profile.dim() == 2
    arr = profile.cpu().numpy()
    n, k = arr.shape
    w = (k + 63) // 64
    padded = np.zeros((n, w * 64), dtype=np.uint8)
    padded[:, :k] = arr
    # numpy packbits is MSB-first per byte; request little bit order to get
    # our LSB-first contract, then view the 8-byte groups as uint64.
    packed = np.packbits(padded, axis=1, bitorder="little")
    words = packed.view(np.uint64).astype(np.int64, copy=False)
    return torch.from_numpy(np.ascontiguousarray(words)).to(profile.device)


def unpack_bits(words: torch.Tensor, nbits: int) -> torch.Tensor:
    """Inverse of :func:`pack_bits` → bool tensor [N, nbits]."""
    arr = words.cpu().numpy().view(np.uint64).view(np.uint8)
    n = words.shape[0]
    bits = np.unpackbits(arr.reshape(n, -1), axis=1, bitorder="little")
    return torch.from_numpy(bits[:, :nbits].astype(bool)).to(words.device)


def popcount_rows(words: torch.Tensor) -> torch.Tensor:
    """Per-row popcount of packed profiles [N, W] → int64 [N]."""
    arr = words.cpu().numpy().view(np.uint8)
    counts = _POPCOUNT_U8[arr.reshape(words.shape[0], -1)].sum(axis=1)
    return torch.from_numpy(counts).to(words.device)


# ---------------------------------------------------------------------------
# Prioritization orders
# ---------------------------------------------------------------------------


def ctm_order(scores: torch.Tensor) -> torch.Tensor:
    """Coverage-Total Method: indices by descending score, ties by index.

    Reference: src/core/prioritizers.py:7-13 (np.argsort(-scores)).
    """
    assert scores.dim() == 1
    order = torch.argsort(scores, descending=True, stable=True)
    return order


def cam_order(scores: torch.Tensor, words: torch.Tensor, nbits: int) -> torch.Tensor:
    """Coverage-Additional Method over packed profiles.

    Greedy max-cover: repeatedly pick the row covering the most
    still-uncovered columns (first index on ties, like np.argmax), mark those
    columns covered, repeat until no row adds coverage; remaining rows follow
    by descending original score (stable). Semantics match reference
    src/core/prioritizers.py:16-59.
    """
    assert scores.dim() == 1 and words.dim() == 2
    n = scores.shape[0]
    w_np = words.cpu().numpy().view(np.uint64).copy()
    uncovered = np.full(w_np.shape[1], ~np.uint64(0), dtype=np.uint64)
    # zero the padding bits of the last word so `remaining` is exact
    tail = nbits % 64
    if tail:
        uncovered[-1] = np.uint64((1 << tail) - 1)
    num_coverable = _popcount_np(w_np & uncovered)
    remaining = nbits
    yielded = np.zeros(n, dtype=bool)
    order = []
    while True:
        nxt = int(np.argmax(num_coverable))
        newly = int(num_coverable[nxt])
        if newly == 0:
            break
        order.append(nxt)
        yielded[nxt] = True
        newly_mask = w_np[nxt] & uncovered
        num_coverable -= _popcount_np(w_np & newly_mask)
        uncovered &= ~newly_mask
        remaining -= newly
        if remaining == 0:
            break
    # Leftovers: descending original score, stable (ties by index).
    if not np.all(yielded):
        s = scores.cpu().numpy()
        left = np.where(~yielded)[0]
        left = left[np.argsort(-s[left], kind="stable")]
        order.extend(int(i) for i in left)
    return torch.tensor(order, dtype=torch.long, device=scores.device)


def cam_order_many(scores, words, nbits) -> List[torch.Tensor]:
    """:func:`cam_order` of every problem ``(scores[p], words[p], nbits[p])``."""
    scores, words, nbits = list(scores), list(words), list(nbits)
    if not len(scores) == len(words) == len(nbits):
        raise ValueError("scores, words and nbits must have one entry per problem")
    # (a problem without rows has the empty order; cam_order wants a row)
    return [
        cam_order(s, w, int(b))
        if s.shape[0]
        else torch.empty(0, dtype=torch.long, device=s.device)
        for s, w, b in zip(scores, words, nbits)
    ]


def _popcount_np(w: np.ndarray) -> np.ndarray:
    """Row-wise popcount of a 2D uint64 array."""
    assert w.ndim == 2
    return _POPCOUNT_U8[w.view(np.uint8).reshape(w.shape[0], -1)].sum(axis=1)


# ---------------------------------------------------------------------------
# Pairwise distances (DSA / KDE / Mahalanobis / kmeans core)
# ---------------------------------------------------------------------------


def pairwise_sqdist(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """Exact squared L2 distances [N, M] between rows of a [N,D] and b [M,D]."""
    d = torch.cdist(
        a.unsqueeze(0), b.unsqueeze(0), compute_mode="donot_use_mm_for_euclid_dist"
    ).squeeze(0)
    return d * d


def rowmin_l2(
    a: torch.Tensor, b: torch.Tensor, bnorm: torch.Tensor = None, chunk: int = 4096
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Per-row (min L2 distance, argmin) from rows of a to rows of b.

    Ties resolve to the lowest b-index (np.argmin semantics).
    """
    mins = torch.empty(a.shape[0], dtype=a.dtype, device=a.device)
    args = torch.empty(a.shape[0], dtype=torch.long, device=a.device)
    for s in range(0, a.shape[0], chunk):
        d = torch.cdist(
            a[s : s + chunk].unsqueeze(0),
            b.unsqueeze(0),
            compute_mode="donot_use_mm_for_euclid_dist",
        ).squeeze(0)
        m, idx = d.min(dim=1)
        mins[s : s + chunk] = m
        args[s : s + chunk] = idx
    return mins, args


def kde_logsumexp(
    test_w: torch.Tensor, train_w: torch.Tensor, chunk: int = 2048
) -> torch.Tensor:
    """logsumexp_i(-0.5 * ||t - x_i||^2) per test row, over whitened coords.

    The Gaussian-KDE hot loop: with both sides whitened by the bandwidth
    Cholesky factor, the kernel sum is a pairwise-sqdist + logsumexp epilogue
    (reference equivalent: scipy gaussian_kde.evaluate via
    src/core/stable_kde.py:79-101, computed there in float64 without the
    log-domain stabilisation we add here).
    """
    out = torch.empty(test_w.shape[0], dtype=test_w.dtype, device=test_w.device)
    for s in range(0, test_w.shape[0], chunk):
        d2 = pairwise_sqdist(test_w[s : s + chunk], train_w)
        out[s : s + chunk] = torch.logsumexp(-0.5 * d2, dim=1)
    return out


# ---------------------------------------------------------------------------
# Softmax-family uncertainty scores
# ---------------------------------------------------------------------------


def softmax_uncertainties(probs: torch.Tensor) -> Dict[str, torch.Tensor]:
    """All point-prediction uncertainty scores from softmax outputs [N, C].

    Naming and sign conventions follow the reference artifacts
    (uncertainty-wizard quantifiers with ``as_confidence=False`` negate
    confidence-type scores; reference handler_model.py:23-86,133-139 and
    plotters/utils.py approach names):
      - ``softmax``          = -max(p)              (negated MaxSoftmax)
      - ``pcs``              = -(p_top1 - p_top2)   (negated PredConfidence)
      - ``softmax_entropy``  = -sum p log p         (natural log; 0 log 0 = 0)
      - ``deep_gini``        = 1 - sum p^2          (reference deepgini.py:32-35)
    """
    top2 = torch.topk(probs, k=min(2, probs.shape[1]), dim=1).values
    p1 = top2[:, 0]
    p2 = top2[:, 1] if probs.shape[1] > 1 else torch.zeros_like(p1)
    logp = torch.where(probs > 0, torch.log(probs), torch.zeros_like(probs))
    entropy = -(probs * logp).sum(dim=1)
    gini = 1.0 - (probs * probs).sum(dim=1)
    return {
        "softmax": -p1,
        "pcs": -(p1 - p2),
        "softmax_entropy": entropy,
        "deep_gini": gini,
    }


def variation_ratio(sample_preds: torch.Tensor, num_classes: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """MC-dropout variation ratio from sampled class predictions [S, N].

    Returns (mode prediction, 1 - mode_count/S). Ties resolve to the lowest
    class index.
    """
    s, n = sample_preds.shape
    onehot = torch.zeros(n, num_classes, dtype=torch.float32, device=sample_preds.device)
    onehot.scatter_add_(
        1,
        sample_preds.t().long(),
        torch.ones(n, s, dtype=torch.float32, device=sample_preds.device),
    )
    counts, mode = onehot.max(dim=1)
    vr = 1.0 - counts / float(s)
    return mode, vr


# ---------------------------------------------------------------------------
# Fused MC-dropout head (variation-ratio votes)
# ---------------------------------------------------------------------------

_M32 = 0xFFFFFFFF
# cap on mask elements materialised at once by mc_dropout_votes (the hash
# runs on int64 temporaries, so 16M elements is ~128 MiB per temporary)
_MCD_MAX_MASK_ELEMS = 16 * 1024 * 1024


def _mix32(x: torch.Tensor) -> torch.Tensor:
    """32-bit finalizer on int64 tensors holding values in [0, 2^32)."""
    x = x ^ (x >> 16)
    x = (x * 0x7FEB352D) & _M32
    x = x ^ (x >> 15)
    x = (x * 0x846CA68B) & _M32
    x = x ^ (x >> 16)
    return x


def dropout_threshold(p: float) -> int:
    """T = floor(p * 2^32) in float64; an element is kept iff word >= T."""
    if not 0.0 <= p < 1.0:
        raise ValueError(f"dropout probability must be in [0, 1), got {p}")
    return int(float(p) * 4294967296.0)


def dropout_scale(p: float) -> float:
    """1 / (1 - p) rounded to float32 (returned as an exact python float)."""
    return float(np.float32(1.0 / (1.0 - float(p))))


def dropout_words(
    seed: int, S: int, N: int, D: int, row_offset: int = 0
) -> torch.Tensor:
    """The stateless generator's 32-bit words, int64 [S, N, D].

    All arithmetic is unsigned 32-bit (wrapping), carried in int64 tensors
    masked to 32 bits::

        r    = mix32(mix32(mix32(g + 0x6A09E667) ^ lo) ^ hi)    g = row_offset + n
        key  = mix32(r + s * 0x9E3779B9)
        word = mix32(key ^ (d * 0x85EBCA6B))
    """
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    lo, hi = seed & _M32, seed >> 32
    g = (torch.arange(N, dtype=torch.int64) + int(row_offset)) & _M32
    r = _mix32((g + 0x6A09E667) & _M32)
    r = _mix32(r ^ lo)
    r = _mix32(r ^ hi)
    s = torch.arange(S, dtype=torch.int64)
    key = _mix32((r[None, :] + ((s * 0x9E3779B9) & _M32)[:, None]) & _M32)
    d = (torch.arange(D, dtype=torch.int64) * 0x85EBCA6B) & _M32
    return _mix32(key[:, :, None] ^ d[None, None, :])


def dropout_keep_mask(
    seed: int, S: int, N: int, D: int, p: float, row_offset: int = 0
) -> torch.Tensor:
    """Keep mask of the MC-dropout head, bool [S, N, D] (True = kept).

    Depends only on (seed, sample, global row, feature) — never on batch
    size or sharding. The HIP kernel generates the same bits in registers.
    """
    return dropout_words(seed, S, N, D, row_offset) >= dropout_threshold(p)


def _mc_dropout_eval(feats, weight, bias, p, num_samples, seed, row_offset,
                     with_stats: bool):
    """Shared body of mc_dropout_votes / mc_dropout_stats (CPU tensors out).

    Returns ``(votes int32 [N, C], mean_probs float64 [N, C] | None,
    mean_entropy float64 [N] | None)``. The logits are float32 (``scale``
    applied once after the sum, then the bias); the statistics are computed
    from those float32 logits in float64.
    """
    n, d = feats.shape
    c = weight.shape[0]
    S = int(num_samples)
    if not 1 <= S <= 65535:
        raise ValueError(f"num_samples must be in [1, 65535], got {S}")
    if row_offset < 0 or row_offset + n > 2 ** 32:
        raise ValueError("rows must satisfy row_offset + N <= 2^32")
    thresh = dropout_threshold(p)
    scale = dropout_scale(p)
    f = feats.detach().float().cpu()
    wt = weight.detach().float().cpu().t().contiguous()
    b = bias.detach().float().cpu()
    votes = torch.zeros(n, c, dtype=torch.int32)
    mean_probs = torch.zeros(n, c, dtype=torch.float64) if with_stats else None
    mean_entropy = torch.zeros(n, dtype=torch.float64) if with_stats else None
    rows = max(1, _MCD_MAX_MASK_ELEMS // max(1, S * d))
    ones = torch.ones(1, dtype=torch.int32)
    cls = torch.arange(c, dtype=torch.int64)
    for s0 in range(0, n, rows):
        fb = f[s0 : s0 + rows]
        nb = fb.shape[0]
        keep = dropout_words(seed, S, nb, d, row_offset + s0) >= thresh
        sums = torch.matmul(keep.to(torch.float32) * fb[None], wt)  # [S,nb,C]
        logits = scale * sums + b
        # first maximal index (torch.argmax does not promise one on ties)
        is_max = logits == logits.max(dim=2, keepdim=True).values
        best = torch.where(is_max, cls, c).min(dim=2).values  # [S, nb]
        best.clamp_(max=c - 1)  # NaN logits match nothing; keep the index valid
        votes[s0 : s0 + nb].scatter_add_(
            1, best.t().contiguous(), ones.expand(nb, S)
        )
        if with_stats:
            v = logits.double()
            v = v - v.max(dim=2, keepdim=True).values
            e = torch.exp(v)
            z = e.sum(dim=2, keepdim=True)
            probs = e / z
            # H = log Z - sum_c p_c (v_c - max); 0 * finite = 0 where p == 0
            ent = torch.log(z.squeeze(2)) - (probs * v).sum(dim=2)  # [S, nb]
            mean_probs[s0 : s0 + nb] = probs.mean(dim=0)
            mean_entropy[s0 : s0 + nb] = ent.mean(dim=0)
    return votes, mean_probs, mean_entropy


def mc_dropout_votes(
    feats: torch.Tensor,
    weight: torch.Tensor,
    bias: torch.Tensor,
    p: float,
    num_samples: int,
    seed: int,
    row_offset: int = 0,
) -> torch.Tensor:
    """Argmax votes of ``num_samples`` dropout-masked linear heads, int32 [N, C].

    ``logit[c] = scale * sum_d keep*feats[n,d]*weight[c,d] + bias[c]`` with
    ``scale = 1/(1-p)`` (float32) applied once after the sum; the vote goes
    to the lowest index among the maximal logits. Inputs must be finite
    (votes of a row with NaN/inf logits are unspecified). Rows are processed
    in chunks so only ``_MCD_MAX_MASK_ELEMS`` mask elements exist at a time.
    """
    votes, _, _ = _mc_dropout_eval(
        feats, weight, bias, p, num_samples, seed, row_offset, with_stats=False
    )
    return votes.to(feats.device)


def _mc_dropout_stats_f64(
    feats, weight, bias, p, num_samples, seed, row_offset=0
) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(votes int32, mean_probs float64, mean_entropy float64) on the CPU:
    the unrounded values behind :func:`mc_dropout_stats`, for tests."""
    return _mc_dropout_eval(
        feats, weight, bias, p, num_samples, seed, row_offset, with_stats=True
    )


def mc_dropout_stats(
    feats: torch.Tensor,
    weight: torch.Tensor,
    bias: torch.Tensor,
    p: float,
    num_samples: int,
    seed: int,
    row_offset: int = 0,
) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Votes, mean softmax and mean per-sample entropy of the masked heads.

    Returns ``(votes int32 [N, C], mean_probs float32 [N, C], mean_entropy
    float32 [N])``. The float32 logits are those of :func:`mc_dropout_votes`
    (so are the votes); softmax, entropy (natural log, ``p log p = 0`` at
    ``p = 0``) and the two means over the samples are evaluated from them in
    float64 and rounded to float32 once at the end. Same row chunking as
    :func:`mc_dropout_votes`.
    """
    votes, mean_probs, mean_entropy = _mc_dropout_stats_f64(
        feats, weight, bias, p, num_samples, seed, row_offset
    )
    dev = feats.device
    return votes.to(dev), mean_probs.float().to(dev), mean_entropy.float().to(dev)


# ---------------------------------------------------------------------------
# Fused MC-dropout transformer tail (four dropout sites)
# ---------------------------------------------------------------------------


class McTransformerParams(NamedTuple):
    """The tensors of a post-LN transformer block's stochastic tail.

    ``w1 [F, E]``/``b1`` and ``w2 [E, F]``/``b2`` are the feed-forward pair,
    ``w3 [H, E]``/``b3`` the hidden Dense and ``w4 [C, H]``/``b4`` the output
    Dense; both LayerNorms share ``eps`` (a python float)."""

    ln1_w: torch.Tensor
    ln1_b: torch.Tensor
    w1: torch.Tensor
    b1: torch.Tensor
    w2: torch.Tensor
    b2: torch.Tensor
    ln2_w: torch.Tensor
    ln2_b: torch.Tensor
    eps: float
    w3: torch.Tensor
    b3: torch.Tensor
    w4: torch.Tensor
    b4: torch.Tensor


def mc_transformer_dims(x, attn, params) -> Tuple[int, int, int, int, int, int]:
    """``(N, T, E, F, H, C)`` of a tail call; ValueError on a shape mismatch."""
    if x.dim() != 3 or attn.shape != x.shape:
        raise ValueError("expected x and attn of one shape [N, T, E]")
    n, t, e = x.shape
    if params.w1.dim() != 2 or params.w3.dim() != 2 or params.w4.dim() != 2:
        raise ValueError("w1, w3 and w4 must be 2-D")
    f, h, c = params.w1.shape[0], params.w3.shape[0], params.w4.shape[0]
    want = {
        "ln1_w": (e,), "ln1_b": (e,), "w1": (f, e), "b1": (f,),
        "w2": (e, f), "b2": (e,), "ln2_w": (e,), "ln2_b": (e,),
        "w3": (h, e), "b3": (h,), "w4": (c, h), "b4": (c,),
    }
    for name, shape in want.items():
        got = tuple(getattr(params, name).shape)
        if got != shape:
            raise ValueError(f"params.{name} must be {shape}, got {got}")
    if min(t, e, f, h, c) < 1:
        raise ValueError("T, E, F, H and C must be at least 1")
    return n, t, e, f, h, c


def _mc_transformer_rates(p) -> Tuple[float, float, float, float]:
    p = tuple(float(v) for v in p)
    if len(p) != 4:
        raise ValueError("p must hold the four rates (attn, ffn, pool, hidden)")
    return p


def mc_transformer_masks(
    seed: int, S: int, N: int, T: int, E: int, H: int, p, row_offset: int = 0
) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """Keep masks of the four dropout sites, bool ``[S, N, T, E]``,
    ``[S, N, T, E]``, ``[S, N, E]`` and ``[S, N, H]``.

    The sites share the flat element axis of one :func:`dropout_words` call
    of length ``2*T*E + E + H``: the attention dropout at ``t*E + e``, the
    feed-forward dropout at ``T*E + t*E + e``, the pooled dropout at
    ``2*T*E + e`` and the hidden dropout at ``2*T*E + E + h``."""
    p = _mc_transformer_rates(p)
    te = T * E
    words = dropout_words(seed, S, N, 2 * te + E + H, row_offset)
    th = [dropout_threshold(v) for v in p]
    return (
        (words[:, :, :te] >= th[0]).reshape(S, N, T, E),
        (words[:, :, te : 2 * te] >= th[1]).reshape(S, N, T, E),
        words[:, :, 2 * te : 2 * te + E] >= th[2],
        words[:, :, 2 * te + E :] >= th[3],
    )


def _layer_norm(v, w, b, eps):
    """LayerNorm over the last axis with the biased variance."""
    d = v - v.mean(dim=-1, keepdim=True)
    var = (d * d).mean(dim=-1, keepdim=True)
    return d / torch.sqrt(var + eps) * w + b


def _mc_transformer_logits(x, attn, q, masks, scales) -> torch.Tensor:
    """Logits [S, N, C] of the masked tails in the dtype of ``x``: ``x`` and
    ``attn`` [N, T, E], ``masks`` the four keep masks of
    :func:`mc_transformer_masks`, ``scales`` the four ``dropout_scale``."""
    lin = torch.nn.functional.linear
    dtype = x.dtype
    k1, k2, k3, k4 = masks
    hid = _layer_norm(
        x[None] + (k1.to(dtype) * scales[0]) * attn[None],
        q.ln1_w, q.ln1_b, q.eps,
    )  # [S, N, T, E]
    ffn = lin(torch.relu(lin(hid, q.w1, q.b1)), q.w2, q.b2)
    y = _layer_norm(
        hid + (k2.to(dtype) * scales[1]) * ffn, q.ln2_w, q.ln2_b, q.eps
    )
    g = y.mean(dim=2)  # [S, N, E]
    z = torch.relu(lin((k3.to(dtype) * scales[2]) * g, q.w3, q.b3))
    return lin((k4.to(dtype) * scales[3]) * z, q.w4, q.b4)


def _mc_transformer_eval(x, attn, params, p, num_samples, seed, row_offset,
                         with_stats: bool, dtype=torch.float32):
    """Shared body of mc_transformer_votes / mc_transformer_stats.

    Returns ``(votes int32 [N, C], mean_probs float64 [N, C] | None,
    mean_entropy float64 [N] | None)`` on the CPU. The logits are evaluated
    in ``dtype``; the statistics are computed from them in float64. A site's
    dropout is ``v + scale * keep * u`` with ``scale * keep`` exact, so the
    product and the sum are rounded separately.
    """
    n, t, e, f, h, c = mc_transformer_dims(x, attn, params)
    S = int(num_samples)
    if not 1 <= S <= 65535:
        raise ValueError(f"num_samples must be in [1, 65535], got {S}")
    if row_offset < 0 or row_offset + n > 2 ** 32:
        raise ValueError("rows must satisfy row_offset + N <= 2^32")
    p = _mc_transformer_rates(p)
    for v in p:
        dropout_threshold(v)  # range check
    sc = [dropout_scale(v) for v in p]

    def cpu(v):
        return v.detach().to("cpu", dtype)

    xs, at = cpu(x), cpu(attn)
    q = McTransformerParams(*[
        float(v) if name == "eps" else cpu(v)
        for name, v in zip(McTransformerParams._fields, params)
    ])
    votes = torch.zeros(n, c, dtype=torch.int32)
    mean_probs = torch.zeros(n, c, dtype=torch.float64) if with_stats else None
    mean_entropy = torch.zeros(n, dtype=torch.float64) if with_stats else None
    dtot = 2 * t * e + e + h
    rows = max(1, _MCD_MAX_MASK_ELEMS // max(1, S * dtot))
    ones = torch.ones(1, dtype=torch.int32)
    cls = torch.arange(c, dtype=torch.int64)
    for s0 in range(0, n, rows):
        xb, ab = xs[s0 : s0 + rows], at[s0 : s0 + rows]
        nb = xb.shape[0]
        k1, k2, k3, k4 = mc_transformer_masks(
            seed, S, nb, t, e, h, p, row_offset + s0
        )
        logits = _mc_transformer_logits(xb, ab, q, (k1, k2, k3, k4), sc)
        is_max = logits == logits.max(dim=2, keepdim=True).values
        best = torch.where(is_max, cls, c).min(dim=2).values  # [S, nb]
        best.clamp_(max=c - 1)
        votes[s0 : s0 + nb].scatter_add_(
            1, best.t().contiguous(), ones.expand(nb, S)
        )
        if with_stats:
            v = logits.double()
            v = v - v.max(dim=2, keepdim=True).values
            ex = torch.exp(v)
            zsum = ex.sum(dim=2, keepdim=True)
            probs = ex / zsum
            ent = torch.log(zsum.squeeze(2)) - (probs * v).sum(dim=2)
            mean_probs[s0 : s0 + nb] = probs.mean(dim=0)
            mean_entropy[s0 : s0 + nb] = ent.mean(dim=0)
    return votes, mean_probs, mean_entropy


def mc_transformer_votes(
    x: torch.Tensor,
    attn: torch.Tensor,
    params: McTransformerParams,
    p,
    num_samples: int,
    seed: int,
    row_offset: int = 0,
) -> torch.Tensor:
    """Argmax votes of ``num_samples`` dropout-masked transformer tails,
    int32 [N, C]: float32 logits from torch ops over row chunks of at most
    ``_MCD_MAX_MASK_ELEMS`` mask elements; the vote goes to the lowest index
    among the maximal logits."""
    votes, _, _ = _mc_transformer_eval(
        x, attn, params, p, num_samples, seed, row_offset, with_stats=False
    )
    return votes.to(x.device)


def _mc_transformer_stats_f64(
    x, attn, params, p, num_samples, seed, row_offset=0
) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(votes int32, mean_probs float64, mean_entropy float64) with the
    whole tail, the logits included, evaluated in float64; for tests."""
    return _mc_transformer_eval(
        x, attn, params, p, num_samples, seed, row_offset, with_stats=True,
        dtype=torch.float64,
    )


def mc_transformer_stats(
    x: torch.Tensor,
    attn: torch.Tensor,
    params: McTransformerParams,
    p,
    num_samples: int,
    seed: int,
    row_offset: int = 0,
) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Votes, mean softmax and mean per-sample entropy of the masked tails:
    the float32 logits (and votes) of :func:`mc_transformer_votes`, the
    statistics from them in float64, rounded to float32 once."""
    votes, mean_probs, mean_entropy = _mc_transformer_eval(
        x, attn, params, p, num_samples, seed, row_offset, with_stats=True
    )
    dev = x.device
    return votes.to(dev), mean_probs.float().to(dev), mean_entropy.float().to(dev)


# ---------------------------------------------------------------------------
# Coverage profiling (bool → packed bitmaps)
# ---------------------------------------------------------------------------


def nac_profile(acts: torch.Tensor, threshold: float) -> torch.Tensor:
    """NAC: bit per neuron, set iff activation > threshold. Returns packed."""
    return pack_bits(acts > threshold)


def snac_profile(acts: torch.Tensor, max_bound: torch.Tensor) -> torch.Tensor:
    """SNAC: activation >= max + scaler*std (bound precomputed)."""
    return pack_bits(acts >= max_bound)


def nbc_profile(
    acts: torch.Tensor, min_bound: torch.Tensor, max_bound: torch.Tensor
) -> torch.Tensor:
    """NBC: two bits per neuron — a <= min_bound, a >= max_bound.

    Column layout: ``neuron*2 + side`` (side 0 = lower, 1 = upper).
    """
    lower = acts <= min_bound
    upper = acts >= max_bound
    prof = torch.stack([lower, upper], dim=2).reshape(acts.shape[0], -1)
    return pack_bits(prof)


def kmnc_profile(
    acts: torch.Tensor, mins: torch.Tensor, maxs: torch.Tensor, sections: int
) -> torch.Tensor:
    """KMNC: per-neuron k-section membership bits (column = neuron*S + s).

    Section s covers [min + jump*s, min + jump*(s+1)); values equal to max or
    outside [min, max) set no bit — matching reference
    neuron_coverage.py:82-94.
    """
    n, k = acts.shape
    jumps = (maxs - mins) / sections
    prof = torch.zeros(n, k, sections, dtype=torch.bool, device=acts.device)
    for s in range(sections):
        lo = mins + jumps * s
        hi = mins + jumps * (s + 1)
        prof[..., s] = (lo <= acts) & (acts < hi)
    return pack_bits(prof.reshape(n, -1))


def tknc_profile(layer_acts, k: int) -> torch.Tensor:
    """TKNC: per layer, bit set for each of the layer's top-k neurons.

    ``layer_acts`` is a list of [N, K_l] tensors; columns are the flattened
    concatenation of layers (reference neuron_coverage.py:155-167).

    The order is total, and the HIP kernel holds to the same one: descending
    value with NaN greatest, then ascending column. Post-ReLU rows are
    mostly exact zeros, so ties at the cut are the normal case; the
    reference's argsort and ``torch.topk`` both leave them unspecified, a
    stable descending sort does not.
    """
    parts = []
    for layer in layer_acts:
        flat = layer.reshape(layer.shape[0], -1)
        kk = min(k, flat.shape[1])
        idx = torch.sort(flat, dim=1, descending=True, stable=True).indices[:, :kk]
        prof = torch.zeros_like(flat, dtype=torch.bool)
        prof.scatter_(1, idx, True)
        parts.append(prof)
    return pack_bits(torch.cat(parts, dim=1))


#: profile families of :func:`coverage_suite`, in output order
COVERAGE_SUITE_FAMILIES = ("nac", "snac", "nbc", "kmnc", "tknc")


def coverage_suite(
    layers,
    nac_thresholds=(),
    upper_bounds=None,
    nbc_lower=None,
    nbc_upper=None,
    kmnc_mins=None,
    kmnc_maxs=None,
    kmnc_sections=(),
    tknc_ks=(),
):
    """Every requested coverage profile of one batch of tapped layers.

    ``layers`` is a list of [N, K_l] tensors; the neuron axis of every table
    is their concatenation order. Returns ``{family: [(words, scores), ...]}``
    for the families ``nac`` (one entry per threshold), ``snac`` (per row of
    ``upper_bounds`` [U, K]), ``nbc`` (per row of ``nbc_lower`` /
    ``nbc_upper`` [B, K]), ``kmnc`` (per entry of ``kmnc_sections``) and
    ``tknc`` (per entry of ``tknc_ks``), with ``scores`` the popcount of
    ``words``. This composes the per-metric functions above, so it defines
    what the fused HIP op must return word for word.
    """
    layers = [l.reshape(l.shape[0], -1) for l in layers]
    acts = torch.cat(layers, dim=1)

    def entry(words):
        return words, popcount_rows(words)

    out = {f: [] for f in COVERAGE_SUITE_FAMILIES}
    for thr in nac_thresholds:
        out["nac"].append(entry(nac_profile(acts, float(thr))))
    for u in range(0 if upper_bounds is None else upper_bounds.shape[0]):
        out["snac"].append(entry(snac_profile(acts, upper_bounds[u])))
    for b in range(0 if nbc_lower is None else nbc_lower.shape[0]):
        out["nbc"].append(entry(nbc_profile(acts, nbc_lower[b], nbc_upper[b])))
    for sections in kmnc_sections:
        out["kmnc"].append(
            entry(kmnc_profile(acts, kmnc_mins, kmnc_maxs, int(sections)))
        )
    for k in tknc_ks:
        out["tknc"].append(entry(tknc_profile(layers, int(k))))
    return out


def bucketize_profile(values: torch.Tensor, thresholds: torch.Tensor) -> torch.Tensor:
    """Surprise-coverage binning: bit s set iff thr[s] <= v < thr[s+1].

    ``thresholds`` has S+1 entries; values outside [thr[0], thr[S]) (including
    v == thr[S] exactly) set no bit — matching reference surprise.py:186-209.
    """
    s = thresholds.shape[0] - 1
    idx = torch.searchsorted(thresholds, values.to(thresholds.dtype), right=True) - 1
    valid = (idx >= 0) & (idx < s)
    # note: searchsorted(right=True) maps v == thr[i] to bucket i, and
    # v == thr[S] to S (invalid) — the reference's half-open intervals.
    prof = torch.zeros(values.shape[0], s, dtype=torch.bool)
    rows = torch.nonzero(valid, as_tuple=True)[0]
    prof[rows, idx[valid]] = True
    return pack_bits(prof).to(values.device)


# ---------------------------------------------------------------------------
# Segment plan (sync-free grouped scoring)
# ---------------------------------------------------------------------------

SEGMENT_ROWS = 128


def segment_plan_rows(batch: int, num_classes: int) -> int:
    """Static bound on the sum of the 128-padded class counts."""
    return SEGMENT_ROWS * ((batch + SEGMENT_ROWS - 1) // SEGMENT_ROWS + num_classes)


def segment_plan(
    pred: torch.Tensor, num_classes: int
) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Class-sorted, 128-padded layout of a batch as an index plan.

    Returns ``(tseg int32[C+1], rowmap int32[bp_max], dest int32[B])``:
    ``tseg`` are the padded segment offsets, ``rowmap[p]`` the input row at
    padded row ``p`` (-1 for pad rows and rows >= ``tseg[C]``) and ``dest[i]``
    the padded row of input ``i``. Inside a class inputs keep ascending
    index order (stable sort). A prediction outside ``[0, C)`` gets
    ``dest = -1`` and appears nowhere in ``rowmap``. Reference for the HIP
    ``segment_plan`` kernel, which must equal it exactly.
    """
    assert pred.dim() == 1
    p = pred.to(torch.int64)
    b = p.shape[0]
    valid = (p >= 0) & (p < num_classes)
    counts = torch.bincount(p[valid], minlength=num_classes)
    padded = (counts + SEGMENT_ROWS - 1) // SEGMENT_ROWS * SEGMENT_ROWS
    tseg = torch.zeros(num_classes + 1, dtype=torch.int64, device=p.device)
    tseg[1:] = torch.cumsum(padded, 0)
    starts = torch.zeros(num_classes, dtype=torch.int64, device=p.device)
    starts[1:] = torch.cumsum(counts, 0)[:-1]
    rows = torch.nonzero(valid, as_tuple=True)[0]
    order = rows[torch.argsort(p[rows], stable=True)]
    cls = p[order]
    intra = torch.arange(order.shape[0], device=p.device) - starts[cls]
    where = tseg[cls] + intra
    rowmap = torch.full(
        (segment_plan_rows(b, num_classes),), -1, dtype=torch.int32, device=p.device
    )
    rowmap[where] = order.to(torch.int32)
    dest = torch.full((b,), -1, dtype=torch.int32, device=p.device)
    dest[order] = where.to(torch.int32)
    return tseg.to(torch.int32), rowmap, dest


# ---------------------------------------------------------------------------
# Grouped Gaussian scoring (pc-MDSA / pc-MLSA / pc-MMDSA)
# ---------------------------------------------------------------------------

GAUSS_MAX_GROUPS = 256  # what one segment plan addresses
GAUSS_MAX_SLOTS = 8     # components per group


def gaussian_check_envelope(comp_off, means, mats, logc):
    """Validate grouped-Gaussian tables; returns ``(G, J, D, max_slots)``.

    ``comp_off`` is read on the host (it is a fit-time table, so this is done
    once per table set, not per call). Raises ValueError outside the
    envelope: more than 256 groups, more than 8 components in a group, a
    non-contiguous ``mats``, or Mahalanobis mode (``logc is None``) with a
    group that does not have exactly one component.
    """
    if means.dim() != 2 or mats.dim() != 3:
        raise ValueError("expected means [J, D] and mats [J, D, D]")
    J, D = means.shape
    if tuple(mats.shape) != (J, D, D):
        raise ValueError(f"mats must be [{J}, {D}, {D}], got {tuple(mats.shape)}")
    if not mats.is_contiguous():
        raise ValueError("mats must be contiguous")
    off = torch.as_tensor(comp_off).detach().cpu().to(torch.int64)
    if off.dim() != 1 or off.numel() < 2:
        raise ValueError("comp_off must be [G+1] with G >= 1")
    G = off.numel() - 1
    if G > GAUSS_MAX_GROUPS:
        raise ValueError(
            f"grouped_gaussian_scores supports up to {GAUSS_MAX_GROUPS} "
            f"groups (got {G})"
        )
    counts = off[1:] - off[:-1]
    if int(off[0]) != 0 or int(off[-1]) != J or bool((counts < 0).any()):
        raise ValueError("comp_off must ascend from 0 to J")
    smax = int(counts.max())
    if smax > GAUSS_MAX_SLOTS:
        raise ValueError(
            f"grouped_gaussian_scores supports up to {GAUSS_MAX_SLOTS} "
            f"components per group (got {smax})"
        )
    if logc is None:
        if bool((counts != 1).any()):
            raise ValueError(
                "Mahalanobis mode (logc=None) needs exactly one component "
                "per group"
            )
    elif logc.dim() != 1 or logc.shape[0] != J:
        raise ValueError("logc must be [J]")
    return G, J, D, smax


def grouped_gaussian_scores(
    x: torch.Tensor,
    group: torch.Tensor,
    comp_off: torch.Tensor,
    means: torch.Tensor,
    mats: torch.Tensor,
    logc: torch.Tensor = None,
) -> torch.Tensor:
    """Per-row Gaussian score of ``x[n]`` under the components of group
    ``group[n]`` (components ``comp_off[g] .. comp_off[g+1]``).

    With ``q_j(x) = (x - mu_j)^T M_j (x - mu_j)``: ``logc is None`` gives the
    Mahalanobis form ``q`` of the group's single component, otherwise the
    mixture NLL ``-logsumexp_j(logc_j - q_j / 2)``. Rows whose group id is
    outside ``[0, G)`` and rows of a group without components score ``+inf``.
    Computes in the dtype of ``mats`` (a float64 call is the test oracle of
    the HIP kernels) and returns that dtype.
    """
    G, J, D, smax = gaussian_check_envelope(comp_off, means, mats, logc)
    dt = mats.dtype
    dev = x.device
    if x.dim() != 2 or x.shape[1] != D:
        raise ValueError(f"x must be [N, {D}]")
    xs = x.to(dt)
    mu = means.to(dev, dt)
    mm = mats.to(dev)
    lc = None if logc is None else logc.to(dev, dt)
    grp = group.to(dev, torch.int64)
    off = torch.as_tensor(comp_off).cpu().to(torch.int64).tolist()
    n = xs.shape[0]
    # t[n, s]: log-term of slot s (or q itself in Mahalanobis mode)
    t = torch.full((n, max(smax, 1)), -float("inf"), dtype=dt, device=dev)
    for g in range(G):
        rows = torch.nonzero(grp == g, as_tuple=True)[0]
        if rows.numel() == 0:
            continue
        for s, j in enumerate(range(off[g], off[g + 1])):
            d = xs[rows] - mu[j]
            q = ((d @ mm[j]) * d).sum(dim=1)
            t[rows, s] = q if lc is None else lc[j] - 0.5 * q
    if lc is None:
        out = t[:, 0].clone()
        out[torch.isneginf(out)] = float("inf")  # unplaced / empty group
        return out
    return -torch.logsumexp(t, dim=1)


# ---------------------------------------------------------------------------
# Batched k-means: P problems over the same rows, centres stacked
# ---------------------------------------------------------------------------


def kmeans_many_segments(seg, seg_host=None) -> List[int]:
    """The host list of ``seg`` (int32 [P+1], problem p owns stacked centres
    ``seg[p] .. seg[p+1]``), validated: starts at 0 and strictly ascending.
    ``seg_host`` is the caller's own host copy, which saves reading a device
    ``seg`` back."""
    if not isinstance(seg, torch.Tensor) or seg.dtype != torch.int32 or seg.dim() != 1:
        raise ValueError("seg must be an int32 [P+1] tensor")
    s = [int(v) for v in (seg.cpu().tolist() if seg_host is None else seg_host)]
    if len(s) != seg.shape[0] or len(s) < 2:
        raise ValueError("seg must hold P+1 >= 2 offsets")
    if s[0] != 0 or any(b <= a for a, b in zip(s, s[1:])):
        raise ValueError(f"seg must start at 0 and ascend strictly (got {s})")
    return s


def _kmeans_many_check(x, seg_list, labels=None, centers=None, active=None):
    """Argument checks shared by the CPU and the GPU implementations."""
    if x.dim() != 2 or x.dtype != torch.float32 or not x.is_contiguous():
        raise ValueError("x must be a contiguous float32 [N, D] tensor")
    n, d = x.shape
    p, c = len(seg_list) - 1, seg_list[-1]
    if n < 1 or d < 1:
        raise ValueError("x must have at least one row and one column")
    if centers is not None:
        if (
            centers.dim() != 2
            or centers.dtype != torch.float32
            or not centers.is_contiguous()
            or tuple(centers.shape) != (c, d)
        ):
            raise ValueError(
                f"centers must be a contiguous float32 [{c}, {d}] tensor "
                f"(got {centers.dtype}, shape {tuple(centers.shape)})"
            )
    if labels is not None:
        if (
            labels.dtype != torch.int32
            or not labels.is_contiguous()
            or tuple(labels.shape) != (p, n)
        ):
            raise ValueError(f"labels must be a contiguous int32 [{p}, {n}] tensor")
    if active is not None:
        if (
            active.dtype != torch.int32
            or not active.is_contiguous()
            or tuple(active.shape) != (p,)
        ):
            raise ValueError(f"active must be a contiguous int32 [{p}] tensor")
    return n, d, p, c


def _same_device(x, **others):
    for name, t in others.items():
        if t is not None and t.device != x.device:
            raise ValueError(
                f"{name} is on {t.device}, x on {x.device}; all tensors "
                "must share one device"
            )


def lloyd_assign_many(x, centers, seg, seg_host=None):
    """Nearest centre per row and problem: ``rowmin_l2`` per segment."""
    s = kmeans_many_segments(seg, seg_host)
    _same_device(x, centers=centers, seg=seg)
    n, _, p, _ = _kmeans_many_check(x, s, centers=centers)
    labels = torch.empty(p, n, dtype=torch.int32, device=x.device)
    mind = torch.empty(p, n, dtype=torch.float32, device=x.device)
    for q in range(p):
        d, idx = rowmin_l2(x, centers[s[q] : s[q + 1]])
        labels[q] = idx.to(torch.int32)
        mind[q] = d
    return labels, mind


def lloyd_update_many(x, labels, centers, seg, active, tol=1e-4, seg_host=None):
    """One Lloyd update per active problem with ``kmeans_fit``'s own
    arithmetic (``index_add_`` sums, the same ``shift`` expression)."""
    s = kmeans_many_segments(seg, seg_host)
    _same_device(x, labels=labels, centers=centers, seg=seg, active=active)
    _, _, p, c = _kmeans_many_check(x, s, labels=labels, centers=centers, active=active)
    shift = torch.zeros(p, dtype=torch.float32, device=x.device)
    counts_all = torch.zeros(c, dtype=torch.int32, device=x.device)
    act = active.tolist()
    for q in range(p):
        if not act[q]:
            continue
        old = centers[s[q] : s[q + 1]]
        k = old.shape[0]
        lab = labels[q].long()
        rows = x
        valid = (lab >= 0) & (lab < k)
        if not bool(valid.all()):
            lab, rows = lab[valid], x[valid]
        new_centers = torch.zeros_like(old)
        counts = torch.zeros(k, dtype=x.dtype, device=x.device)
        new_centers.index_add_(0, lab, rows)
        counts.index_add_(0, lab, torch.ones(lab.shape[0], dtype=x.dtype, device=x.device))
        counts_all[s[q] : s[q + 1]] = counts.to(torch.int32)
        empty = counts == 0
        counts = counts.clamp_min(1.0)
        new_centers /= counts.unsqueeze(1)
        new_centers[empty] = old[empty]
        sh = (new_centers - old).pow(2).sum()
        centers[s[q] : s[q + 1]] = new_centers
        shift[q] = sh
        if float(sh) <= tol:
            active[q] = 0
    return shift, counts_all


def silhouette_cluster_sums(x, labels, seg, seg_host=None, chunk: int = 2048):
    """``out[i, seg[p]+c]``: sum of the L2 distances from row i to the other
    rows that labeling p puts into cluster c. Labels outside a problem's
    range belong to no cluster."""
    s = kmeans_many_segments(seg, seg_host)
    _same_device(x, labels=labels, seg=seg)
    n, _, p, c = _kmeans_many_check(x, s, labels=labels)
    onehot = torch.zeros(n, c, dtype=x.dtype, device=x.device)
    rows = torch.arange(n, device=x.device)
    for q in range(p):
        lab = labels[q].long()
        valid = (lab >= 0) & (lab < s[q + 1] - s[q])
        onehot[rows[valid], s[q] + lab[valid]] = 1.0
    out = torch.empty(n, c, dtype=x.dtype, device=x.device)
    for s0 in range(0, n, chunk):
        xc = x[s0 : s0 + chunk]
        d = pairwise_sqdist(xc, x).clamp_min_(0).sqrt_()
        m = xc.shape[0]
        d[torch.arange(m, device=x.device), torch.arange(s0, s0 + m, device=x.device)] = 0.0
        out[s0 : s0 + chunk] = d @ onehot
    return out
