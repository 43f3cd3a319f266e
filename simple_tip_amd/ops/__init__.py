"""Device-dispatching TIP ops.

Every op has two implementations:
- ``fallback``: pure torch/numpy (the CPU path and the GPU-test oracle)
- ``_tip_hip``: hand-written HIP/CDNA4 kernels (gfx950), built in-tree by
  ``setup.py`` / ``__graft_entry__.build()``.

Dispatch rule: CUDA tensors REQUIRE the HIP extension — on a GPU box a
missing/failed extension raises instead of silently falling back to eager
torch (set ``TIP_ALLOW_GPU_FALLBACK=1`` only for debugging). CPU tensors use
the fallback.
"""

import os
from typing import Dict, List, Sequence, Tuple

import torch

from . import fallback

_EXT = None
_EXT_ERR = None


def _load_compiled():
    """Import the compiled _tip_hip extension module (raises ImportError)."""
    from . import _tip_hip  # built in-tree by setup.py build_ext --inplace

    return _tip_hip


def _load_ext():
    """Load the HIP op wrapper (returns None if the .so is unavailable)."""
    global _EXT, _EXT_ERR
    if _EXT is not None or _EXT_ERR is not None:
        return _EXT
    try:
        from . import hip_ops  # thin wrapper over the compiled _tip_hip .so

        _EXT = hip_ops
    except Exception as e:  # noqa: BLE001
        _EXT_ERR = e
        _EXT = None
    return _EXT


def hip_available() -> bool:
    """True iff the HIP extension is importable."""
    return _load_ext() is not None


def _route(t: torch.Tensor):
    """Return the implementing module for a tensor's device."""
    if t.is_cuda:
        ext = _load_ext()
        if ext is None:
            if os.environ.get("TIP_ALLOW_GPU_FALLBACK") == "1":
                return fallback
            raise RuntimeError(
                "simple_tip_amd: tensor is on GPU but the HIP extension "
                "_tip_hip is not importable (build it with "
                "`python setup.py build_ext --inplace`); refusing to fall "
                f"back to eager torch. Import error: {_EXT_ERR!r}"
            )
        return ext
    return fallback


# --- bitmap ops -------------------------------------------------------------

def pack_bits(profile: torch.Tensor) -> torch.Tensor:
    return _route(profile).pack_bits(profile)


def unpack_bits(words: torch.Tensor, nbits: int) -> torch.Tensor:
    return fallback.unpack_bits(words, nbits)


def popcount_rows(words: torch.Tensor) -> torch.Tensor:
    return _route(words).popcount_rows(words)


def ctm_order(scores: torch.Tensor) -> torch.Tensor:
    return fallback.ctm_order(scores)


def cam_order(scores: torch.Tensor, words: torch.Tensor, nbits: int) -> torch.Tensor:
    return _route(words).cam_order(scores, words, nbits)


def cam_order_many(
    scores: Sequence[torch.Tensor],
    words: Sequence[torch.Tensor],
    nbits: Sequence[int],
) -> List[torch.Tensor]:
    """The CAM orders of P independent problems.

    ``scores[p]`` is [N_p], ``words[p]`` a contiguous int64 [N_p, W_p]
    packed profile with ``W_p == ceil(nbits[p] / 64)``; rows, widths and
    ``nbits`` may differ freely between the problems. ``out[p]`` equals
    ``cam_order(scores[p], words[p], nbits[p])`` element for element, for
    every input: greedy max-cover, ties to the lowest row, bits past
    ``nbits`` ignored, the loop stops when no row adds coverage, leftovers
    by descending score, stable. ``P == 0`` returns ``[]`` and a problem
    with 0 rows an empty order.

    On GPU tensors one persistent launch serves up to
    :func:`cam_many_max_problems` problems, each on its own team of blocks,
    reading the profiles where they lie; more problems are split into
    consecutive launches. All arithmetic is integer: a problem's order does
    not depend on the other problems of the call, on their order or on how
    the grid was divided. Tensors on different devices, ``words`` that is
    not contiguous int64 2-D, ``W_p != ceil(nbits_p / 64)`` or a ``scores``
    of another length raise ValueError, the call never falls back. A team
    whose bounded barrier wait runs out raises RuntimeError naming the
    problem; a partial order is never returned.
    """
    words = list(words)
    if not words:
        return fallback.cam_order_many(scores, words, nbits)
    return _route(words[0]).cam_order_many(scores, words, nbits)


def cam_many_max_problems() -> int:
    """Problems one launch of the GPU batched-CAM kernel takes; needs the
    HIP extension."""
    ext = _load_ext()
    if ext is None:
        raise RuntimeError(f"HIP extension not importable: {_EXT_ERR!r}")
    return ext.cam_many_max_problems()


# --- pairwise-distance family ----------------------------------------------

def pairwise_sqdist(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    return _route(a).pairwise_sqdist(a.contiguous(), b.contiguous())


def rowmin_l2(
    a: torch.Tensor, b: torch.Tensor, bnorm: torch.Tensor = None
) -> Tuple[torch.Tensor, torch.Tensor]:
    return _route(a).rowmin_l2(a.contiguous(), b.contiguous(), bnorm)


def kde_logsumexp(test_w: torch.Tensor, train_w: torch.Tensor) -> torch.Tensor:
    return _route(test_w).kde_logsumexp(test_w.contiguous(), train_w.contiguous())


def grouped_gaussian_scores(
    x: torch.Tensor,
    group: torch.Tensor,
    comp_off: torch.Tensor,
    means: torch.Tensor,
    mats: torch.Tensor,
    logc: torch.Tensor = None,
) -> torch.Tensor:
    """Gaussian scores [N] of rows ``x[n]`` under the components of group
    ``group[n]``, all groups in one pass.

    ``means`` [J, D] and ``mats`` [J, D, D] (symmetric precision matrices)
    stack the components of all G groups; group ``g`` owns components
    ``comp_off[g] .. comp_off[g+1]`` (``comp_off`` int32 [G+1]). With
    ``q_j = (x - mu_j)^T M_j (x - mu_j)``: ``logc=None`` is the Mahalanobis
    form of the group's single component, otherwise the mixture NLL
    ``-logsumexp_j(logc_j - q_j / 2)``. Rows whose group id is outside
    ``[0, G)`` score ``+inf``.

    On GPU tensors (fp32 or bf16 ``x``, fp32 tables) one exact-fp32 MFMA
    launch covers every group and the result is float32; a row's score does
    not depend on the batch it arrives in. Outside the envelope (more than
    256 groups, more than 8 components in a group, non-contiguous ``mats``)
    the call raises ValueError, it never falls back. CPU tensors compute in
    the dtype of ``mats``.
    """
    return _route(x).grouped_gaussian_scores(x, group, comp_off, means, mats, logc)


# --- batched k-means ---------------------------------------------------------
#
# P problems share the rows ``x`` [N, D] (float32, contiguous). Their centres
# are stacked in ``centers`` [C, D]; ``seg`` (int32 [P+1], starting at 0,
# strictly ascending) gives problem p the rows ``seg[p] .. seg[p+1]`` of it.
# ``seg_host`` is an optional host copy of ``seg`` (a sequence of ints) that
# saves the validation from reading a device ``seg`` back.
#
# GPU envelope of the three ops: P <= 64 problems, at most 16 centres per
# problem, C <= 256. Outside it, and for a non-contiguous or non-float32
# ``x``, a ``seg`` that does not ascend or tensors on different devices, the
# calls raise ValueError; they never fall back.


def lloyd_assign_many(
    x: torch.Tensor,
    centers: torch.Tensor,
    seg: torch.Tensor,
    seg_host: Sequence[int] = None,
    xnorm: torch.Tensor = None,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(labels int32 [P, N], mind float32 [P, N])``: for every problem the
    problem-local index of the nearest centre of each row and its L2
    distance, ties to the lowest index.

    ``labels[p]`` and ``mind[p]`` equal
    ``rowmin_l2(x, centers[seg[p]:seg[p+1]])`` bit for bit. On GPU tensors
    one exact-fp32 launch of the pairwise tile core computes the distances to
    all C centres and a small kernel takes the per-problem minima; ``xnorm``
    (GPU only) passes the squared row norms of ``x`` from
    :func:`row_sqnorms`, which a loop over the same ``x`` computes once.
    """
    impl = _route(x)
    if impl is fallback:
        return fallback.lloyd_assign_many(x, centers, seg, seg_host)
    return impl.lloyd_assign_many(x, centers, seg, seg_host, xnorm)


def row_sqnorms(x: torch.Tensor) -> torch.Tensor:
    """Squared row norms of a GPU ``x`` as the pairwise kernels compute them
    (the ``xnorm`` of :func:`lloyd_assign_many`); ``None`` for CPU tensors,
    whose implementation takes none."""
    impl = _route(x)
    return None if impl is fallback else impl.row_sqnorms(x)


def lloyd_update_many(
    x: torch.Tensor,
    labels: torch.Tensor,
    centers: torch.Tensor,
    seg: torch.Tensor,
    active: torch.Tensor,
    tol: float = 1e-4,
    seg_host: Sequence[int] = None,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """One Lloyd update of every problem with ``active[p] != 0`` (int32 [P]);
    returns ``(shift float32 [P], counts int32 [C])``.

    Every centre of an active problem is replaced IN PLACE by the mean of the
    rows that ``labels[p]`` gives it; a centre without rows keeps its value
    and labels outside the problem's range are ignored. ``shift[p]`` is the
    summed squared movement of the problem's centres and ``active[p]`` is
    cleared, on the device, when ``shift[p] <= tol``. Inactive problems are
    left untouched; their ``shift`` and ``counts`` are 0.

    On CPU the arithmetic is ``kmeans_fit``'s own. On GPU tensors one pass
    over ``x`` serves all problems and every sum has a fixed order (rows
    ascending within 256-row chunks, chunks ascending, no float atomics):
    two calls give bit-identical centres and a problem's result does not
    depend on the other problems of the call.
    """
    return _route(x).lloyd_update_many(x, labels, centers, seg, active, tol, seg_host)


def silhouette_cluster_sums(
    x: torch.Tensor,
    labels: torch.Tensor,
    seg: torch.Tensor,
    seg_host: Sequence[int] = None,
) -> torch.Tensor:
    """float32 [N, C]: ``out[i, seg[p] + c]`` is the sum of ``||x_i - x_j||``
    over the rows ``j != i`` with ``labels[p, j] == c`` (``labels`` int32
    [P, N]; a label outside its problem's range belongs to no cluster). The
    ``j == i`` term is exactly 0.

    On GPU tensors the N x N distance matrix is never written: an epilogue of
    the pairwise tile core adds each tile's distances into per-row cluster
    bins, for every labeling of a pass at once, and a fold adds the
    column-strip partials in ascending order. One Gram pass serves
    consecutive problems of up to 16 bins in total (k = 2..5 is one pass);
    further problems take further passes.
    """
    return _route(x).silhouette_cluster_sums(x, labels, seg, seg_host)


# --- score / profile ops ----------------------------------------------------

def softmax_uncertainties(probs: torch.Tensor) -> Dict[str, torch.Tensor]:
    return _route(probs).softmax_uncertainties(probs.contiguous())


def variation_ratio(sample_preds: torch.Tensor, num_classes: int):
    return fallback.variation_ratio(sample_preds, num_classes)


def mc_dropout_votes(
    feats: torch.Tensor,
    weight: torch.Tensor,
    bias: torch.Tensor,
    p: float,
    num_samples: int,
    seed: int,
    row_offset: int = 0,
) -> torch.Tensor:
    """Votes [N, C] (int32) of ``num_samples`` dropout-masked linear heads.

    Masks come from a stateless hash of (seed, sample, row_offset + n, d), so
    the result is reproducible and independent of batching and sharding. On
    GPU tensors the head must fit the kernel envelope (C <= 16, D <= 2048):
    outside it the call raises ValueError, it never falls back.
    """
    return _route(feats).mc_dropout_votes(
        feats, weight, bias, p, num_samples, seed, row_offset
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
    """Votes plus the sample statistics of the same dropout-masked heads.

    Returns ``(votes int32 [N, C], mean_probs float32 [N, C], mean_entropy
    float32 [N])``: ``votes`` is bit-identical to :func:`mc_dropout_votes`,
    ``mean_probs`` is the mean over the samples of softmax(logits) and
    ``mean_entropy`` the mean of the samples' softmax entropies (natural
    log). Predictive entropy, mutual information and the mean-softmax
    confidence follow from the last two
    (``core.quantifiers.mc_sample_scores``). Same masks, envelope and
    ``row_offset`` semantics as :func:`mc_dropout_votes`; on GPU tensors the
    floats are reduced in a fixed order, so a row's result does not depend
    on the batch it arrives in.
    """
    return _route(feats).mc_dropout_stats(
        feats, weight, bias, p, num_samples, seed, row_offset
    )


def mc_dropout_supported(t: torch.Tensor, C: int, D: int) -> bool:
    """Whether a [C, D] head on ``t``'s device is inside the op's envelope."""
    impl = _route(t)
    if impl is fallback:
        return True
    try:
        impl.mc_dropout_check_envelope(C, D)
    except ValueError:
        return False
    return True


#: the tensors of a transformer block's stochastic tail (see fallback)
McTransformerParams = fallback.McTransformerParams


def mc_transformer_votes(
    x: torch.Tensor,
    attn: torch.Tensor,
    params: "McTransformerParams",
    p,
    num_samples: int,
    seed: int,
    row_offset: int = 0,
) -> torch.Tensor:
    """Votes [N, C] (int32) of ``num_samples`` dropout-masked transformer
    tails.

    ``x`` [N, T, E] is the block input (the embedding output) and ``attn``
    [N, T, E] the attention output before its dropout; a sample evaluates
    ``h = LN1(x + drop1(attn))``, ``y = LN2(h + drop2(FFN(h)))``,
    ``g = mean_t y``, ``z = relu(W3 drop3(g) + b3)``, ``W4 drop4(z) + b4``
    with the four rates ``p = (p_attn, p_ffn, p_pool, p_hidden)``. The masks
    are slices of the stateless generator of :func:`mc_dropout_votes` over
    one element axis of length ``2*T*E + E + H`` (site offsets ``0``,
    ``T*E``, ``2*T*E``, ``2*T*E + E``), so the result is reproducible and
    independent of batching and sharding. On GPU tensors the tail must fit
    the kernel envelope (E == 32, T <= 128, F <= 64, H <= 64, C <= 4):
    outside it the call raises ValueError, it never falls back.
    """
    return _route(x).mc_transformer_votes(
        x, attn, params, p, num_samples, seed, row_offset
    )


def mc_transformer_stats(
    x: torch.Tensor,
    attn: torch.Tensor,
    params: "McTransformerParams",
    p,
    num_samples: int,
    seed: int,
    row_offset: int = 0,
) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``(votes int32 [N, C], mean_probs float32 [N, C], mean_entropy
    float32 [N])`` of the same masked tails as :func:`mc_transformer_votes`
    (bit-identical votes); the output contract of :func:`mc_dropout_stats`.
    """
    return _route(x).mc_transformer_stats(
        x, attn, params, p, num_samples, seed, row_offset
    )


def mc_transformer_supported(
    t: torch.Tensor, E: int, T: int, F: int, H: int, C: int
) -> bool:
    """Whether a tail of these sizes on ``t``'s device is inside the op's
    envelope."""
    impl = _route(t)
    if impl is fallback:
        return True
    try:
        impl.mc_transformer_check_envelope(E, T, F, H, C)
    except ValueError:
        return False
    return True


def nac_profile(acts: torch.Tensor, threshold: float) -> torch.Tensor:
    return _route(acts).nac_profile(acts.contiguous(), threshold)


def snac_profile(acts: torch.Tensor, max_bound: torch.Tensor) -> torch.Tensor:
    return _route(acts).snac_profile(acts.contiguous(), max_bound.contiguous())


def nbc_profile(acts: torch.Tensor, min_bound: torch.Tensor, max_bound: torch.Tensor) -> torch.Tensor:
    return _route(acts).nbc_profile(
        acts.contiguous(), min_bound.contiguous(), max_bound.contiguous()
    )


def kmnc_profile(acts: torch.Tensor, mins: torch.Tensor, maxs: torch.Tensor, sections: int) -> torch.Tensor:
    return _route(acts).kmnc_profile(
        acts.contiguous(), mins.contiguous(), maxs.contiguous(), sections
    )


def tknc_profile(layer_acts: List[torch.Tensor], k: int) -> torch.Tensor:
    return _route(layer_acts[0]).tknc_profile(
        [l.contiguous() for l in layer_acts], k
    )


def coverage_suite(
    layers: List[torch.Tensor],
    nac_thresholds: Tuple[float, ...] = (),
    upper_bounds: torch.Tensor = None,
    nbc_lower: torch.Tensor = None,
    nbc_upper: torch.Tensor = None,
    kmnc_mins: torch.Tensor = None,
    kmnc_maxs: torch.Tensor = None,
    kmnc_sections: Tuple[int, ...] = (),
    tknc_ks: Tuple[int, ...] = (),
) -> Dict[str, List[Tuple[torch.Tensor, torch.Tensor]]]:
    """Every requested NAC / SNAC / NBC / KMNC / TKNC profile of one batch.

    ``layers`` are the tapped layers as fp32 contiguous [N, K_l] tensors,
    NOT concatenated; the neuron axis of every table (``upper_bounds``
    [U, K], ``nbc_lower`` / ``nbc_upper`` [B, K], ``kmnc_mins`` /
    ``kmnc_maxs`` [K]) is their concatenation order. Returns
    ``{family: [(words int64 [N, W], scores int64 [N]), ...]}`` for the
    families ``nac``, ``snac``, ``nbc``, ``kmnc``, ``tknc``, one entry per
    threshold / table row / section count / k, with the bit layouts of the
    per-metric ops and ``scores == popcount_rows(words)``. Any family may be
    empty.

    Every word equals what :func:`nac_profile`, :func:`snac_profile`,
    :func:`nbc_profile`, :func:`kmnc_profile` and :func:`tknc_profile`
    return for the concatenated input, for every input. On GPU tensors two
    launches read the layers where they lie (once for the threshold
    families, once for top-k) and a row's words do not depend on the batch
    it arrives in. Outside the envelope (more than 8 layers, more than 4
    entries in a family, a section count outside 1..16, a k outside 1..4,
    layers of different N, a table whose width is not K) the call raises
    ValueError, it never falls back.
    """
    return _route(layers[0]).coverage_suite(
        layers, nac_thresholds, upper_bounds, nbc_lower, nbc_upper,
        kmnc_mins, kmnc_maxs, kmnc_sections, tknc_ks,
    )


def coverage_suite_chunk() -> int:
    """Neurons of the concatenated axis that one block of the GPU suite
    kernel owns (a multiple of 64); needs the HIP extension."""
    ext = _load_ext()
    if ext is None:
        raise RuntimeError(f"HIP extension not importable: {_EXT_ERR!r}")
    return ext.coverage_suite_chunk()


def bucketize_profile(values: torch.Tensor, thresholds: torch.Tensor) -> torch.Tensor:
    return _route(values).bucketize_profile(values, thresholds)
