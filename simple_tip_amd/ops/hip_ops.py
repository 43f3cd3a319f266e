"""GPU implementations of the TIP ops, backed by the _tip_hip extension.

Presents the same API as ops/fallback.py; ops/__init__.py routes CUDA
tensors here. Import fails (propagated by the dispatcher as a loud error)
when the extension .so is missing."""

from typing import Dict, List, Sequence, Tuple

import torch

from . import _load_compiled

_ext = _load_compiled()

# profile kernel modes (must match coverage.hip ProfMode)
_PROF_NAC, _PROF_SNAC, _PROF_NBC, _PROF_KMNC, _PROF_PACK = range(5)


def pack_bits(profile: torch.Tensor) -> torch.Tensor:
    return _ext.pack_bits(profile.contiguous())


def unpack_bits(words: torch.Tensor, nbits: int) -> torch.Tensor:
    from . import fallback

    return fallback.unpack_bits(words, nbits)


def popcount_rows(words: torch.Tensor) -> torch.Tensor:
    return _ext.popcount_rows(words.contiguous())


def ctm_order(scores: torch.Tensor) -> torch.Tensor:
    return torch.argsort(scores, descending=True, stable=True)


def _cam_with_leftovers(scores: torch.Tensor, picked: torch.Tensor) -> torch.Tensor:
    """``picked`` (the rows that added coverage) followed by the other rows
    by descending score, stable."""
    n = scores.shape[0]
    mask = torch.ones(n, dtype=torch.bool, device=scores.device)
    if picked.numel():
        mask[picked] = False
    left = torch.nonzero(mask, as_tuple=True)[0]
    if left.numel():
        order_left = left[
            torch.argsort(scores[left].float(), descending=True, stable=True)
        ]
        return torch.cat([picked, order_left])
    return picked


def cam_order(scores: torch.Tensor, words: torch.Tensor, nbits: int) -> torch.Tensor:
    picked = _ext.cam_greedy(words.contiguous(), nbits).to(scores.device)
    return _cam_with_leftovers(scores, picked)


def cam_many_max_problems() -> int:
    """Problems one launch of the batched CAM kernel takes."""
    return _ext.cam_many_max_problems()


#: constants of cam_many.hip: full sweeps give a row to a wave from
#: CAM_MANY_WIDE_WORDS words on; a pick whose ``newly`` mask has L non-zero
#: words updates the gains incrementally when L * CAM_MANY_INCR_DIV <= W and
#: L <= CAM_MANY_LIST_CAP; a team has at most CAM_MANY_TEAM_CAP blocks
CAM_MANY_WIDE_WORDS = _ext.cam_many_wide_words()
CAM_MANY_INCR_DIV = _ext.cam_many_incr_div()
CAM_MANY_LIST_CAP = _ext.cam_many_list_cap()
CAM_MANY_TEAM_CAP = _ext.cam_many_team_cap()


def cam_many_force_full(on: bool) -> None:
    """Measurement switch: with ``on`` the batched kernel recounts every row
    after every pick instead of updating the gains from the pick's list.
    Orders do not change."""
    _ext.cam_many_force_full(bool(on))


def cam_many_plan(rows: Sequence[int], widths: Sequence[int], grid: int) -> List[int]:
    """Blocks per problem of one launch on a grid of ``grid`` blocks."""
    return _ext.cam_many_plan([int(r) for r in rows], [int(w) for w in widths], int(grid))


def cam_order_many(scores, words, nbits) -> List[torch.Tensor]:
    scores, words = list(scores), list(words)
    nbits = [int(b) for b in nbits]
    if not len(scores) == len(words) == len(nbits):
        raise ValueError("scores, words and nbits must have one entry per problem")
    if not words:
        return []
    dev = words[0].device
    for p, (s, w, b) in enumerate(zip(scores, words, nbits)):
        if s.device != dev or w.device != dev:
            raise ValueError(
                f"cam_order_many: problem {p} is on {s.device} / {w.device}, "
                f"problem 0 on {dev}; all tensors must share one device"
            )
        if w.dtype != torch.int64 or w.dim() != 2 or not w.is_contiguous():
            raise ValueError(
                f"cam_order_many: words[{p}] must be a contiguous int64 "
                f"[N, W] tensor (got {w.dtype}, shape {tuple(w.shape)})"
            )
        if b < 0 or w.shape[1] != (b + 63) // 64:
            raise ValueError(
                f"cam_order_many: words[{p}] has {w.shape[1]} words per row, "
                f"nbits={b} needs {(b + 63) // 64}"
            )
        if s.dim() != 1 or s.shape[0] != w.shape[0]:
            raise ValueError(
                f"cam_order_many: scores[{p}] has shape {tuple(s.shape)}, "
                f"words[{p}] has {w.shape[0]} rows"
            )
        if w.shape[0] >= 1 << 23 or w.shape[1] >= 1 << 24:
            raise ValueError(
                f"cam_order_many on GPU takes fewer than 2^23 rows of fewer "
                f"than 2^24 words (problem {p}: {tuple(w.shape)})"
            )
    # a problem without rows or without bits picks nothing: no team for it
    live = [p for p, w in enumerate(words) if w.shape[0] and w.shape[1]]
    picked = {}
    step = cam_many_max_problems()
    for lo in range(0, len(live), step):
        chunk = live[lo : lo + step]
        outs = _ext.cam_greedy_many(
            [words[p] for p in chunk], [nbits[p] for p in chunk]
        )
        picked.update(zip(chunk, outs))
    empty = torch.empty(0, dtype=torch.int64, device=dev)
    return [
        _cam_with_leftovers(scores[p], picked.get(p, empty))
        for p in range(len(words))
    ]


def pairwise_sqdist(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    return _ext.pairwise_sqdist(a.float(), b.float())


def rowmin_l2(
    a: torch.Tensor, b: torch.Tensor, bnorm: torch.Tensor = None
) -> Tuple[torch.Tensor, torch.Tensor]:
    d, i = _ext.rowmin_l2(a.float(), b.float(), bnorm)
    return d, i


def kde_logsumexp(test_w: torch.Tensor, train_w: torch.Tensor) -> torch.Tensor:
    return _ext.kde_logsumexp(test_w.float(), train_w.float())


def softmax_uncertainties(probs: torch.Tensor) -> Dict[str, torch.Tensor]:
    neg_max, neg_pcs, entropy, gini = _ext.softmax_scores(probs.float())
    return {
        "softmax": neg_max,
        "pcs": neg_pcs,
        "softmax_entropy": entropy,
        "deep_gini": gini,
    }


def variation_ratio(sample_preds: torch.Tensor, num_classes: int):
    from . import fallback

    return fallback.variation_ratio(sample_preds, num_classes)


#: device envelope of the fused MC-dropout head (mcdropout.hip): the
#: transposed weights [D][C padded to 4] plus the bias row must fit in LDS
MC_DROPOUT_MAX_CLASSES = _ext.mc_dropout_max_classes()
MC_DROPOUT_MAX_FEATURES = _ext.mc_dropout_max_features()


def mc_dropout_launch_config(D: int, C: int) -> Dict[str, int]:
    """Launch constants of ``mc_dropout_votes`` on the current device.

    One wave handles one row; a block holds ``rows_per_block`` waves and the
    grid is capped at ``max_grid`` blocks, so ``rows_per_pass`` rows are in
    flight and the grid-stride row loop runs ``ceil(N / rows_per_pass)``
    passes.
    """
    rows_per_block = _ext.mc_dropout_rows_per_block()
    max_grid = _ext.mc_dropout_max_grid(int(D), int(C))
    return {
        "rows_per_block": rows_per_block,
        "max_grid": max_grid,
        "rows_per_pass": rows_per_block * max_grid,
    }


def mc_dropout_check_envelope(C: int, D: int) -> None:
    """Raise ValueError if a [C, D] head is outside the kernel's envelope."""
    if not (1 <= C <= MC_DROPOUT_MAX_CLASSES and 1 <= D <= MC_DROPOUT_MAX_FEATURES):
        raise ValueError(
            f"mc_dropout_votes on GPU supports C <= {MC_DROPOUT_MAX_CLASSES} "
            f"classes and D <= {MC_DROPOUT_MAX_FEATURES} features "
            f"(got C={C}, D={D})"
        )


def _mc_dropout_args(feats, weight, bias, p, num_samples, seed, row_offset):
    """Validate and convert the arguments shared by the two mcdropout ops."""
    from . import fallback

    if feats.dim() != 2 or weight.dim() != 2 or bias.dim() != 1:
        raise ValueError("expected feats [N, D], weight [C, D], bias [C]")
    n, d = feats.shape
    c = weight.shape[0]
    if weight.shape[1] != d or bias.shape[0] != c:
        raise ValueError("weight must be [C, D] and bias [C]")
    mc_dropout_check_envelope(c, d)
    S = int(num_samples)
    if not 1 <= S <= 65535:
        raise ValueError(f"num_samples must be in [1, 65535], got {S}")
    row_offset = int(row_offset)
    if row_offset < 0 or row_offset + n > 2 ** 32:
        raise ValueError("rows must satisfy row_offset + N <= 2^32")
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    dev = feats.device
    return (
        feats.float().contiguous(),
        weight.to(dev).float().contiguous(),
        bias.to(dev).float().contiguous(),
        fallback.dropout_threshold(p),
        fallback.dropout_scale(p),
        S,
        seed & 0xFFFFFFFF,
        seed >> 32,
        row_offset,
    )


def mc_dropout_votes(
    feats: torch.Tensor,
    weight: torch.Tensor,
    bias: torch.Tensor,
    p: float,
    num_samples: int,
    seed: int,
    row_offset: int = 0,
) -> torch.Tensor:
    return _ext.mc_dropout_votes(
        *_mc_dropout_args(feats, weight, bias, p, num_samples, seed, row_offset)
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
    votes, mean_probs, mean_entropy = _ext.mc_dropout_stats(
        *_mc_dropout_args(feats, weight, bias, p, num_samples, seed, row_offset)
    )
    return votes, mean_probs, mean_entropy


#: device envelope of the fused transformer tail (mctail.hip): the embedding
#: width is fixed, the row's x / attn and the parameters must fit in LDS
(
    MC_TRANSFORMER_EMBED,
    MC_TRANSFORMER_MAX_TOKENS,
    MC_TRANSFORMER_MAX_FF,
    MC_TRANSFORMER_MAX_HIDDEN,
    MC_TRANSFORMER_MAX_CLASSES,
) = _ext.mc_transformer_envelope()


def mc_transformer_launch_config(T: int, F: int, H: int) -> Dict[str, int]:
    """Launch constants of ``mc_transformer_votes`` on the current device.

    One block handles one row at a time; the grid is capped at ``max_grid``
    blocks, so ``rows_per_pass`` rows are in flight and the grid-stride row
    loop runs ``ceil(N / rows_per_pass)`` passes.
    """
    max_grid = _ext.mc_transformer_max_grid(int(T), int(F), int(H))
    return {
        "rows_per_block": 1,
        "max_grid": max_grid,
        "rows_per_pass": max_grid,
        "lds_bytes": _ext.mc_transformer_lds_bytes(int(T), int(F), int(H)),
    }


def mc_transformer_check_envelope(E: int, T: int, F: int, H: int, C: int) -> None:
    """Raise ValueError if a tail of these sizes is outside the envelope."""
    if not (
        E == MC_TRANSFORMER_EMBED
        and 1 <= T <= MC_TRANSFORMER_MAX_TOKENS
        and 1 <= F <= MC_TRANSFORMER_MAX_FF
        and 1 <= H <= MC_TRANSFORMER_MAX_HIDDEN
        and 1 <= C <= MC_TRANSFORMER_MAX_CLASSES
    ):
        raise ValueError(
            f"mc_transformer_votes on GPU supports E == {MC_TRANSFORMER_EMBED}, "
            f"T <= {MC_TRANSFORMER_MAX_TOKENS}, F <= {MC_TRANSFORMER_MAX_FF}, "
            f"H <= {MC_TRANSFORMER_MAX_HIDDEN}, C <= {MC_TRANSFORMER_MAX_CLASSES} "
            f"(got E={E}, T={T}, F={F}, H={H}, C={C})"
        )


def _mc_transformer(x, attn, params, p, num_samples, seed, row_offset, stats):
    """Validate and convert the arguments, then launch."""
    from . import fallback

    n, t, e, f, h, c = fallback.mc_transformer_dims(x, attn, params)
    mc_transformer_check_envelope(e, t, f, h, c)
    S = int(num_samples)
    if not 1 <= S <= 65535:
        raise ValueError(f"num_samples must be in [1, 65535], got {S}")
    row_offset = int(row_offset)
    if row_offset < 0 or row_offset + n > 2 ** 32:
        raise ValueError("rows must satisfy row_offset + N <= 2^32")
    rates = fallback._mc_transformer_rates(p)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    dev = x.device
    tensors = [
        v.to(dev).float().contiguous()
        for name, v in zip(params._fields, params)
        if name != "eps"
    ]
    return _ext.mc_transformer(
        x.float().contiguous(),
        attn.to(dev).float().contiguous(),
        tensors,
        float(params.eps),
        [fallback.dropout_threshold(v) for v in rates],
        [fallback.dropout_scale(v) for v in rates],
        S,
        seed & 0xFFFFFFFF,
        seed >> 32,
        row_offset,
        stats,
    )


def mc_transformer_votes(
    x, attn, params, p, num_samples: int, seed: int, row_offset: int = 0
) -> torch.Tensor:
    return _mc_transformer(
        x, attn, params, p, num_samples, seed, row_offset, False
    )[0]


def mc_transformer_stats(
    x, attn, params, p, num_samples: int, seed: int, row_offset: int = 0
) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    votes, mean_probs, mean_entropy = _mc_transformer(
        x, attn, params, p, num_samples, seed, row_offset, True
    )
    return votes, mean_probs, mean_entropy


#: Cap on the centred workspace of one grouped-Gaussian launch, in bytes
#: (``slots * padded_rows * D * 4``). A batch whose workspace would be larger
#: is scored in row chunks; per-row results do not depend on the batch a row
#: arrives in, so chunking is invisible in the output. 256 MiB holds both
#: measured shapes in one chunk (serving batch 20480 x 64; study batch
#: 10000 x 1600 with three components, which fits up to 12672 rows) and
#: stays far below the HBM a fitted study already occupies. A chunk is never
#: smaller than one 128-row block, so a tiny cap (tests set one) only means
#: many chunks.
GAUSS_WORKSPACE_BYTES = 256 << 20


class GaussianTables:
    """Validated, device-resident tables of a grouped Gaussian scorer.

    Built once per fit (the validation reads ``comp_off`` on the host); every
    call through :func:`grouped_gaussian_scores_tables` is then free of host
    copies. ``means`` [J, D], ``mats`` [J, D, D] and ``logc`` [J] are fp32,
    ``comp_off`` int32 [G+1].
    """

    def __init__(self, comp_off, means, mats, logc, device):
        from . import fallback

        if mats.dtype != torch.float32:
            raise ValueError("mats must be float32 on the GPU path")
        self.G, self.J, self.D, self.slots = fallback.gaussian_check_envelope(
            comp_off, means, mats, logc
        )
        self.device = torch.device(device)
        f32 = dict(device=self.device, dtype=torch.float32)
        self.comp_off = torch.as_tensor(comp_off).to(self.device, torch.int32).contiguous()
        self.means = means.to(**f32).contiguous()
        self.mats = mats.to(**f32).contiguous()
        self.logc = None if logc is None else logc.to(**f32).contiguous()
        self.jb = (self.D + 127) // 128
        self._ws = {}

    def chunk_rows(self) -> int:
        """Largest 128-multiple batch whose workspace fits the cap."""
        per_row = max(self.slots, 1) * self.D * 4
        rows = GAUSS_WORKSPACE_BYTES // per_row - 128 * self.G
        return max(128, rows // 128 * 128)

    def workspace(self, b: int, own_plan: bool):
        """Per-batch-size scratch, reused from call to call on one stream."""
        ws = self._ws.get(b)
        if ws is None:
            if len(self._ws) >= 4:
                self._ws.clear()
            bp = _ext.segment_plan_rows(b, self.G)
            slots = max(self.slots, 1)
            f32 = dict(device=self.device, dtype=torch.float32)
            ws = {
                "dc": torch.empty(slots * bp * self.D, **f32),
                "pquad": torch.empty(slots * self.jb * bp, **f32),
            }
            self._ws[b] = ws
        if own_plan and "tseg" not in ws:
            bp = _ext.segment_plan_rows(b, self.G)
            i32 = dict(device=self.device, dtype=torch.int32)
            ws["tseg"] = torch.empty(self.G + 1, **i32)
            ws["rowmap"] = torch.empty(bp, **i32)
            ws["dest"] = torch.empty(b, **i32)
        return ws


def grouped_gaussian_into(x, tables: GaussianTables, tseg, rowmap, out) -> None:
    """Score ``x`` [B, D] (fp32 or bf16) through an existing segment plan over
    ``tables.G`` groups into ``out`` [B] (fp32, pre-filled with +inf)."""
    ws = tables.workspace(x.shape[0], own_plan=False)
    _ext.grouped_gauss_plan(
        x, tseg, rowmap, tables.comp_off, tables.means, tables.mats,
        tables.logc, max(tables.slots, 1), ws["dc"], ws["pquad"], out,
    )


def grouped_gaussian_scores_tables(
    x: torch.Tensor, group: torch.Tensor, tables: GaussianTables, out=None
) -> torch.Tensor:
    """float32 [N] scores; no host copy, one plan + three kernels per chunk.
    ``out`` (optional) is a float32 [N] tensor already filled with +inf."""
    if x.dim() != 2 or x.shape[1] != tables.D:
        raise ValueError(f"x must be [N, {tables.D}]")
    if x.dtype != torch.bfloat16:
        x = x.float()
    x = x.contiguous()
    group = group.to(x.device, torch.int64).contiguous()
    n = x.shape[0]
    if out is None:
        out = torch.full((n,), float("inf"), dtype=torch.float32, device=x.device)
    if n == 0 or tables.slots == 0:
        return out
    step = tables.chunk_rows()
    for lo in range(0, n, step):
        hi = min(n, lo + step)
        ws = tables.workspace(hi - lo, own_plan=True)
        _ext.segment_plan_out(
            group[lo:hi], tables.G, ws["tseg"], ws["rowmap"], ws["dest"]
        )
        grouped_gaussian_into(
            x[lo:hi], tables, ws["tseg"], ws["rowmap"], out[lo:hi]
        )
    return out


def grouped_gaussian_scores(
    x: torch.Tensor,
    group: torch.Tensor,
    comp_off: torch.Tensor,
    means: torch.Tensor,
    mats: torch.Tensor,
    logc: torch.Tensor = None,
) -> torch.Tensor:
    tables = GaussianTables(comp_off, means, mats, logc, x.device)
    return grouped_gaussian_scores_tables(x, group, tables)


def _empty(t):
    return torch.empty(0, dtype=torch.float32, device=t.device)


def nac_profile(acts: torch.Tensor, threshold: float) -> torch.Tensor:
    words, _ = _ext.profile(
        _PROF_NAC, acts.float(), _empty(acts), _empty(acts), float(threshold),
        1, acts.shape[1],
    )
    return words


def snac_profile(acts: torch.Tensor, max_bound: torch.Tensor) -> torch.Tensor:
    words, _ = _ext.profile(
        _PROF_SNAC, acts.float(), _empty(acts), max_bound.float(), 0.0, 1,
        acts.shape[1],
    )
    return words


def nbc_profile(acts, min_bound, max_bound) -> torch.Tensor:
    words, _ = _ext.profile(
        _PROF_NBC, acts.float(), min_bound.float(), max_bound.float(), 0.0, 2,
        acts.shape[1] * 2,
    )
    return words


def kmnc_profile(acts, mins, maxs, sections: int) -> torch.Tensor:
    words, _ = _ext.profile(
        _PROF_KMNC, acts.float(), mins.float(), maxs.float(), 0.0, sections,
        acts.shape[1] * sections,
    )
    return words


def tknc_profile(layer_acts: List[torch.Tensor], k: int) -> torch.Tensor:
    nbits = sum(l.shape[1] for l in layer_acts)
    n = layer_acts[0].shape[0]
    w = (nbits + 63) // 64
    words = torch.zeros(n, w, dtype=torch.int64, device=layer_acts[0].device)
    offset = 0
    for layer in layer_acts:
        _ext.tknc_layer(layer.float(), k, offset, words)
        offset += layer.shape[1]
    return words


#: device envelope of the fused coverage suite (coverage_suite.hip)
COVERAGE_SUITE_MAX_LAYERS = 8
COVERAGE_SUITE_MAX_FAMILY = 4
COVERAGE_SUITE_MAX_SECTIONS = 16
COVERAGE_SUITE_MAX_TOPK = 4


def coverage_suite_chunk() -> int:
    """Neurons of the concatenated axis one block of the suite kernel owns."""
    return _ext.coverage_suite_chunk()


def _suite_table(t, ndim, k, name, dev):
    """``t`` as an fp32 table on ``dev`` whose last axis is the K neurons;
    None (or no rows) becomes an empty tensor."""
    if t is None or t.shape[0] == 0:
        return torch.empty(0, dtype=torch.float32, device=dev)
    if t.dim() != ndim or t.shape[-1] != k:
        raise ValueError(
            f"{name} must have width K={k} (got shape {tuple(t.shape)})"
        )
    return t.to(dev).float().contiguous()


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
    from . import fallback

    cap = COVERAGE_SUITE_MAX_FAMILY
    layers = list(layers)
    if not 1 <= len(layers) <= COVERAGE_SUITE_MAX_LAYERS:
        raise ValueError(
            f"coverage_suite on GPU takes 1..{COVERAGE_SUITE_MAX_LAYERS} "
            f"layers (got {len(layers)})"
        )
    if any(l.dim() != 2 for l in layers):
        raise ValueError("layers must be [N, K_l]")
    n = layers[0].shape[0]
    if any(l.shape[0] != n for l in layers):
        raise ValueError("all layers must share N")
    dev = layers[0].device
    k = sum(l.shape[1] for l in layers)
    nac_thresholds = tuple(float(t) for t in nac_thresholds)
    kmnc_sections = tuple(int(v) for v in kmnc_sections)
    tknc_ks = tuple(int(v) for v in tknc_ks)
    if any(not 1 <= v <= COVERAGE_SUITE_MAX_SECTIONS for v in kmnc_sections):
        raise ValueError(
            f"kmnc_sections must lie in 1..{COVERAGE_SUITE_MAX_SECTIONS}"
        )
    if any(not 1 <= v <= COVERAGE_SUITE_MAX_TOPK for v in tknc_ks):
        raise ValueError(f"tknc_ks must lie in 1..{COVERAGE_SUITE_MAX_TOPK}")
    if (nbc_lower is None) != (nbc_upper is None) or (
        nbc_lower is not None and nbc_lower.shape != nbc_upper.shape
    ):
        raise ValueError("nbc_lower and nbc_upper must have the same shape")
    if kmnc_sections and (kmnc_mins is None or kmnc_maxs is None):
        raise ValueError("kmnc_sections needs kmnc_mins and kmnc_maxs")
    upper = _suite_table(upper_bounds, 2, k, "upper_bounds", dev)
    lower_b = _suite_table(nbc_lower, 2, k, "nbc_lower", dev)
    upper_b = _suite_table(nbc_upper, 2, k, "nbc_upper", dev)
    mins = _suite_table(kmnc_mins if kmnc_sections else None, 1, k, "kmnc_mins", dev)
    maxs = _suite_table(kmnc_maxs if kmnc_sections else None, 1, k, "kmnc_maxs", dev)
    counts = {
        "nac": len(nac_thresholds),
        "snac": upper.shape[0] if upper.dim() == 2 else 0,
        "nbc": lower_b.shape[0] if lower_b.dim() == 2 else 0,
        "kmnc": len(kmnc_sections),
        "tknc": len(tknc_ks),
    }
    for fam, c in counts.items():
        if c > cap:
            raise ValueError(
                f"coverage_suite on GPU takes at most {cap} {fam} profiles "
                f"per call (got {c})"
            )
    flat = _ext.coverage_suite(
        [l.float().contiguous() for l in layers],
        list(nac_thresholds), upper, lower_b, upper_b, mins, maxs,
        list(kmnc_sections), list(tknc_ks),
    )
    scores = flat[-1]
    out, at = {}, 0
    for fam in fallback.COVERAGE_SUITE_FAMILIES:
        out[fam] = [(flat[at + i], scores[at + i]) for i in range(counts[fam])]
        at += counts[fam]
    return out


def bucketize_profile(values: torch.Tensor, thresholds: torch.Tensor) -> torch.Tensor:
    return _ext.bucketize(
        values.double().contiguous(),
        thresholds.to(values.device).double().contiguous(),
        thresholds.shape[0] - 1,
    )


#: device envelope of the batched k-means ops (kmeans_many.hip): problems per
#: call, centres per problem, stacked centres per call; the rows one block of
#: the update folds before it writes a partial; the bins one Gram pass of
#: silhouette_cluster_sums serves
(
    KMEANS_MANY_MAX_PROBLEMS,
    KMEANS_MANY_MAX_K,
    KMEANS_MANY_MAX_CENTERS,
    KMEANS_MANY_CHUNK_ROWS,
    SILHOUETTE_PASS_BINS,
) = _ext.kmeans_many_envelope()


def _kmeans_many_args(x, seg, seg_host, **tensors):
    """Validate the arguments shared by the three batched k-means ops and
    return the host segment list."""
    from . import fallback

    s = fallback.kmeans_many_segments(seg, seg_host)
    fallback._same_device(x, seg=seg, **tensors)
    fallback._kmeans_many_check(x, s, **tensors)
    p, c = len(s) - 1, s[-1]
    if p > KMEANS_MANY_MAX_PROBLEMS or c > KMEANS_MANY_MAX_CENTERS:
        raise ValueError(
            f"batched k-means on GPU takes P <= {KMEANS_MANY_MAX_PROBLEMS} "
            f"problems and C <= {KMEANS_MANY_MAX_CENTERS} stacked centres "
            f"(got P={p}, C={c})"
        )
    widest = max(b - a for a, b in zip(s, s[1:]))
    if widest > KMEANS_MANY_MAX_K:
        raise ValueError(
            f"batched k-means on GPU takes at most {KMEANS_MANY_MAX_K} "
            f"centres per problem (got {widest})"
        )
    if x.shape[0] >= 1 << 24:
        raise ValueError("batched k-means on GPU takes fewer than 2^24 rows")
    if not seg.is_contiguous():
        raise ValueError("seg must be contiguous")
    return s


def row_sqnorms(x: torch.Tensor) -> torch.Tensor:
    """Squared row norms as the pairwise kernels compute them."""
    return _ext.rownorm(x)


def lloyd_assign_many(x, centers, seg, seg_host=None, xnorm=None):
    """One EPI_FULL launch against the stacked centres, then the per-problem
    arg-min; ``xnorm`` reuses the row norms of ``x`` (:func:`row_sqnorms`)."""
    _kmeans_many_args(x, seg, seg_host, centers=centers)
    labels, mind = _ext.lloyd_assign_many(x, centers, seg, xnorm)
    return labels, mind


def lloyd_update_many(x, labels, centers, seg, active, tol=1e-4, seg_host=None):
    """Fixed-order centre update of the active problems, in place."""
    _kmeans_many_args(
        x, seg, seg_host, labels=labels, centers=centers, active=active
    )
    shift, counts = _ext.lloyd_update_many(
        x, labels, centers, seg, active, float(tol)
    )
    return shift, counts


def silhouette_passes(seg_list: Sequence[int]) -> List[int]:
    """First problem of every Gram pass of ``silhouette_cluster_sums``, and P
    at the end: consecutive problems share a pass while their bins number at
    most ``SILHOUETTE_PASS_BINS``."""
    groups, bins = [0], 0
    for p, (a, b) in enumerate(zip(seg_list, seg_list[1:])):
        if bins + (b - a) > SILHOUETTE_PASS_BINS:
            groups.append(p)
            bins = 0
        bins += b - a
    groups.append(len(seg_list) - 1)
    return groups


def silhouette_cluster_sums(x, labels, seg, seg_host=None):
    """[N, C] cluster sums, one Gram pass per group of
    :func:`silhouette_passes`."""
    s = _kmeans_many_args(x, seg, seg_host, labels=labels)
    return _ext.silhouette_cluster_sums(x, labels, seg, s, silhouette_passes(s))
