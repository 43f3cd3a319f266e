"""Model-centric utilities: activation collection and uncertainty scoring.

Capability parity with reference src/dnn_test_prio/handler_model.py:88-206.
MI355X-native differences:
- activation taps come out of the single forward pass (models/base.py), not a
  second "transparent" keras model; tensors stay on device;
- the four point-prediction quantifiers are one fused epilogue over the
  softmax (ops.softmax_uncertainties — the K14 kernel on device);
- MC-dropout variation ratio runs DROPOUT_SAMPLE_SIZE stochastic forwards
  with device RNG and on-device vote counting ("replay", the default), or,
  for models that end in Dropout -> Linear, runs the deterministic trunk once
  and all masked heads in one kernel (``vr_mode="fused"``,
  ops.mc_dropout_votes: seeded, batch- and shard-invariant); a model with
  a ``dropout_tail()`` (the IMDB transformer: four dropouts behind a
  deterministic attention prefix) runs embedding + attention once and all
  masked tails in one kernel (ops.mc_transformer_votes), on an explicit
  ``vr_mode="fused"`` only;
- the other sampling quantifiers (predictive entropy, mutual information,
  mean softmax) are opt-in (``mc_quantifiers``) and come from the same
  samples: on the fused path one ops.mc_dropout_stats call per batch
  replaces the votes call, on replay the loop also sums the softmax outputs.
Timing taxonomy is the reference's: per metric [setup, pred, quant, cam].
"""

import logging
from typing import Dict, Generator, List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn as nn

from .. import config
from ..config import DROPOUT_SAMPLE_SIZE
from ..core.quantifiers import probs_entropy, mc_sample_scores
from ..core.timer import DeviceTimer
from .. import ops
from ..models.base import DropoutTail, TapModel

logger = logging.getLogger(__name__)


def iter_batches(x, batch_size: int):
    """Yield contiguous batches of a tensor/ndarray along dim 0."""
    n = x.shape[0]
    for s in range(0, n, batch_size):
        yield x[s : s + batch_size]


class BaseModel:
    """Wraps a :class:`TapModel` for AT extraction and uncertainty scoring."""

    def __init__(
        self,
        model: TapModel,
        activation_layers: Optional[Sequence[int]],
        include_last_layer: bool = False,
        device: Optional[torch.device] = None,
        predict_batch: int = 512,
        vr_mode: Optional[str] = None,
        vr_seed: int = 0,
        mc_quantifiers: Optional[Sequence[str]] = None,
    ):
        """``vr_mode`` selects how the variation ratio is sampled: "replay"
        (whole model per sample), "fused" (trunk once + mc_dropout_votes for
        a model that ends in Dropout -> Linear, prefix once +
        mc_transformer_votes for one with a ``dropout_tail()``; ValueError
        for any other model or outside the kernel envelope), "auto" (the
        fused head where applicable, else replay; never the tail) or None
        (``config.VR_MODE``). ``vr_seed`` seeds the fused masks.
        ``mc_quantifiers`` names the sampling scores to return, out of "VR",
        "PE" (predictive entropy), "MI" (mutual information) and "MS"
        (negated max of the mean softmax); None means
        ``config.MC_QUANTIFIERS``. "VR" is always computed."""
        if mc_quantifiers is None:
            mc_quantifiers = config.MC_QUANTIFIERS
        mc_quantifiers = tuple(mc_quantifiers)
        unknown = [q for q in mc_quantifiers if q not in config.MC_QUANTIFIER_NAMES]
        if unknown:
            raise ValueError(
                f"mc_quantifiers must be among {config.MC_QUANTIFIER_NAMES}, "
                f"got {unknown!r}"
            )
        self.mc_quantifiers = mc_quantifiers
        # the scores beyond VR, in canonical order
        self._mc_extras = tuple(
            q for q in config.MC_QUANTIFIER_NAMES
            if q != "VR" and q in mc_quantifiers
        )
        if vr_mode is None:
            vr_mode = config.VR_MODE
        if vr_mode not in config.VR_MODES:
            raise ValueError(
                f"vr_mode must be one of {config.VR_MODES}, got {vr_mode!r}"
            )
        self.vr_mode = vr_mode
        self.vr_seed = int(vr_seed)
        self.model = model
        self.activation_layers = list(activation_layers) if activation_layers else None
        self.include_last_layer = include_last_layer
        self.device = device or next(model.parameters()).device
        self.predict_batch = predict_batch
        self._graphed = None  # lazy GraphedExtractor (GPU fast path, K15)
        self.model.eval()
        if self.vr_mode == "fused":
            self._fused_vr_head()  # fail at construction, not mid-run

    def _to_device(self, x) -> torch.Tensor:
        if not isinstance(x, torch.Tensor):
            x = torch.from_numpy(np.ascontiguousarray(x))
        if x.dtype == torch.float64:
            x = x.float()
        return x.to(self.device, non_blocking=True)

    # -- activation extraction (K15) ------------------------------------

    @torch.no_grad()
    def get_activations(self, x) -> List[torch.Tensor]:
        """Single pass over (possibly large) input; returns per-layer AT
        tensors (+ softmax output last iff include_last_layer)."""
        outs: Optional[List[List[torch.Tensor]]] = None
        for batch in self.walk_activations(iter_batches(x, self.predict_batch)):
            if outs is None:
                outs = [[t] for t in batch]
            else:
                for acc, t in zip(outs, batch):
                    acc.append(t)
        assert outs is not None, "empty dataset"
        return [torch.cat(parts, dim=0) for parts in outs]

    @torch.no_grad()
    def walk_activations(self, batches) -> Generator[List[torch.Tensor], None, None]:
        """Stream batches -> per-batch list of tapped activation tensors.

        On GPU this routes through the BN-folded, hipGraph-replayed
        :class:`~simple_tip_amd.engine.extractor.GraphedExtractor` (bf16
        channels_last; fused ResNet-20 block kernels where applicable) —
        the eager MIOpen path was launch-bound.
        ``TIP_NO_GRAPH_EXTRACTOR=1`` restores the eager path for debugging.
        """
        import os

        if self.activation_layers is None:
            raise ValueError("No activation layers specified")
        if (
            self.device.type == "cuda"
            and os.environ.get("TIP_NO_GRAPH_EXTRACTOR") != "1"
        ):
            if self._graphed is None:
                from .extractor import GraphedExtractor

                self._graphed = GraphedExtractor(
                    self.model, self.activation_layers, self.device,
                    self.predict_batch,
                )
            for batch in batches:
                taps, probs = self._graphed(batch)
                out = list(taps)
                if self.include_last_layer:
                    out.append(probs)
                yield out
            return
        for batch in batches:
            xb = self._to_device(batch)
            taps, logits = self.model.forward_taps(xb, self.activation_layers)
            out = list(taps)
            if self.include_last_layer:
                out.append(torch.softmax(logits.float(), dim=1))
            yield out

    # -- uncertainty quantification (K14 + MC-dropout VR) ----------------

    @torch.no_grad()
    def get_pred_and_uncertainty(
        self, x, row_base: int = 0
    ) -> Tuple[np.ndarray, Dict[str, np.ndarray], Dict[str, List[float]]]:
        """Point predictions + all uncertainty scores + per-metric times.

        Returns (pred, {metric: scores}, {metric: [setup, pred, quant, cam]}).
        ``row_base`` is the global index of ``x[0]`` when ``x`` is a shard of
        a larger dataset; only the fused sampling path uses it (mask row
        ids). The sampling scores requested with ``mc_quantifiers`` beyond
        "VR" appear under "PE", "MI" and "MS" (higher = more uncertain).
        """
        pred_timer = DeviceTimer()
        quant_timer = DeviceTimer()
        unc_parts: Dict[str, List[torch.Tensor]] = {}
        preds_parts: List[torch.Tensor] = []
        for batch in iter_batches(x, self.predict_batch):
            with pred_timer:
                xb = self._to_device(batch)
                logits = self.model(xb)
                probs = torch.softmax(logits.float(), dim=1)
            with quant_timer:
                scores = ops.softmax_uncertainties(probs)
            preds_parts.append(probs.argmax(dim=1))
            for k, v in scores.items():
                unc_parts.setdefault(k, []).append(v)

        pred = torch.cat(preds_parts).cpu().numpy()
        uncertainties = {
            k: torch.cat(v).float().cpu().numpy() for k, v in unc_parts.items()
        }
        times = {
            k: [0.0, pred_timer.get(), quant_timer.get(), 0.0] for k in uncertainties
        }

        if self.model.has_dropout():
            if self._mc_extras:
                mc, mc_times = self._mc_scores(x, row_base=row_base)
                for k in ("VR",) + self._mc_extras:
                    uncertainties[k] = mc[k]
                    times[k] = list(mc_times)
            else:
                vr, vr_times = self._variation_ratio(x, row_base=row_base)
                uncertainties["VR"] = vr
                times["VR"] = vr_times
        else:
            logger.warning(
                "No stochastic (dropout) layers in model; skipping VR."
            )
        return pred, uncertainties, times

    def _fused_vr_head(self):
        """The Dropout -> Linear head ``(k, p, linear)`` or, in "fused" mode
        only, the :class:`DropoutTail` to fuse; None for the replay path.

        Raises ValueError in "fused" mode when the model has neither or the
        one it has is outside the kernel envelope on this device."""
        if self.vr_mode == "replay":
            return None
        head = self.model.dropout_head()
        if head is None:
            if self.vr_mode != "fused":
                return None
            tail = self.model.dropout_tail()
            if tail is None:
                raise ValueError(
                    'vr_mode="fused" needs a model whose only Dropout feeds '
                    "the final Linear layer, or one with a dropout tail "
                    "(TapModel.dropout_head() and dropout_tail() are None "
                    f"for {type(self.model).__name__})"
                )
            q = tail.params
            dims = (
                q.w1.shape[1], self.model.input_shape[0], q.w1.shape[0],
                q.w3.shape[0], q.w4.shape[0],
            )
            if not ops.mc_transformer_supported(q.w1, *dims):
                raise ValueError(
                    'vr_mode="fused": the transformer tail (E, T, F, H, C) = '
                    f"{dims} is outside the mc_transformer_votes kernel "
                    "envelope (E == 32, T <= 128, F <= 64, H <= 64, C <= 4)"
                )
            return tail
        lin = head[2]
        if not ops.mc_dropout_supported(
            lin.weight, lin.out_features, lin.in_features
        ):
            if self.vr_mode == "fused":
                raise ValueError(
                    'vr_mode="fused": the head Linear'
                    f"({lin.in_features}, {lin.out_features}) is outside the "
                    "mc_dropout_votes kernel envelope (C <= 16, D <= 2048)"
                )
            return None
        return head

    @torch.no_grad()
    def _variation_ratio(
        self, x, row_base: int = 0
    ) -> Tuple[np.ndarray, List[float]]:
        """MC-dropout variation ratio over DROPOUT_SAMPLE_SIZE samples."""
        head = self._fused_vr_head()
        if head is not None:
            return self._variation_ratio_fused(x, head, row_base)
        return self._variation_ratio_replay(x)

    @torch.no_grad()
    def _mc_scores(
        self, x, row_base: int = 0
    ) -> Tuple[Dict[str, np.ndarray], List[float]]:
        """VR plus the requested extra sampling scores, from one sampling
        pass: ({"VR": ..., "PE": ..., ...}, [0, sampling, quant, 0])."""
        head = self._fused_vr_head()
        if head is not None:
            return self._sample_fused(x, head, row_base, extras=True)
        return self._sample_replay(x, extras=True)

    def _extra_scores(self, mean_probs, mean_entropy) -> Dict[str, np.ndarray]:
        """The requested extras as float32 numpy arrays."""
        s = mc_sample_scores(mean_probs, mean_entropy)
        return {k: s[k].float().cpu().numpy() for k in self._mc_extras}

    @torch.no_grad()
    def _variation_ratio_fused(
        self, x, head, row_base: int
    ) -> Tuple[np.ndarray, List[float]]:
        """Trunk once per batch, then all masked heads in one kernel."""
        scores, times = self._sample_fused(x, head, row_base, extras=False)
        return scores["VR"], times

    def _fused_scores(self, parts, prob_parts, ent_parts, num_classes, extras):
        """VR (and the extras) from the per-batch votes / statistics."""
        if not parts:
            parts.append(torch.zeros(
                0, num_classes, dtype=torch.int32, device=self.device
            ))
            prob_parts.append(torch.zeros(0, num_classes, device=self.device))
            ent_parts.append(torch.zeros(0, device=self.device))
        counts = torch.cat(parts, dim=0)
        top = counts.max(dim=1).values.float()
        vr = 1.0 - top / float(DROPOUT_SAMPLE_SIZE)
        scores = {"VR": vr.cpu().numpy()}
        if extras:
            scores.update(self._extra_scores(
                torch.cat(prob_parts, dim=0), torch.cat(ent_parts, dim=0)
            ))
        return scores

    @torch.no_grad()
    def _sample_tail(
        self, x, tail: DropoutTail, row_base: int, extras: bool
    ) -> Tuple[Dict[str, np.ndarray], List[float]]:
        """Fused sampling of a transformer tail: embedding + attention once
        per batch in fp32 (outside autocast, so the tail's inputs do not
        depend on it), then ops.mc_transformer_votes or, with ``extras``,
        ops.mc_transformer_stats (its votes are the same votes)."""
        sampling_timer = DeviceTimer()
        quant_timer = DeviceTimer()
        self.model.eval()
        tail_op = ops.mc_transformer_stats if extras else ops.mc_transformer_votes
        params = ops.McTransformerParams(*[
            v if name == "eps" else v.detach().float().contiguous()
            for name, v in zip(tail.params._fields, tail.params)
        ])
        parts: List[torch.Tensor] = []
        prob_parts: List[torch.Tensor] = []
        ent_parts: List[torch.Tensor] = []
        with sampling_timer:
            for s0 in range(0, x.shape[0], self.predict_batch):
                tokens = self._to_device(x[s0 : s0 + self.predict_batch])
                with torch.autocast(self.device.type, enabled=False):
                    emb = tail.embed(tokens).float()
                    attn = tail.att(emb, emb, emb, need_weights=False)[0]
                out = tail_op(
                    emb.contiguous(),
                    attn.float().contiguous(),
                    params,
                    tail.rates,
                    DROPOUT_SAMPLE_SIZE,
                    self.vr_seed,
                    row_offset=int(row_base) + s0,
                )
                if extras:
                    parts.append(out[0])
                    prob_parts.append(out[1])
                    ent_parts.append(out[2])
                else:
                    parts.append(out)
        with quant_timer:
            scores = self._fused_scores(
                parts, prob_parts, ent_parts, params.w4.shape[0], extras
            )
        return (
            scores,
            [0.0, sampling_timer.get(), quant_timer.get(), 0.0],
        )

    @torch.no_grad()
    def _sample_fused(
        self, x, head, row_base: int, extras: bool
    ) -> Tuple[Dict[str, np.ndarray], List[float]]:
        """Fused sampling: ops.mc_dropout_votes per batch, or, with
        ``extras``, ops.mc_dropout_stats (its votes are the same votes). A
        :class:`DropoutTail` goes to :meth:`_sample_tail`."""
        if isinstance(head, DropoutTail):
            return self._sample_tail(x, head, row_base, extras)
        k, p, lin = head
        sampling_timer = DeviceTimer()
        quant_timer = DeviceTimer()
        self.model.eval()
        use_amp = self.device.type == "cuda"
        bias = lin.bias
        if bias is None:
            bias = torch.zeros(lin.out_features, device=lin.weight.device)
        head_op = ops.mc_dropout_stats if extras else ops.mc_dropout_votes
        parts: List[torch.Tensor] = []
        prob_parts: List[torch.Tensor] = []
        ent_parts: List[torch.Tensor] = []
        with sampling_timer:
            for s0 in range(0, x.shape[0], self.predict_batch):
                h = self._to_device(x[s0 : s0 + self.predict_batch])
                with torch.autocast("cuda", dtype=torch.bfloat16,
                                    enabled=use_amp):
                    for layer in self.model.layers[:k]:
                        h = layer(h)
                out = head_op(
                    h.float().reshape(h.shape[0], -1),
                    lin.weight.float(),
                    bias.float(),
                    p,
                    DROPOUT_SAMPLE_SIZE,
                    self.vr_seed,
                    row_offset=int(row_base) + s0,
                )
                if extras:
                    parts.append(out[0])
                    prob_parts.append(out[1])
                    ent_parts.append(out[2])
                else:
                    parts.append(out)
        with quant_timer:
            scores = self._fused_scores(
                parts, prob_parts, ent_parts, lin.out_features, extras
            )
        return (
            scores,
            [0.0, sampling_timer.get(), quant_timer.get(), 0.0],
        )

    @torch.no_grad()
    def _variation_ratio_replay(self, x) -> Tuple[np.ndarray, List[float]]:
        """MC-dropout variation ratio over DROPOUT_SAMPLE_SIZE forwards."""
        scores, times = self._sample_replay(x, extras=False)
        return scores["VR"], times

    @torch.no_grad()
    def _sample_replay(
        self, x, extras: bool
    ) -> Tuple[Dict[str, np.ndarray], List[float]]:
        """DROPOUT_SAMPLE_SIZE stochastic forwards with on-device vote
        counting; with ``extras`` the loop also sums the samples' softmax
        outputs and entropies (float32 [b, C] / [b] sums per batch)."""
        sampling_timer = DeviceTimer()
        quant_timer = DeviceTimer()
        self.model.eval()
        # enable ONLY dropout stochasticity
        for m in self.model.modules():
            if isinstance(m, nn.Dropout):
                m.train()
        try:
            n = x.shape[0]
            num_classes = self.model.num_classes
            counts = torch.zeros(
                n, num_classes, dtype=torch.float32, device=self.device
            )
            if extras:
                prob_sums = torch.zeros(
                    n, num_classes, dtype=torch.float32, device=self.device
                )
                ent_sums = torch.zeros(
                    n, dtype=torch.float32, device=self.device
                )
            with sampling_timer:
                for s0 in range(0, n, self.predict_batch):
                    xb = self._to_device(x[s0 : s0 + self.predict_batch])
                    b = xb.shape[0]
                    votes = torch.zeros(
                        b, num_classes, dtype=torch.float32, device=self.device
                    )
                    if extras:
                        psum = torch.zeros_like(votes)
                        hsum = torch.zeros(
                            b, dtype=torch.float32, device=self.device
                        )
                    # vectorize the MC samples: R independent dropout
                    # replicas per forward pass (throughput, not 200 passes)
                    # macro-batch cap 8192: measured optimum (32768 made
                    # MIOpen pick a 5x slower conv algo for these shapes)
                    reps = max(1, min(DROPOUT_SAMPLE_SIZE, 8192 // max(b, 1)))
                    done = 0
                    use_amp = self.device.type == "cuda"
                    while done < DROPOUT_SAMPLE_SIZE:
                        r = min(reps, DROPOUT_SAMPLE_SIZE - done)
                        xrep = xb.repeat(r, *([1] * (xb.dim() - 1)))
                        # bf16 autocast: the VR statistic is an argmax vote,
                        # robust to reduced-precision logits
                        with torch.autocast("cuda", dtype=torch.bfloat16,
                                            enabled=use_amp):
                            logits = self.model(xrep)
                        preds = logits.argmax(dim=1).reshape(r, b)
                        votes.scatter_add_(
                            1,
                            preds.t(),
                            torch.ones(b, r, device=self.device),
                        )
                        if extras:
                            probs = torch.softmax(
                                logits.float(), dim=1
                            ).reshape(r, b, num_classes)
                            psum += probs.sum(dim=0)
                            hsum += probs_entropy(probs).sum(dim=0)
                        done += r
                    counts[s0 : s0 + b] = votes
                    if extras:
                        prob_sums[s0 : s0 + b] = psum
                        ent_sums[s0 : s0 + b] = hsum
            with quant_timer:
                top = counts.max(dim=1).values
                vr = 1.0 - top / float(DROPOUT_SAMPLE_SIZE)
                scores = {"VR": vr.cpu().numpy()}
                if extras:
                    scores.update(self._extra_scores(
                        prob_sums / float(DROPOUT_SAMPLE_SIZE),
                        ent_sums / float(DROPOUT_SAMPLE_SIZE),
                    ))
            return (
                scores,
                [0.0, sampling_timer.get(), quant_timer.get(), 0.0],
            )
        finally:
            self.model.eval()
