"""Uncertainty-quantifier registry (uncertainty-wizard replacement).

The reference registers quantifiers by alias in uwiz's registry (reference
deepgini.py:12-40, handler_model.py:16-20). This is the native equivalent:
each quantifier maps softmax outputs [N, C] to (point predictions,
per-input quantification), declares whether higher means confidence or
uncertainty, and is resolvable by alias. The registry is what
``BaseModel.get_pred_and_uncertainty`` conceptually evaluates — on device
all point quantifiers run as one fused kernel pass (ops.softmax_uncertainties).
"""

from typing import Callable, Dict, List, Tuple

import torch

from .. import ops


class Quantifier:
    """A softmax-output quantifier."""

    aliases: List[str] = []
    is_confidence = False
    takes_samples = False

    def calculate(self, nn_outputs: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        raise NotImplementedError

    def as_uncertainty(self, nn_outputs: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """(predictions, quantification with higher = more uncertain)."""
        pred, q = self.calculate(nn_outputs)
        return pred, (-q if self.is_confidence else q)


def _pred(probs):
    return probs.argmax(dim=1)


class MaxSoftmax(Quantifier):
    aliases = ["softmax", "max_softmax", "MaxSoftmax", "SM"]
    is_confidence = True

    def calculate(self, probs):
        return _pred(probs), probs.max(dim=1).values


class PredictionConfidenceScore(Quantifier):
    aliases = ["pcs", "PCS", "prediction_confidence_score"]
    is_confidence = True

    def calculate(self, probs):
        top2 = torch.topk(probs, k=min(2, probs.shape[1]), dim=1).values
        p2 = top2[:, 1] if probs.shape[1] > 1 else torch.zeros_like(top2[:, 0])
        return _pred(probs), top2[:, 0] - p2


class SoftmaxEntropy(Quantifier):
    aliases = ["softmax_entropy", "SE", "entropy"]
    is_confidence = False

    def calculate(self, probs):
        logp = torch.where(probs > 0, torch.log(probs), torch.zeros_like(probs))
        return _pred(probs), -(probs * logp).sum(dim=1)


class DeepGini(Quantifier):
    """1 - sum(softmax^2) (reference deepgini.py:32-35)."""

    aliases = ["custom::deep_gini", "deep_gini", "DeepGini"]
    is_confidence = False

    def calculate(self, probs):
        return _pred(probs), 1.0 - (probs * probs).sum(dim=1)


class VariationRatio(Quantifier):
    """MC-dropout variation ratio over sampled class predictions [S, N]."""

    aliases = ["VR", "var_ratio", "variation_ratio"]
    is_confidence = False
    takes_samples = True

    def calculate(self, sample_preds, num_classes=None):
        nc = num_classes or int(sample_preds.max().item()) + 1
        mode, vr = ops.variation_ratio(sample_preds, nc)
        return mode, vr


def probs_entropy(probs: torch.Tensor) -> torch.Tensor:
    """-sum p log p over the last dim (natural log, 0 log 0 = 0)."""
    logp = torch.where(probs > 0, torch.log(probs), torch.zeros_like(probs))
    return -(probs * logp).sum(dim=-1)


def _first_argmax(t: torch.Tensor) -> torch.Tensor:
    """Row argmax of [N, C], lowest index on ties."""
    c = t.shape[1]
    idx = torch.arange(c, device=t.device)
    is_max = t == t.max(dim=1, keepdim=True).values
    return torch.where(is_max, idx, c).min(dim=1).values.clamp_(max=c - 1)


def mc_sample_scores(
    mean_probs: torch.Tensor, mean_entropy: torch.Tensor
) -> Dict[str, torch.Tensor]:
    """The sampling quantifications from the two sample statistics.

    ``mean_probs`` [N, C] is the mean over the samples of the softmax
    outputs, ``mean_entropy`` [N] the mean of the samples' entropies (what
    ``ops.mc_dropout_stats`` returns, or what a replay loop accumulates).
    Returns ``pred`` (argmax of the mean, lowest index on ties) and, with
    higher = more uncertain, ``PE`` = H(mean), ``MI`` = H(mean) - mean
    entropy and ``MS`` = -max(mean).
    """
    pe = probs_entropy(mean_probs)
    return {
        "pred": _first_argmax(mean_probs),
        "PE": pe,
        "MI": pe - mean_entropy,
        "MS": -mean_probs.max(dim=1).values,
    }


def _sample_stats(sample_probs: torch.Tensor):
    """[S, N, C] probabilities -> (mean over samples, mean sample entropy)."""
    return sample_probs.mean(dim=0), probs_entropy(sample_probs).mean(dim=0)


class MeanSoftmax(Quantifier):
    """Max of the mean softmax over MC samples [S, N, C] (a confidence)."""

    aliases = ["mean_softmax", "MeanSoftmax", "ensembling"]
    is_confidence = True
    takes_samples = True

    def calculate(self, sample_probs):
        s = mc_sample_scores(*_sample_stats(sample_probs))
        return s["pred"], -s["MS"]


class PredictiveEntropy(Quantifier):
    """Entropy of the mean softmax over MC samples [S, N, C]."""

    aliases = ["predictive_entropy", "pred_entropy", "PE", "PredictiveEntropy"]
    is_confidence = False
    takes_samples = True

    def calculate(self, sample_probs):
        s = mc_sample_scores(*_sample_stats(sample_probs))
        return s["pred"], s["PE"]


class MutualInformation(Quantifier):
    """BALD: entropy of the mean minus the mean entropy of the samples."""

    aliases = ["mutual_information", "mutu_info", "MI", "MutualInformation"]
    is_confidence = False
    takes_samples = True

    def calculate(self, sample_probs):
        s = mc_sample_scores(*_sample_stats(sample_probs))
        return s["pred"], s["MI"]


class QuantifierRegistry:
    """Alias -> quantifier lookup; extensible like the uwiz registry."""

    _by_alias: Dict[str, Quantifier] = {}

    @classmethod
    def register(cls, q: Quantifier):
        for a in q.aliases:
            if a in cls._by_alias:
                raise ValueError(f"alias already registered: {a}")
            cls._by_alias[a] = q

    @classmethod
    def find(cls, alias: str) -> Quantifier:
        return cls._by_alias[alias]


for _q in (MaxSoftmax(), PredictionConfidenceScore(), SoftmaxEntropy(),
           DeepGini(), VariationRatio(), MeanSoftmax(), PredictiveEntropy(),
           MutualInformation()):
    QuantifierRegistry.register(_q)
