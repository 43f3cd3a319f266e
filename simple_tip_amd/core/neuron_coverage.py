"""Neuron-coverage metrics: NAC, KMNC, NBC, SNAC, TKNC.

Capability parity with reference src/core/neuron_coverage.py:31-167, with two
MI355X-native changes:
- profiles are packed bitmaps (:class:`BitProfile`) produced by fused HIP
  kernels on device (bool numpy arrays in the reference);
- the score is the profile popcount, computed in the same pass
  (reference ``sum_score``, neuron_coverage.py:8-22).

Every metric takes a list of per-layer activation tensors [N, ...] and
returns ``(scores, BitProfile)``. :class:`CoverageSuite` evaluates a whole
dictionary of fitted metrics in one fused call per batch.
"""

import abc
from typing import Dict, List, Tuple

import torch

from .. import ops
from .bitmap import BitProfile


def flatten_layers(layers: List[torch.Tensor]) -> torch.Tensor:
    """Flatten each layer to [N, K_l] and concatenate along features."""
    flat = [l.reshape(l.shape[0], -1) for l in layers]
    return torch.cat(flat, dim=1)


def sum_score(profile: BitProfile) -> torch.Tensor:
    """Number of covered profile sections per sample."""
    return profile.popcount()


class CoverageMethod(abc.ABC):
    """Base class for coverage criteria (fit in __init__, profile in call)."""

    @abc.abstractmethod
    def __call__(
        self, activations: List[torch.Tensor]
    ) -> Tuple[torch.Tensor, BitProfile]:
        """Per-sample (scores, packed profiles) for a batch of activations."""


class NAC(CoverageMethod):
    """Neuron-Activation Coverage: activation > threshold."""

    def __init__(self, cov_threshold: float):
        self.cov_threshold = float(cov_threshold)

    def __call__(self, activations):
        acts = flatten_layers(activations)
        words = ops.nac_profile(acts, self.cov_threshold)
        prof = BitProfile(words, acts.shape[1])
        return sum_score(prof), prof


class KMNC(CoverageMethod):
    """K-Multisection Neuron Coverage over train min/max ranges."""

    def __init__(self, mins: List[torch.Tensor], maxs: List[torch.Tensor], sections: int):
        self.sections = int(sections)
        self.mins = flatten_layers([m.unsqueeze(0) for m in mins]).squeeze(0)
        self.maxs = flatten_layers([m.unsqueeze(0) for m in maxs]).squeeze(0)

    def __call__(self, activations):
        acts = flatten_layers(activations)
        words = ops.kmnc_profile(
            acts, self.mins.to(acts.device), self.maxs.to(acts.device), self.sections
        )
        prof = BitProfile(words, acts.shape[1] * self.sections)
        return sum_score(prof), prof


class NBC(CoverageMethod):
    """Neuron Boundary Coverage: a <= min - s*std or a >= max + s*std."""

    def __init__(self, mins, maxs, stds, scaler: float):
        min_arr = flatten_layers([m.unsqueeze(0) for m in mins]).squeeze(0)
        max_arr = flatten_layers([m.unsqueeze(0) for m in maxs]).squeeze(0)
        std_arr = flatten_layers([m.unsqueeze(0) for m in stds]).squeeze(0)
        self.min_boundaries = min_arr - scaler * std_arr
        self.max_boundaries = max_arr + scaler * std_arr

    def __call__(self, activations):
        acts = flatten_layers(activations)
        words = ops.nbc_profile(
            acts,
            self.min_boundaries.to(acts.device),
            self.max_boundaries.to(acts.device),
        )
        prof = BitProfile(words, acts.shape[1] * 2)
        return sum_score(prof), prof


class SNAC(CoverageMethod):
    """Strong Neuron Activation Coverage: a >= max + s*std."""

    def __init__(self, maxs, stds, scaler: float):
        max_arr = flatten_layers([m.unsqueeze(0) for m in maxs]).squeeze(0)
        std_arr = flatten_layers([m.unsqueeze(0) for m in stds]).squeeze(0)
        self.max_boundaries = max_arr + scaler * std_arr

    def __call__(self, activations):
        acts = flatten_layers(activations)
        words = ops.snac_profile(acts, self.max_boundaries.to(acts.device))
        prof = BitProfile(words, acts.shape[1])
        return sum_score(prof), prof


class TKNC(CoverageMethod):
    """Top-k Neuron Coverage: per layer, the k most-active neurons."""

    def __init__(self, top_neurons: int):
        self.top_neurons = int(top_neurons)

    def __call__(self, activations):
        layers = [l.reshape(l.shape[0], -1) for l in activations]
        words = ops.tknc_profile(layers, self.top_neurons)
        nbits = sum(l.shape[1] for l in layers)
        prof = BitProfile(words, nbits)
        return sum_score(prof), prof


class CoverageSuite:
    """All metrics of a dictionary from one fused ``ops.coverage_suite`` call.

    ``metrics`` maps ids to fitted NAC / SNAC / NBC / KMNC / TKNC objects
    (any other type raises TypeError). Their tables are stacked once per
    device; ``suite(activations)`` then returns ``{metric_id: (scores,
    BitProfile)}`` in the metrics' order, each entry equal to
    ``metrics[metric_id](activations)`` bit for bit. The layers are read
    where they lie: nothing is concatenated.

    The op takes at most four profiles per family and one KMNC range table
    per call; a larger dictionary is split over several calls, it is not
    refused.
    """

    FAMILY_CAP = 4
    _FAMILY = {NAC: "nac", SNAC: "snac", NBC: "nbc", KMNC: "kmnc", TKNC: "tknc"}

    def __init__(self, metrics: Dict[str, CoverageMethod]):
        self.metrics = dict(metrics)
        for metric_id, metric in self.metrics.items():
            if type(metric) not in self._FAMILY:
                raise TypeError(
                    f"CoverageSuite cannot evaluate {metric_id!r}: "
                    f"{type(metric).__name__} is not one of NAC, SNAC, NBC, "
                    f"KMNC, TKNC"
                )
        self._calls = self._plan()
        self._tables: Dict[torch.device, List[dict]] = {}

    def _plan(self) -> List[Dict[str, List[str]]]:
        """Metric ids per family for each suite call, first fit."""
        calls: List[Dict[str, List[str]]] = []
        for metric_id, metric in self.metrics.items():
            fam = self._FAMILY[type(metric)]
            for call in calls:
                if len(call[fam]) < self.FAMILY_CAP and (
                    fam != "kmnc"
                    or not call[fam]
                    or self._same_ranges(self.metrics[call[fam][0]], metric)
                ):
                    call[fam].append(metric_id)
                    break
            else:
                calls.append({f: [] for f in self._FAMILY.values()})
                calls[-1][fam].append(metric_id)
        return calls

    @staticmethod
    def _same_ranges(a: KMNC, b: KMNC) -> bool:
        return torch.equal(a.mins, b.mins) and torch.equal(a.maxs, b.maxs)

    def _call_tables(self, call, device) -> dict:
        """Keyword arguments of ``ops.coverage_suite`` for one call."""
        m = self.metrics

        def stack(ids, attr):
            if not ids:
                return None
            return torch.stack(
                [getattr(m[i], attr).to(device).float() for i in ids]
            ).contiguous()

        kmnc = [m[i] for i in call["kmnc"]]
        return dict(
            nac_thresholds=tuple(m[i].cov_threshold for i in call["nac"]),
            upper_bounds=stack(call["snac"], "max_boundaries"),
            nbc_lower=stack(call["nbc"], "min_boundaries"),
            nbc_upper=stack(call["nbc"], "max_boundaries"),
            kmnc_mins=kmnc[0].mins.to(device).float().contiguous() if kmnc else None,
            kmnc_maxs=kmnc[0].maxs.to(device).float().contiguous() if kmnc else None,
            kmnc_sections=tuple(k.sections for k in kmnc),
            tknc_ks=tuple(m[i].top_neurons for i in call["tknc"]),
        )

    def __call__(
        self, activations: List[torch.Tensor]
    ) -> Dict[str, Tuple[torch.Tensor, BitProfile]]:
        layers = [
            l.reshape(l.shape[0], -1).float().contiguous() for l in activations
        ]
        device = layers[0].device
        if device not in self._tables:
            self._tables[device] = [
                self._call_tables(call, device) for call in self._calls
            ]
        k = sum(l.shape[1] for l in layers)
        done = {}
        for call, tables in zip(self._calls, self._tables[device]):
            out = ops.coverage_suite(layers, **tables)
            for fam, ids in call.items():
                for metric_id, (words, scores) in zip(ids, out[fam]):
                    per_neuron = (
                        2 if fam == "nbc"
                        else self.metrics[metric_id].sections if fam == "kmnc"
                        else 1
                    )
                    done[metric_id] = (scores, BitProfile(words, k * per_neuron))
        return {metric_id: done[metric_id] for metric_id in self.metrics}
