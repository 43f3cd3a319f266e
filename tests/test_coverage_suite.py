"""The fused coverage suite without a GPU: the fallback op against the
per-metric fallbacks, CoverageSuite against the metric objects, the error
contract, and CoverageWorker's ``nc_mode`` end to end on the CPU."""

import numpy as np
import pytest
import torch

from simple_tip_amd import ops
from simple_tip_amd.core import neuron_coverage as nc
from simple_tip_amd.engine.coverage_handler import CoverageWorker
from simple_tip_amd.engine.model_handler import BaseModel
from simple_tip_amd.models import MnistCNN
from simple_tip_amd.ops import fallback

WIDTHS = [70, 64, 1, 130]
N = 5
# the canon of CoverageWorker
NAC_THRESHOLDS = (0.0, 0.75)
SCALERS = (0, 0.5, 1)
KMNC_SECTIONS = (2,)
TKNC_KS = (1, 2, 3)


@pytest.fixture(scope="module")
def case():
    rng = np.random.RandomState(0)
    # post-ReLU-like: mostly exact zeros, so the TKNC cut falls inside ties
    layers = [
        torch.from_numpy(np.maximum(rng.randn(N, k), 0).astype(np.float32))
        for k in WIDTHS
    ]
    mins = [torch.from_numpy(rng.randn(k).astype(np.float32)) - 1 for k in WIDTHS]
    maxs = [
        m + torch.from_numpy(rng.rand(m.shape[0]).astype(np.float32)) + 0.5
        for m in mins
    ]
    stds = [torch.from_numpy(rng.rand(k).astype(np.float32)) for k in WIDTHS]
    return layers, mins, maxs, stds


def _canon_metrics(mins, maxs, stds):
    metrics = {}
    for s in SCALERS:
        metrics[f"NBC_{s:g}"] = nc.NBC(mins=mins, maxs=maxs, stds=stds, scaler=s)
    for s in SCALERS:
        metrics[f"SNAC_{s:g}"] = nc.SNAC(maxs=maxs, stds=stds, scaler=s)
    for t in NAC_THRESHOLDS:
        metrics[f"NAC_{t:g}"] = nc.NAC(cov_threshold=t)
    for k in TKNC_KS:
        metrics[f"TKNC_{k}"] = nc.TKNC(top_neurons=k)
    for s in KMNC_SECTIONS:
        metrics[f"KMNC_{s}"] = nc.KMNC(mins, maxs, sections=s)
    return metrics


def test_fallback_suite_equals_the_per_metric_fallbacks(case):
    layers, mins, maxs, stds = case
    acts = torch.cat(layers, dim=1)
    lo, hi, sd = torch.cat(mins), torch.cat(maxs), torch.cat(stds)
    upper = torch.stack([hi + s * sd for s in SCALERS])
    lower = torch.stack([lo - s * sd for s in SCALERS])
    out = fallback.coverage_suite(
        layers, NAC_THRESHOLDS, upper, lower, upper, lo, hi, KMNC_SECTIONS, TKNC_KS
    )
    want = {
        "nac": [fallback.nac_profile(acts, t) for t in NAC_THRESHOLDS],
        "snac": [fallback.snac_profile(acts, u) for u in upper],
        "nbc": [fallback.nbc_profile(acts, l, u) for l, u in zip(lower, upper)],
        "kmnc": [fallback.kmnc_profile(acts, lo, hi, s) for s in KMNC_SECTIONS],
        "tknc": [fallback.tknc_profile(layers, k) for k in TKNC_KS],
    }
    assert list(out) == list(fallback.COVERAGE_SUITE_FAMILIES)
    for fam, words in want.items():
        assert len(out[fam]) == len(words)
        for (got_w, got_s), w in zip(out[fam], words):
            assert got_w.dtype == torch.int64 and got_s.dtype == torch.int64
            assert torch.equal(got_w, w)
            assert torch.equal(got_s, fallback.popcount_rows(w))
    # the dispatcher routes CPU tensors to the same function
    again = ops.coverage_suite(layers, nac_thresholds=NAC_THRESHOLDS, tknc_ks=(2,))
    assert torch.equal(again["nac"][1][0], want["nac"][1])
    assert torch.equal(again["tknc"][0][0], want["tknc"][1])
    assert again["snac"] == again["nbc"] == again["kmnc"] == []


def test_coverage_suite_equals_the_metric_objects(case):
    layers, mins, maxs, stds = case
    metrics = _canon_metrics(mins, maxs, stds)
    # taps arrive unflattened: [N, C, H, W] for the first layer
    taps = [layers[0].reshape(N, 7, 5, 2)] + layers[1:]
    got = nc.CoverageSuite(metrics)(taps)
    assert list(got) == list(metrics)
    for metric_id, metric in metrics.items():
        scores, prof = metric(taps)
        assert torch.equal(got[metric_id][0], scores), metric_id
        assert got[metric_id][1].nbits == prof.nbits, metric_id
        assert torch.equal(got[metric_id][1].words, prof.words), metric_id


def test_coverage_suite_splits_what_exceeds_one_call(case, monkeypatch):
    layers, mins, maxs, stds = case
    metrics = {f"NAC_{i}": nc.NAC(cov_threshold=0.1 * i) for i in range(6)}
    metrics["KMNC_a"] = nc.KMNC(mins, maxs, sections=3)
    metrics["KMNC_b"] = nc.KMNC(mins, [m + 1 for m in maxs], sections=3)
    calls = []
    real = ops.coverage_suite

    def spy(layers_, **kw):
        calls.append(kw)
        return real(layers_, **kw)

    monkeypatch.setattr(ops, "coverage_suite", spy)
    got = nc.CoverageSuite(metrics)(layers)
    # six thresholds need two calls; the two range tables one call each
    assert len(calls) == 2
    assert all(len(kw["nac_thresholds"]) <= 4 for kw in calls)
    assert all(len(kw["kmnc_sections"]) == 1 for kw in calls)
    for metric_id, metric in metrics.items():
        scores, prof = metric(layers)
        assert torch.equal(got[metric_id][0], scores), metric_id
        assert torch.equal(got[metric_id][1].words, prof.words), metric_id


def test_error_contract(monkeypatch):
    class Other(nc.CoverageMethod):
        def __call__(self, activations):
            raise AssertionError("never evaluated")

    with pytest.raises(TypeError, match="Other"):
        nc.CoverageSuite({"NAC_0": nc.NAC(0.0), "X": Other()})

    monkeypatch.delenv("TIP_NC_MODE", raising=False)
    model = MnistCNN().eval()
    train = np.zeros((4, 1, 28, 28), dtype=np.float32)

    def base():
        return BaseModel(model, [0, 1, 2, 3], device=torch.device("cpu"), predict_batch=4)

    with pytest.raises(ValueError, match="nc_mode"):
        CoverageWorker(base(), train, nc_mode="nope")
    monkeypatch.setenv("TIP_NC_MODE", "bogus")
    with pytest.raises(ValueError, match="nc_mode"):
        CoverageWorker(base(), train)
    monkeypatch.setenv("TIP_NC_MODE", "fused")
    assert CoverageWorker(base(), train).nc_mode == "fused"


def test_worker_fused_mode_equals_the_default(monkeypatch):
    monkeypatch.delenv("TIP_NC_MODE", raising=False)
    torch.manual_seed(0)
    model = MnistCNN().eval()
    rng = np.random.RandomState(0)
    train = rng.rand(96, 1, 28, 28).astype(np.float32)
    test = rng.rand(96, 1, 28, 28).astype(np.float32)

    suite_calls = []
    real = ops.coverage_suite

    def spy(layers, **kw):
        suite_calls.append(layers[0].shape[0])
        return real(layers, **kw)

    monkeypatch.setattr(ops, "coverage_suite", spy)

    def run(**kw):
        worker = CoverageWorker(
            BaseModel(model, [0, 1, 2, 3], device=torch.device("cpu"), predict_batch=32),
            train, **kw,
        )
        return worker, worker.evaluate_all(test, "nominal")

    default, (t_def, s_def, o_def) = run()
    assert default.nc_mode == "per_metric"
    assert suite_calls == []  # the default never touches the suite
    fused, (t_fus, s_fus, o_fus) = run(nc_mode="fused")
    assert suite_calls == [32, 32, 32]  # one suite call per batch
    assert list(s_fus) == list(s_def) and len(s_def) == 12
    for metric_id in s_def:
        assert np.array_equal(s_fus[metric_id], s_def[metric_id]), metric_id
        assert o_fus[metric_id] == o_def[metric_id], metric_id
        assert len(t_fus[metric_id]) == len(t_def[metric_id]) == 4
    # every metric is charged the whole suite call
    quant = {t_fus[m][2] for m in t_fus}
    assert len(quant) == 1 and quant.pop() > 0.0
