"""Batched CAM on the CPU: ``ops.cam_order_many`` against the per-problem
``ops.cam_order``, ``core.prioritizers.cam_many`` against ``cam``, and the
``cam_mode`` of CoverageWorker and SurpriseHandler end to end."""

import random

import numpy as np
import pytest
import torch

from simple_tip_amd import ops
from simple_tip_amd.core import prioritizers
from simple_tip_amd.core.bitmap import BitProfile
from simple_tip_amd.core.prioritizers import cam, cam_many
from simple_tip_amd.engine.coverage_handler import CoverageWorker
from simple_tip_amd.engine.model_handler import BaseModel
from simple_tip_amd.engine.surprise_handler import SurpriseHandler
from simple_tip_amd.models import MnistCNN
from simple_tip_amd.ops import fallback


def _problem(seed, rows, nbits, density, garbage=False):
    """(scores, int64 words [rows, ceil(nbits/64)], nbits); the scores take
    four values only, so stability decides the leftover order."""
    rng = np.random.RandomState(seed)
    bools = torch.from_numpy(rng.rand(rows, nbits) < density)
    words = fallback.pack_bits(bools)
    if garbage:  # bits past nbits are not part of the profile
        tail = nbits % 64
        assert tail
        junk = torch.from_numpy(rng.randint(1, 2 ** 20, size=rows)) << tail
        words = words.clone()
        words[:, -1] |= junk
    scores = torch.from_numpy(rng.randint(0, 4, size=rows).astype(np.float32))
    return scores, words.contiguous(), nbits


def _five_problems():
    return [
        _problem(1, 37, 128, 0.1),
        _problem(2, 50, 100, 0.1, garbage=True),  # tail bits 100..127 dirty
        _problem(3, 20, 300, 0.0),                # all-zero profile
        _problem(4, 1, 70, 0.3),                  # a single row
        _problem(5, 90, 1000, 0.02),
    ]


def test_cam_order_many_equals_per_problem_cam_order():
    probs = _five_problems()
    got = ops.cam_order_many(*zip(*probs))
    assert len(got) == 5
    for (scores, words, nbits), order in zip(probs, got):
        want = ops.cam_order(scores, words, nbits)
        assert order.dtype == torch.int64
        assert sorted(order.tolist()) == list(range(scores.shape[0]))
        assert torch.equal(order, want)
    # the garbage was really there, and ignoring it matters
    _, dirty, nbits = probs[1]
    assert (dirty[:, -1] >> (nbits % 64)).any()
    # the all-zero profile is ordered by score alone
    zs, zw, zb = probs[2]
    assert torch.equal(got[2], torch.argsort(zs, descending=True, stable=True))
    # a problem's order does not depend on its neighbours or their order
    rev = ops.cam_order_many(*zip(*probs[::-1]))[::-1]
    for a, b in zip(got, rev):
        assert torch.equal(a, b)


def test_cam_order_many_empty_cases():
    assert ops.cam_order_many([], [], []) == []
    assert fallback.cam_order_many([], [], []) == []
    scores = torch.zeros(0)
    words = torch.zeros(0, 2, dtype=torch.int64)
    other = _problem(6, 9, 128, 0.2)
    got = ops.cam_order_many([scores, other[0]], [words, other[1]], [128, 128])
    assert got[0].shape == (0,) and got[0].dtype == torch.int64
    assert torch.equal(got[1], ops.cam_order(*other))
    with pytest.raises(ValueError):
        ops.cam_order_many([scores], [words, words], [128])


def test_cam_many_equals_cam_for_profiles_and_bool_matrices():
    rng = np.random.RandomState(7)
    bools = [
        rng.rand(40, 130) < 0.1,
        rng.rand(25, 64) < 0.3,
        rng.rand(12, 3, 50) < 0.05,  # higher rank: flattened per sample
    ]
    scores = [rng.rand(b.shape[0]).astype(np.float32) for b in bools]
    want = [list(cam(s, b)) for s, b in zip(scores, bools)]
    # bool matrices as numpy, as tensors, and packed BitProfiles
    assert cam_many(scores, bools) == want
    assert cam_many(scores, [torch.from_numpy(b) for b in bools]) == want
    profiles = [
        BitProfile.from_bool(torch.from_numpy(b).reshape(b.shape[0], -1))
        for b in bools
    ]
    assert cam_many([torch.from_numpy(s) for s in scores], profiles) == want
    assert cam_many([], []) == []
    with pytest.raises(ValueError):
        cam_many(scores, bools[:2])


def test_cam_many_makes_one_batched_call(monkeypatch):
    calls = []
    real = ops.cam_order_many

    def spy(scores, words, nbits):
        calls.append(len(words))
        return real(scores, words, nbits)

    monkeypatch.setattr(prioritizers.ops, "cam_order_many", spy)
    rng = np.random.RandomState(8)
    bools = [rng.rand(10, 70) < 0.2 for _ in range(3)]
    cam_many([rng.rand(10) for _ in range(3)], bools)
    assert calls == [3]


def _base(model, batch):
    return BaseModel(model, [0, 1, 2, 3], device=torch.device("cpu"), predict_batch=batch)


def test_coverage_worker_batched_equals_the_default(monkeypatch):
    monkeypatch.delenv("TIP_CAM_MODE", raising=False)
    monkeypatch.delenv("TIP_NC_MODE", raising=False)
    torch.manual_seed(0)
    model = MnistCNN().eval()
    train = np.random.RandomState(0).rand(80, 1, 28, 28).astype(np.float32)
    test = np.random.RandomState(1).rand(48, 1, 28, 28).astype(np.float32)

    many_calls = []
    real = ops.cam_order_many

    def spy(scores, words, nbits):
        many_calls.append(len(words))
        return real(scores, words, nbits)

    monkeypatch.setattr(prioritizers.ops, "cam_order_many", spy)

    def run(**kw):
        worker = CoverageWorker(_base(model, 32), train, **kw)
        return worker, worker.evaluate_all(test, "nominal")

    default, (t_def, s_def, o_def) = run()
    assert default.cam_mode == "per_metric"
    assert many_calls == []  # the default never touches the batched op
    batched, (t_bat, s_bat, o_bat) = run(cam_mode="batched")
    assert batched.cam_mode == "batched"
    assert many_calls == [12]  # one call for all 12 metrics
    assert list(s_bat) == list(s_def) and len(s_def) == 12
    assert list(o_bat) == list(o_def)
    for metric_id in s_def:
        assert np.array_equal(s_bat[metric_id], s_def[metric_id]), metric_id
        assert o_bat[metric_id] == o_def[metric_id], metric_id
        assert sorted(o_bat[metric_id]) == list(range(48))
        assert len(t_bat[metric_id]) == len(t_def[metric_id]) == 4
    # every metric's cam slot is charged the whole batched call
    cam_slots = {t_bat[m][3] for m in t_bat}
    assert len(cam_slots) == 1 and cam_slots.pop() > 0.0


def _seed_all():
    torch.manual_seed(1)
    np.random.seed(1)
    random.seed(1)


def test_surprise_handler_batched_equals_the_default(monkeypatch):
    monkeypatch.delenv("TIP_CAM_MODE", raising=False)
    monkeypatch.delenv("TIP_MODAL_SA_MODE", raising=False)
    rng = np.random.RandomState(2)
    train = rng.rand(120, 1, 28, 28).astype(np.float32)
    datasets = {
        "nominal": rng.rand(40, 1, 28, 28).astype(np.float32),
        "ood": rng.rand(40, 1, 28, 28).astype(np.float32),
    }
    many_calls = []
    real = ops.cam_order_many

    def spy(scores, words, nbits):
        many_calls.append(len(words))
        return real(scores, words, nbits)

    monkeypatch.setattr(prioritizers.ops, "cam_order_many", spy)
    results = {}
    for mode in ("per_metric", "batched"):
        _seed_all()
        model = MnistCNN().eval()
        sh = SurpriseHandler(
            model, sa_layers=[3], training_dataset=train,
            device=torch.device("cpu"), predict_batch=32, cam_mode=mode,
        )
        assert sh.cam_mode == mode
        results[mode] = sh.evaluate_all(datasets)
    assert many_calls == [10]  # five SAs x two datasets, one call
    assert list(results["batched"]) == list(results["per_metric"])
    assert set(results["batched"]) == {"dsa", "pc-lsa", "pc-mdsa", "pc-mlsa", "pc-mmdsa"}
    slots = set()
    for name, per_ds in results["batched"].items():
        for ds_name in datasets:
            scores, order, times = per_ds[ds_name]
            ref_scores, ref_order, ref_times = results["per_metric"][name][ds_name]
            assert scores.dtype == ref_scores.dtype and scores.shape == (40,)
            assert np.array_equal(scores, ref_scores, equal_nan=True), (name, ds_name)
            assert isinstance(order, np.ndarray)
            assert order.tolist() == ref_order.tolist(), (name, ds_name)
            assert sorted(order.tolist()) == list(range(40))
            assert len(times) == len(ref_times) == 4
            slots.add(times[3])
    assert len(slots) == 1 and slots.pop() > 0.0  # the whole call, each


def test_cam_mode_env_override_and_bad_values(monkeypatch):
    monkeypatch.delenv("TIP_CAM_MODE", raising=False)
    model = MnistCNN().eval()
    train = np.zeros((4, 1, 28, 28), dtype=np.float32)

    def surprise(**kw):
        return SurpriseHandler(
            model, sa_layers=[3], training_dataset=train,
            device=torch.device("cpu"), predict_batch=4, **kw,
        )

    with pytest.raises(ValueError, match="cam_mode"):
        CoverageWorker(_base(model, 4), train, cam_mode="nope")
    with pytest.raises(ValueError, match="cam_mode"):
        surprise(cam_mode="nope")
    assert CoverageWorker(_base(model, 4), train).cam_mode == "per_metric"
    assert surprise().cam_mode == "per_metric"
    monkeypatch.setenv("TIP_CAM_MODE", "bogus")
    with pytest.raises(ValueError, match="cam_mode"):
        CoverageWorker(_base(model, 4), train)
    with pytest.raises(ValueError, match="cam_mode"):
        surprise()
    monkeypatch.setenv("TIP_CAM_MODE", "batched")
    assert CoverageWorker(_base(model, 4), train).cam_mode == "batched"
    assert surprise().cam_mode == "batched"
    # the environment wins over the argument
    monkeypatch.setenv("TIP_CAM_MODE", "per_metric")
    assert CoverageWorker(_base(model, 4), train, cam_mode="batched").cam_mode == "per_metric"
    assert surprise(cam_mode="batched").cam_mode == "per_metric"
