"""Fused VR under input sharding: ``eval_prioritization``'s ``dist_shard``
path passes each shard's global start row, so the per-rank VR pieces are the
single-process VR, bit for bit. The ranks are simulated in one process (the
collectives themselves are covered by tests/test_dist_shard.py)."""

import numpy as np
import torch

from simple_tip_amd import config
from simple_tip_amd.engine import eval_prioritization
from simple_tip_amd.models import MnistCNN
from simple_tip_amd.parallel import dist as pdist

WORLD = 3
N = 41  # uneven shards: 14, 14, 13


def _run(monkeypatch, model, x, labels, rank=None):
    """uncertainty_VR as one rank persists it (rank None: unsharded)."""
    got = {}
    monkeypatch.setattr(
        eval_prioritization, "_persist",
        lambda cs, ds, data_type, mid, data: got.__setitem__(data_type, data),
    )
    monkeypatch.setattr(
        eval_prioritization, "_persist_times_multiple_metrics",
        lambda *a, **k: None,
    )
    if rank is not None:
        real_slice = pdist.shard_slice
        monkeypatch.setattr(pdist, "get_world_size", lambda: WORLD)
        monkeypatch.setattr(
            pdist, "shard_slice", lambda n: real_slice(n, rank, WORLD)
        )

        def place(local, n_total):
            # this rank's rows at their global position, NaN-free filler 0
            full = torch.zeros((n_total,) + tuple(local.shape[1:]), dtype=local.dtype)
            full[real_slice(n_total, rank, WORLD)] = local
            return full

        monkeypatch.setattr(pdist, "allgather_rows", place)
    eval_prioritization._eval_fault_predictors(
        "shardcheck", model, 0, x, labels, "nominal",
        torch.device("cpu"), 8, dist_shard=rank is not None,
    )
    return got["uncertainty_VR"]


def test_sharded_fused_vr_equals_single_process(monkeypatch):
    monkeypatch.setattr(config, "VR_MODE", "fused")
    torch.manual_seed(0)
    model = MnistCNN()
    x = torch.randn(N, 1, 28, 28).numpy()
    labels = np.zeros(N, dtype=np.int64)

    with monkeypatch.context() as m:
        single = _run(m, model, x, labels)
    assert single.shape == (N,) and single.std() > 0

    pieces = np.zeros(N, dtype=single.dtype)
    for rank in range(WORLD):
        with monkeypatch.context() as m:
            part = _run(m, model, x, labels, rank)
        sl = pdist.shard_slice(N, rank, WORLD)
        pieces[sl] = part[sl]
    assert np.array_equal(pieces, single)
