"""Grouped Gaussian scoring (pc-MDSA / pc-MLSA / pc-MMDSA), CPU side: the
fallback op against a direct per-component einsum, MultiModalSA.fuse()
against the per-mode loop, unseen-mode semantics, and the handler switch."""

import warnings

import numpy as np
import pytest
import torch

from simple_tip_amd import ops
from simple_tip_amd.core import surprise
from simple_tip_amd.core.surprise import (
    LSA,
    MDSA,
    MLSA,
    GroupedGaussianSA,
    MultiModalSA,
)
from simple_tip_amd.ops import fallback


def _spd(gen, d):
    a = torch.randn(d, d, generator=gen, dtype=torch.float64)
    return a @ a.t() / d + 0.1 * torch.eye(d, dtype=torch.float64)


def _tables(gen, counts, d):
    j = sum(counts)
    means = torch.randn(j, d, generator=gen, dtype=torch.float64)
    mats = torch.stack([_spd(gen, d) for _ in range(j)])
    logc = torch.randn(j, generator=gen, dtype=torch.float64)
    off = torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int32)
    return off, means, mats, logc


def test_fallback_mixture_matches_einsum():
    gen = torch.Generator().manual_seed(0)
    d = 9
    counts = [1, 3, 0, 2, 1]  # ragged; group 2 has no component
    off, means, mats, logc = _tables(gen, counts, d)
    n = 60
    x = torch.randn(n, d, generator=gen, dtype=torch.float64)
    group = torch.randint(0, 4, (n,), generator=gen)  # group 4 gets no row
    group[:3] = torch.tensor([-1, 5, 2])  # out of range, and the empty group
    got = ops.grouped_gaussian_scores(x, group, off, means, mats, logc)
    assert got.dtype == torch.float64 and got.shape == (n,)

    # direct: every row against every component, then pick the group's
    diff = x[:, None, :] - means[None]
    q = torch.einsum("njd,jde,nje->nj", diff, mats, diff)
    terms = logc[None] - 0.5 * q
    want = torch.full((n,), float("inf"), dtype=torch.float64)
    for i in range(n):
        g = int(group[i])
        if 0 <= g < len(counts) and counts[g] > 0:
            want[i] = -torch.logsumexp(terms[i, off[g] : off[g + 1]], dim=0)
    assert torch.isinf(got[:3]).all() and (got[:3] > 0).all()
    assert (int((group == 2).sum()) >= 1) and torch.isinf(got[group == 2]).all()
    torch.testing.assert_close(got, want, rtol=1e-12, atol=1e-12)


def test_fallback_mahalanobis_matches_einsum():
    gen = torch.Generator().manual_seed(1)
    d = 7
    off, means, mats, _ = _tables(gen, [1, 1, 1], d)
    x = torch.randn(40, d, generator=gen, dtype=torch.float64)
    group = torch.randint(0, 3, (40,), generator=gen)
    group[0], group[1] = -1, 3
    got = fallback.grouped_gaussian_scores(x, group, off, means, mats)
    gc = group.clamp(0, 2)
    diff = x - means[gc]
    want = torch.einsum("nd,nde,ne->n", diff, mats[gc], diff)
    want[:2] = float("inf")
    torch.testing.assert_close(got, want, rtol=1e-12, atol=1e-12)


def test_envelope_errors():
    gen = torch.Generator().manual_seed(2)
    d = 4
    x = torch.randn(5, d, generator=gen, dtype=torch.float64)
    group = torch.zeros(5, dtype=torch.int64)
    off, means, mats, logc = _tables(gen, [9], d)
    with pytest.raises(ValueError, match="components per group"):
        ops.grouped_gaussian_scores(x, group, off, means, mats, logc)
    off, means, mats, logc = _tables(gen, [1] * 257, d)
    with pytest.raises(ValueError, match="groups"):
        ops.grouped_gaussian_scores(x, group, off, means, mats, logc)
    off, means, mats, logc = _tables(gen, [2, 1], d)
    with pytest.raises(ValueError, match="contiguous"):
        ops.grouped_gaussian_scores(
            x, group, off, means, mats.transpose(1, 2), logc
        )
    with pytest.raises(ValueError, match="exactly one component"):
        ops.grouped_gaussian_scores(x, group, off, means, mats)


# --- MultiModalSA.fuse() against the per-mode loop ---------------------------

D = 12


def _ats(seed, n, classes=3):
    rng = np.random.RandomState(seed)
    pred = rng.randint(0, classes, size=n)
    centers = rng.randn(classes, D) * 3.0
    ats = centers[pred] + rng.randn(n, D) * (1.0 + 0.3 * pred[:, None])
    return torch.from_numpy(ats), torch.from_numpy(pred)


@pytest.fixture(scope="module")
def fitted():
    np.random.seed(0)  # sklearn's EM seeds from the process RNG
    train, train_pred = _ats(0, 360)
    return {
        "pc-mdsa": MultiModalSA.build_by_class(
            train, train_pred, lambda a, p: MDSA(a)
        ),
        "pc-mlsa": MultiModalSA.build_by_class(
            train, train_pred, lambda a, p: MLSA(a, num_components=3)
        ),
        "pc-mmdsa": MultiModalSA.build_with_kmeans(
            train, train_pred, lambda a, p: MDSA(a),
            potential_k=range(2, 4), n_init=2, max_iter=50,
        ),
    }


@pytest.mark.parametrize("name", ["pc-mdsa", "pc-mlsa", "pc-mmdsa"])
def test_fuse_equals_per_mode(fitted, name):
    test, test_pred = _ats(1, 240)
    sa = fitted[name]
    fused = sa.fuse()
    assert isinstance(fused, GroupedGaussianSA)
    want = sa(test, test_pred)
    got = fused(test, test_pred)
    assert got.dtype == torch.float64 and got.shape == want.shape
    assert torch.isfinite(want).all()
    torch.testing.assert_close(got, want, rtol=1e-9, atol=0.0)


def test_unseen_mode_warns_then_raises_in_strict_mode(fitted):
    test, test_pred = _ats(2, 50)
    test_pred = test_pred.clone()
    test_pred[::7] = 5  # a class never predicted on the training set
    sa = fitted["pc-mdsa"]
    fused = sa.fuse()
    with pytest.warns(UserWarning, match="No modal found for modal id 5"):
        got = fused(test, test_pred)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want = sa(test, test_pred)
    assert torch.isinf(got[::7]).all() and (got[::7] > 0).all()
    torch.testing.assert_close(got, want, rtol=1e-9, atol=0.0)
    prev = surprise.set_strict_modes(True)
    try:
        with pytest.raises(ValueError, match="No modal found"):
            fused(test, test_pred)
    finally:
        surprise.set_strict_modes(prev)


def test_fuse_rejects_non_gaussian_modes():
    train, train_pred = _ats(3, 120)
    lsa = MultiModalSA.build_by_class(train, train_pred, lambda a, p: LSA(a))
    with pytest.raises(TypeError):
        lsa.fuse()


def test_handler_fused_mode_keeps_the_result_taxonomy(monkeypatch):
    from simple_tip_amd.engine.surprise_handler import SurpriseHandler
    from simple_tip_amd.models import MnistCNN

    monkeypatch.delenv("TIP_MODAL_SA_MODE", raising=False)
    rng = np.random.RandomState(2)
    train = rng.rand(120, 1, 28, 28).astype(np.float32)
    nominal = rng.rand(40, 1, 28, 28).astype(np.float32)
    results = {}
    for mode in ("per_mode", "fused"):
        torch.manual_seed(1)
        model = MnistCNN().eval()
        sh = SurpriseHandler(
            model, sa_layers=[3], training_dataset=train,
            device=torch.device("cpu"), predict_batch=32, modal_sa_mode=mode,
        )
        assert sh.modal_sa_mode == mode
        results[mode] = sh.evaluate_all({"nominal": nominal})
    assert set(results["fused"]) == set(results["per_mode"])
    for name, per_ds in results["fused"].items():
        scores, cam_order, times = per_ds["nominal"]
        ref_scores, ref_order, ref_times = results["per_mode"][name]["nominal"]
        assert scores.shape == ref_scores.shape == (40,)
        assert scores.dtype == ref_scores.dtype
        assert sorted(cam_order.tolist()) == list(range(40))
        assert len(times) == len(ref_times) == 4
    with pytest.raises(ValueError):
        SurpriseHandler(
            MnistCNN().eval(), sa_layers=[3], training_dataset=train,
            device=torch.device("cpu"), modal_sa_mode="nope",
        )
    monkeypatch.setenv("TIP_MODAL_SA_MODE", "fused")
    sh = SurpriseHandler(
        MnistCNN().eval(), sa_layers=[3], training_dataset=train,
        device=torch.device("cpu"), predict_batch=32,
    )
    assert sh.modal_sa_mode == "fused"
