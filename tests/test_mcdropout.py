"""Fused MC-dropout head on the CPU: the stateless mask generator, the
``mc_dropout_votes`` fallback (the oracle of the HIP kernel), the
``TapModel.dropout_head`` detector and ``BaseModel``'s ``vr_mode``."""

import math

import numpy as np
import pytest
import torch

from simple_tip_amd import config, ops
from simple_tip_amd.engine.model_handler import BaseModel
from simple_tip_amd.models import Cifar10CNN, ImdbTransformer, MnistCNN, ResNet20
from simple_tip_amd.ops import fallback


def int_problem(n, d, c, seed=0):
    """Integer-valued head: every partial sum is exact in float32."""
    g = torch.Generator().manual_seed(seed)
    feats = torch.randint(-3, 4, (n, d), generator=g).float()
    weight = torch.randint(-2, 3, (c, d), generator=g).float()
    bias = torch.randint(-3, 4, (c,), generator=g).float()
    return feats, weight, bias


def dense_votes(feats, weight, bias, p, S, seed, row_offset=0):
    """Independent reconstruction: mask -> masked einsum -> argmax -> bincount.

    Returns (votes [N, C], tie fraction over (s, n) pairs)."""
    n, d = feats.shape
    c = weight.shape[0]
    keep = fallback.dropout_keep_mask(seed, S, n, d, p, row_offset)
    scale = np.float32(1.0 / (1.0 - p))
    sums = torch.einsum("snd,cd->snc", keep.float() * feats[None], weight)
    logits = (torch.from_numpy(np.asarray(scale)) * sums + bias).numpy()
    best = np.argmax(logits, axis=2)  # numpy: first maximal index
    votes = np.zeros((n, c), dtype=np.int32)
    for i in range(n):
        votes[i] = np.bincount(best[:, i], minlength=c)
    top = np.sort(logits, axis=2)
    ties = float((top[..., -1] == top[..., -2]).mean()) if c > 1 else 0.0
    return torch.from_numpy(votes), ties


# -- 1. golden values --------------------------------------------------------

GOLDEN_WORDS = [
    (0, 0, 0, 0, 0xC7F0BDFE),
    (1, 0, 0, 0, 0x3CF7483E),
    (1234, 199, 9999, 1599, 0x7BD2B9BE),
    ((5 << 32) | 7, 3, 70000, 2047, 0xE879609B),
    (2 ** 64 - 1, 65534, 1, 1, 0x0CC5A2F4),
]


@pytest.mark.parametrize("seed,s,g,d,word", GOLDEN_WORDS)
def test_golden_words(seed, s, g, d, word):
    # words[s, 0, d] of a 1-row call whose row 0 is global row g
    words = fallback.dropout_words(seed, s + 1, 1, d + 1, row_offset=g)
    assert int(words[s, 0, d]) == word


def test_golden_mask_row_and_thresholds():
    keep = fallback.dropout_keep_mask(1234, 1, 1, 8, 0.5)
    assert keep.dtype == torch.bool and keep.shape == (1, 1, 8)
    assert keep[0, 0].int().tolist() == [1, 1, 0, 1, 0, 1, 1, 0]
    assert fallback.dropout_threshold(0.1) == 429496729
    assert fallback.dropout_threshold(0.5) == 2147483648
    assert fallback.dropout_threshold(0.9) == 3865470566
    assert fallback.dropout_threshold(0.0) == 0
    assert bool(fallback.dropout_keep_mask(7, 3, 5, 11, 0.0).all())


# -- 2. mask statistics ------------------------------------------------------


def _lag1_corr(x, dim):
    a = x.narrow(dim, 0, x.shape[dim] - 1).reshape(-1).double()
    b = x.narrow(dim, 1, x.shape[dim] - 1).reshape(-1).double()
    return float(np.corrcoef(a.numpy(), b.numpy())[0, 1])


@pytest.mark.parametrize("p", [0.1, 0.5, 0.9])
def test_mask_statistics(p):
    S, N, D = 200, 64, 1600
    keep = fallback.dropout_keep_mask(0, S, N, D, p)
    count = keep.numel()
    rate = float(keep.double().mean())
    print(f"p={p} keep rate {rate:.6f} (want {1 - p})")
    assert abs(rate - (1 - p)) < 5 * math.sqrt(p * (1 - p) / count)
    for dim, name in enumerate("sgd"):
        corr = _lag1_corr(keep, dim)
        print(f"p={p} lag-1 corr along {name}: {corr:.2e}")
        assert abs(corr) < 5 / math.sqrt(count)
    other = fallback.dropout_keep_mask(1, S, N, D, p)
    cross = float(
        np.corrcoef(
            keep.reshape(-1).double().numpy(), other.reshape(-1).double().numpy()
        )[0, 1]
    )
    print(f"p={p} seed 0 vs 1 corr: {cross:.2e}")
    assert abs(cross) < 5 / math.sqrt(count)


# -- 3. votes against the dense reconstruction -------------------------------


@pytest.mark.parametrize("p", [0.5, 0.1])
def test_votes_match_dense_reconstruction(p):
    feats, weight, bias = int_problem(37, 193, 10)
    want, ties = dense_votes(feats, weight, bias, p, 200, seed=11)
    got = ops.mc_dropout_votes(feats, weight, bias, p, 200, 11)
    assert got.dtype == torch.int32 and got.shape == (37, 10)
    print(f"p={p}: exact ties on {100 * ties:.2f}% of (s, n) pairs")
    assert ties > 0, "data must exercise the lowest-index tie rule"
    assert torch.equal(got, want)


def test_votes_chunking_is_invisible(monkeypatch):
    feats, weight, bias = int_problem(37, 193, 10, seed=3)
    want = fallback.mc_dropout_votes(feats, weight, bias, 0.5, 200, 5, 17)
    # 5 rows per chunk, last chunk partial
    monkeypatch.setattr(fallback, "_MCD_MAX_MASK_ELEMS", 5 * 200 * 193)
    got = fallback.mc_dropout_votes(feats, weight, bias, 0.5, 200, 5, 17)
    assert torch.equal(got, want)


# -- 4. edge cases -----------------------------------------------------------


def test_p_zero_votes_deterministic_argmax():
    feats, weight, bias = int_problem(19, 50, 7, seed=1)
    votes = ops.mc_dropout_votes(feats, weight, bias, 0.0, 33, 9)
    logits = (feats @ weight.t() + bias).numpy()
    want = np.zeros((19, 7), dtype=np.int32)
    want[np.arange(19), np.argmax(logits, axis=1)] = 33
    assert torch.equal(votes, torch.from_numpy(want))


def test_zero_row_votes_argmax_bias_and_zero_head_votes_class0():
    feats, weight, bias = int_problem(6, 40, 5, seed=2)
    feats[2] = 0
    bias = torch.tensor([-1.0, 2.0, 0.5, 2.0, -3.0])  # tie: lowest index
    votes = ops.mc_dropout_votes(feats, weight, bias, 0.5, 50, 1)
    assert votes[2].tolist() == [0, 50, 0, 0, 0]
    zero = ops.mc_dropout_votes(
        feats, torch.zeros_like(weight), torch.zeros(5), 0.5, 50, 1
    )
    assert torch.equal(zero[:, 0], torch.full((6,), 50, dtype=torch.int32))
    assert int(zero[:, 1:].sum()) == 0


def test_single_sample_rowsum_determinism_and_seed():
    feats, weight, bias = int_problem(23, 77, 10, seed=4)
    one = ops.mc_dropout_votes(feats, weight, bias, 0.5, 1, 3)
    assert torch.equal(one.sum(dim=1), torch.ones(23, dtype=torch.int32))
    a = ops.mc_dropout_votes(feats, weight, bias, 0.5, 200, 3)
    b = ops.mc_dropout_votes(feats, weight, bias, 0.5, 200, 3)
    c = ops.mc_dropout_votes(feats, weight, bias, 0.5, 200, 4)
    assert torch.equal(a.sum(dim=1), torch.full((23,), 200, dtype=torch.int32))
    assert torch.equal(a, b)
    assert not torch.equal(a, c)
    # the seed is used mod 2^64
    d = ops.mc_dropout_votes(feats, weight, bias, 0.5, 200, 3 + 2 ** 64)
    assert torch.equal(a, d)


def test_argument_checks():
    feats, weight, bias = int_problem(4, 8, 3)
    with pytest.raises(ValueError):
        ops.mc_dropout_votes(feats, weight, bias, 1.0, 10, 0)
    with pytest.raises(ValueError):
        ops.mc_dropout_votes(feats, weight, bias, 0.5, 0, 0)
    with pytest.raises(ValueError):
        ops.mc_dropout_votes(feats, weight, bias, 0.5, 65536, 0)
    with pytest.raises(ValueError):
        ops.mc_dropout_votes(feats, weight, bias, 0.5, 10, 0, 2 ** 32 - 3)


# -- 5. sharding invariance --------------------------------------------------


def test_row_offset_makes_shards_invariant():
    feats, weight, bias = int_problem(150, 64, 10, seed=6)
    full = ops.mc_dropout_votes(feats, weight, bias, 0.5, 70, 21)
    for a, b in [(0, 64), (64, 150), (37, 101), (149, 150), (1, 150)]:
        part = ops.mc_dropout_votes(
            feats[a:b], weight, bias, 0.5, 70, 21, row_offset=a
        )
        assert torch.equal(part, full[a:b]), (a, b)
    hi = 2 ** 32 - 150
    top = ops.mc_dropout_votes(feats, weight, bias, 0.5, 70, 21, row_offset=hi)
    part = ops.mc_dropout_votes(
        feats[100:], weight, bias, 0.5, 70, 21, row_offset=hi + 100
    )
    assert torch.equal(part, top[100:])


# -- 6. dropout_head ---------------------------------------------------------


def test_dropout_head_detection():
    m = MnistCNN()
    k, p, lin = m.dropout_head()
    assert (k, p) == (5, 0.5)
    assert lin is m.layers[6]
    assert (lin.in_features, lin.out_features) == (1600, 10)
    assert Cifar10CNN().dropout_head() is None
    assert ResNet20().dropout_head() is None
    assert ImdbTransformer().dropout_head() is None


# -- 7. BaseModel vr_mode ----------------------------------------------------


@pytest.fixture(scope="module")
def mnist_case():
    torch.manual_seed(0)
    model = MnistCNN()
    x = torch.randn(256, 1, 28, 28)
    return model, x


def _spy(monkeypatch):
    """Record which VR implementation BaseModel runs."""
    calls = []
    real_fused = BaseModel._variation_ratio_fused
    real_replay = BaseModel._variation_ratio_replay

    def fused(self, *a, **k):
        calls.append("fused")
        return real_fused(self, *a, **k)

    def replay(self, *a, **k):
        calls.append("replay")
        return real_replay(self, *a, **k)

    monkeypatch.setattr(BaseModel, "_variation_ratio_fused", fused)
    monkeypatch.setattr(BaseModel, "_variation_ratio_replay", replay)
    return calls


def test_fused_mode_values_and_determinism(mnist_case, monkeypatch):
    model, x = mnist_case
    calls = _spy(monkeypatch)
    bm = BaseModel(model, None, predict_batch=100, vr_mode="fused", vr_seed=5)
    _, unc, times = bm.get_pred_and_uncertainty(x)
    assert calls == ["fused"]
    vr = unc["VR"]
    assert vr.shape == (256,)
    assert vr.min() >= 0.0 and vr.max() <= 1.0
    k = vr.astype(np.float64) * 200
    assert np.allclose(k, np.round(k), atol=1e-3)
    t = times["VR"]
    assert t[0] == 0.0 and t[1] > 0.0 and t[2] >= 0.0 and t[3] == 0.0
    _, unc2, _ = bm.get_pred_and_uncertainty(x)
    assert np.array_equal(vr, unc2["VR"])
    # batch size does not matter; another seed does (a prefix of the inputs
    # is enough: rows are independent of what else is in the call)
    other_batch = BaseModel(model, None, predict_batch=37, vr_mode="fused", vr_seed=5)
    assert np.array_equal(
        vr[:64], other_batch.get_pred_and_uncertainty(x[:64])[1]["VR"]
    )
    other_seed = BaseModel(model, None, predict_batch=100, vr_mode="fused", vr_seed=6)
    assert not np.array_equal(
        vr[:64], other_seed.get_pred_and_uncertainty(x[:64])[1]["VR"]
    )
    # a shard with row_base reproduces its slice of the full run
    part = bm.get_pred_and_uncertainty(x[100:140], row_base=100)[1]["VR"]
    assert np.array_equal(part, vr[100:140])


def test_mode_selection(monkeypatch):
    torch.manual_seed(0)
    with pytest.raises(ValueError):
        BaseModel(Cifar10CNN(), None, vr_mode="fused")
    with pytest.raises(ValueError):
        BaseModel(MnistCNN(), None, vr_mode="nonsense")

    calls = _spy(monkeypatch)
    imdb = ImdbTransformer()
    tokens = torch.randint(0, 2000, (6, 100))
    bm = BaseModel(imdb, None, predict_batch=6, vr_mode="auto")
    assert "VR" in bm.get_pred_and_uncertainty(tokens)[1]
    assert calls == ["replay"]

    del calls[:]
    x = torch.randn(8, 1, 28, 28)
    assert config.VR_MODE == "replay"
    default = BaseModel(MnistCNN(), None, predict_batch=8)
    assert default.vr_mode == "replay"
    default.get_pred_and_uncertainty(x)
    assert calls == ["replay"]

    del calls[:]
    BaseModel(MnistCNN(), None, predict_batch=8, vr_mode="auto").get_pred_and_uncertainty(x)
    assert calls == ["fused"]

    del calls[:]
    monkeypatch.setattr(config, "VR_MODE", "fused")
    from_config = BaseModel(MnistCNN(), None, predict_batch=8)
    assert from_config.vr_mode == "fused"
    from_config.get_pred_and_uncertainty(x)
    assert calls == ["fused"]


def test_vr_mode_env_override(monkeypatch):
    monkeypatch.delenv("TIP_VR_MODE", raising=False)
    assert config._default_vr_mode() == "replay"
    monkeypatch.setenv("TIP_VR_MODE", "auto")
    assert config._default_vr_mode() == "auto"
    monkeypatch.setattr(config, "VR_MODE", config._default_vr_mode())
    assert BaseModel(MnistCNN(), None).vr_mode == "auto"
    # a bad value is reported where it is used
    monkeypatch.setattr(config, "VR_MODE", "bogus")
    with pytest.raises(ValueError):
        BaseModel(MnistCNN(), None)


def test_fused_agrees_statistically_with_replay(mnist_case):
    """|mean(A - F)| <= 5 * std(A - B) / sqrt(N) for two replay runs A, B and
    one fused run F: the margin is the replay path's own Monte-Carlo noise."""
    model, x = mnist_case
    n = x.shape[0]
    replay = BaseModel(model, None, predict_batch=256, vr_mode="replay")
    torch.manual_seed(1)
    a = replay._variation_ratio(x)[0].astype(np.float64)
    b = replay._variation_ratio(x)[0].astype(np.float64)
    fused = BaseModel(model, None, predict_batch=256, vr_mode="fused", vr_seed=0)
    f = fused._variation_ratio(x)[0].astype(np.float64)
    bound = 5 * np.std(a - b) / math.sqrt(n)
    print(
        f"mean(A-B)={np.mean(a - b):.5f} mean(A-F)={np.mean(a - f):.5f} "
        f"bound={bound:.5f} mean VR={a.mean():.4f}"
    )
    assert np.std(a - b) > 0, "replay VR must carry Monte-Carlo noise here"
    assert abs(np.mean(a - f)) <= bound
