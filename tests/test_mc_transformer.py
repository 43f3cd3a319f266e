"""Fused MC-dropout sampling of the IMDB transformer's stochastic tail: the
CPU implementation (ops.fallback.mc_transformer_*), the model's
``dropout_tail()`` and BaseModel's ``vr_mode="fused"`` on that model."""

import math

import numpy as np
import pytest
import torch

from simple_tip_amd import ops
from simple_tip_amd.engine.model_handler import BaseModel
from simple_tip_amd.models import Cifar10CNN, ImdbTransformer, MnistCNN, ResNet20
from simple_tip_amd.models.base import DropoutTail
from simple_tip_amd.ops import fallback

EPS = 2.0 ** -24  # half a float32 ulp at 1
S = 200


def prob_tol(s, c):
    return (s + c + 8) * EPS


@pytest.fixture(scope="module")
def imdb_case():
    """Model, 256 token rows and the tail's deterministic inputs."""
    torch.manual_seed(0)
    model = ImdbTransformer().eval()
    tokens = torch.randint(0, 2000, (256, 100))
    tail = model.dropout_tail()
    with torch.no_grad():
        emb = tail.embed(tokens)
        attn = tail.att(emb, emb, emb, need_weights=False)[0]
    return model, tokens, tail, emb, attn


# -- 1. masks ----------------------------------------------------------------


def test_site_masks_are_slices_of_one_element_axis():
    seed, s, n, t, e, h, p, off = 9, 5, 3, 7, 32, 20, 0.3, 11
    dtot = 2 * t * e + e + h
    flat = fallback.dropout_keep_mask(seed, s, n, dtot, p, row_offset=off)
    k1, k2, k3, k4 = fallback.mc_transformer_masks(
        seed, s, n, t, e, h, (p, p, p, p), row_offset=off
    )
    assert k1.shape == (s, n, t, e) and k2.shape == (s, n, t, e)
    assert k3.shape == (s, n, e) and k4.shape == (s, n, h)
    assert torch.equal(k1.reshape(s, n, -1), flat[:, :, : t * e])
    assert torch.equal(k2.reshape(s, n, -1), flat[:, :, t * e : 2 * t * e])
    assert torch.equal(k3, flat[:, :, 2 * t * e : 2 * t * e + e])
    assert torch.equal(k4, flat[:, :, 2 * t * e + e :])
    # element (t, e) of site 1 sits at t*E + e
    assert bool(k1[2, 1, 4, 9]) == bool(flat[2, 1, 4 * e + 9])
    # each site uses its own rate; p = 0 keeps everything
    m1, m2, m3, m4 = fallback.mc_transformer_masks(
        seed, s, n, t, e, h, (0.0, p, 0.9, 0.0), row_offset=off
    )
    assert bool(m1.all()) and bool(m4.all())
    assert torch.equal(m2, k2)
    assert float(m3.float().mean()) < float(k3.float().mean())


# -- 2. the op on the CPU ----------------------------------------------------


def test_p_zero_is_the_deterministic_model(imdb_case):
    model, tokens, tail, emb, attn = imdb_case
    n = 16
    with torch.no_grad():
        logits = model(tokens[:n])
    votes, mean_probs, mean_entropy = ops.mc_transformer_stats(
        emb[:n], attn[:n], tail.params, (0.0, 0.0, 0.0, 0.0), S, 4
    )
    assert votes.dtype == torch.int32 and votes.shape == (n, 2)
    assert mean_probs.dtype == torch.float32 and mean_probs.shape == (n, 2)
    assert mean_entropy.dtype == torch.float32 and mean_entropy.shape == (n,)
    want = torch.zeros(n, 2, dtype=torch.int32)
    want[torch.arange(n), logits.argmax(dim=1)] = S
    assert torch.equal(votes, want)
    err = float((mean_probs - torch.softmax(logits, dim=1)).abs().max())
    print(f"mean_probs vs eval softmax: {err:.3e} (tol {prob_tol(S, 2):.3e})")
    assert err <= prob_tol(S, 2)
    assert torch.equal(
        votes,
        ops.mc_transformer_votes(
            emb[:n], attn[:n], tail.params, (0.0, 0.0, 0.0, 0.0), S, 4
        ),
    )


def test_row_offset_slices_equal_the_full_call(imdb_case, monkeypatch):
    _, _, tail, emb, attn = imdb_case
    n, s, seed = 12, 33, 21
    x, a = emb[:n], attn[:n]
    full = ops.mc_transformer_stats(x, a, tail.params, tail.rates, s, seed)
    assert torch.equal(full[0].sum(dim=1), torch.full((n,), s, dtype=torch.int32))
    assert torch.equal(
        full[0], ops.mc_transformer_votes(x, a, tail.params, tail.rates, s, seed)
    )
    for lo, hi in [(0, 5), (5, 12), (3, 4), (11, 12)]:
        part = ops.mc_transformer_stats(
            x[lo:hi], a[lo:hi], tail.params, tail.rates, s, seed, row_offset=lo
        )
        for got, want in zip(part, full):
            assert torch.equal(got, want[lo:hi]), (lo, hi)
    # the row chunking of the implementation is invisible
    monkeypatch.setattr(fallback, "_MCD_MAX_MASK_ELEMS", 3 * s * 6452)
    chunked = ops.mc_transformer_stats(x, a, tail.params, tail.rates, s, seed)
    for got, want in zip(chunked, full):
        assert torch.equal(got, want)
    monkeypatch.undo()
    # the last admissible offset, one past it, and N = 0
    top = 2 ** 32 - 2
    hi = ops.mc_transformer_votes(
        x[:2], a[:2], tail.params, tail.rates, s, seed, row_offset=top
    )
    assert torch.equal(hi.sum(dim=1), torch.full((2,), s, dtype=torch.int32))
    last = ops.mc_transformer_votes(
        x[1:2], a[1:2], tail.params, tail.rates, s, seed, row_offset=top + 1
    )
    assert torch.equal(last, hi[1:2])
    with pytest.raises(ValueError):
        ops.mc_transformer_votes(
            x[:2], a[:2], tail.params, tail.rates, s, seed, row_offset=top + 1
        )
    votes, mp, me = ops.mc_transformer_stats(
        x[:0], a[:0], tail.params, tail.rates, s, seed
    )
    assert votes.shape == (0, 2) and mp.shape == (0, 2) and me.shape == (0,)


def test_argument_errors(imdb_case):
    _, _, tail, emb, attn = imdb_case
    x, a, q, p = emb[:2], attn[:2], tail.params, tail.rates
    for bad_s in (0, 65536):
        with pytest.raises(ValueError):
            ops.mc_transformer_votes(x, a, q, p, bad_s, 0)
    with pytest.raises(ValueError):
        ops.mc_transformer_votes(x, a, q, p, 5, 0, row_offset=-1)
    for bad_p in ((0.1, 0.1, 0.1), (0.1, 0.1, 1.0, 0.1), (-0.1, 0, 0, 0)):
        with pytest.raises(ValueError):
            ops.mc_transformer_votes(x, a, q, bad_p, 5, 0)
    with pytest.raises(ValueError):
        ops.mc_transformer_votes(x, a[:, :50], q, p, 5, 0)
    with pytest.raises(ValueError):
        ops.mc_transformer_votes(x, a, q._replace(b3=q.b3[:5]), p, 5, 0)
    assert ops.mc_transformer_supported(x, 16, 500, 99, 99, 9)  # CPU: no envelope


# -- 3. the model ------------------------------------------------------------


def test_dropout_tail_structure():
    m = ImdbTransformer()
    tail = m.dropout_tail()
    assert isinstance(tail, DropoutTail)
    blk = m.layers[2]
    assert tail.embed is m.layers[1] and tail.att is blk.att
    assert tail.rates == (0.1, 0.1, 0.1, 0.1)
    q = tail.params
    assert isinstance(q, ops.McTransformerParams)
    assert q.w1 is blk.ffn[0].weight and q.w2 is blk.ffn[2].weight
    assert q.ln1_w is blk.layernorm1.weight and q.ln2_b is blk.layernorm2.bias
    assert q.w3 is m.layers[5][0].weight and q.w4 is m.layers[7].weight
    assert tuple(q.w1.shape) == (32, 32) and tuple(q.w2.shape) == (32, 32)
    assert tuple(q.w3.shape) == (20, 32) and tuple(q.w4.shape) == (2, 20)
    assert q.eps == 1e-6
    assert m.dropout_head() is None
    for other in (MnistCNN(), Cifar10CNN(), ResNet20()):
        assert other.dropout_tail() is None
    # any other layer list is not a tail
    extra = ImdbTransformer()
    extra.layers.append(torch.nn.Dropout(0.5))
    assert extra.dropout_tail() is None
    noisy = ImdbTransformer()
    noisy.layers[2].att.dropout = 0.1
    assert noisy.dropout_tail() is None


# -- 4. BaseModel ------------------------------------------------------------


def test_fused_mode_constructs_and_samples(imdb_case):
    model, tokens, _, _, _ = imdb_case
    x = tokens[:48]
    bm = BaseModel(model, None, predict_batch=20, vr_mode="fused", vr_seed=3)
    _, unc, times = bm.get_pred_and_uncertainty(x)
    vr = unc["VR"]
    assert vr.shape == (48,) and vr.dtype == np.float32
    assert vr.min() >= 0.0 and vr.max() <= 1.0
    k = vr.astype(np.float64) * S
    assert np.allclose(k, np.round(k), atol=1e-3)
    assert vr.std() > 0
    t = times["VR"]
    assert t[0] == 0.0 and t[1] > 0.0 and t[2] >= 0.0 and t[3] == 0.0
    # repeat runs, other batching, shards with row_base; another seed differs
    assert np.array_equal(vr, bm.get_pred_and_uncertainty(x)[1]["VR"])
    part = bm.get_pred_and_uncertainty(x[20:31], row_base=20)[1]["VR"]
    assert np.array_equal(part, vr[20:31])
    other = BaseModel(model, None, predict_batch=20, vr_mode="fused", vr_seed=4)
    assert not np.array_equal(vr, other.get_pred_and_uncertainty(x)[1]["VR"])
    # "auto" stays on replay for this model; the model is left in eval mode
    assert BaseModel(model, None, vr_mode="auto")._fused_vr_head() is None
    assert not any(m.training for m in model.modules())


def test_fused_extras(imdb_case):
    model, tokens, _, _, _ = imdb_case
    x = tokens[:48]
    keys = ("VR", "PE", "MI", "MS")
    c = 2
    tol = (S + 2 * c + 8) * EPS * math.log(c)
    bm = BaseModel(model, None, predict_batch=20, vr_mode="fused", vr_seed=3,
                   mc_quantifiers=keys)
    _, unc, times = bm.get_pred_and_uncertainty(x)
    for key in keys:
        assert unc[key].shape == (48,) and unc[key].dtype == np.float32
        assert np.isfinite(unc[key]).all()
        assert len(times[key]) == 4 and times[key][1] > 0.0
    vr_only = BaseModel(model, None, predict_batch=20, vr_mode="fused", vr_seed=3)
    unc_vr = vr_only.get_pred_and_uncertainty(x)[1]
    assert "PE" not in unc_vr
    assert np.array_equal(unc["VR"], unc_vr["VR"])
    pe, mi = unc["PE"], unc["MI"]
    assert pe.min() >= 0.0 and pe.max() <= math.log(c) + tol
    assert mi.min() >= -tol
    assert (mi <= pe + tol).all()
    assert pe.std() > 0
    assert unc["MS"].min() >= -1.0 and unc["MS"].max() <= -1.0 / c + prob_tol(S, c)


def test_fused_agrees_statistically_with_replay(imdb_case):
    """|mean(A - F)| <= 5 * std(A - B) / sqrt(N) for two replay runs A, B and
    one fused run F: the margin is the replay path's own Monte-Carlo noise."""
    model, tokens, _, _, _ = imdb_case
    n = tokens.shape[0]
    replay = BaseModel(model, None, predict_batch=256, vr_mode="replay")
    torch.manual_seed(1)
    a = replay._variation_ratio(tokens)[0].astype(np.float64)
    b = replay._variation_ratio(tokens)[0].astype(np.float64)
    fused = BaseModel(model, None, predict_batch=256, vr_mode="fused", vr_seed=0)
    f = fused._variation_ratio(tokens)[0].astype(np.float64)
    bound = 5 * np.std(a - b) / math.sqrt(n)
    print(
        f"mean(A-B)={np.mean(a - b):.5f} mean(A-F)={np.mean(a - f):.5f} "
        f"bound={bound:.5f} mean VR={a.mean():.4f}"
    )
    assert np.std(a - b) > 0, "replay VR must carry Monte-Carlo noise here"
    assert abs(np.mean(a - f)) <= bound
