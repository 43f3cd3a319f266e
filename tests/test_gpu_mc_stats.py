"""The statistics variant of mcdropout.hip on the device against the CPU
oracle (``fallback.mc_dropout_stats``: float32 logits, float64 statistics),
and ``BaseModel(vr_mode="fused", mc_quantifiers=...)`` end to end on the GPU.

Tolerances are worst-case float32 bounds, not measured values:
``mean_probs`` (S + C + 8) * 2^-24 absolute, ``mean_entropy``
(S + 2C + 8) * 2^-24 * ln C absolute."""

import math

import numpy as np
import pytest
import torch

from simple_tip_amd import ops
from simple_tip_amd.ops import fallback

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EPS = 2.0 ** -24
SEED = 1234


def prob_tol(S, C):
    return (S + C + 8) * EPS


def entropy_tol(S, C):
    return (S + 2 * C + 8) * EPS * math.log(C)


def dyadic_problem(n, d, c, seed=0):
    """Float32 logits exact in any order (multiples of 1/64), softmax
    unsaturated: the device logits equal the oracle's bit for bit."""
    g = torch.Generator().manual_seed(seed)
    feats = torch.randint(-3, 4, (n, d), generator=g).float()
    weight = torch.randint(-2, 3, (c, d), generator=g).float() / 64
    bias = torch.randint(-3, 4, (c,), generator=g).float() / 8
    return feats, weight, bias


def int_problem(n, d, c, seed=0):
    """Integer-valued head: exact logits with large margins (saturation)."""
    g = torch.Generator().manual_seed(seed)
    feats = torch.randint(-3, 4, (n, d), generator=g).float()
    weight = torch.randint(-2, 3, (c, d), generator=g).float()
    bias = torch.randint(-3, 4, (c,), generator=g).float()
    return feats, weight, bias


def gpu_stats(feats, weight, bias, p, S, seed, row_offset=0):
    votes, mean_probs, mean_entropy = ops.mc_dropout_stats(
        feats.to(DEV), weight.to(DEV), bias.to(DEV), p, S, seed, row_offset
    )
    n, c = feats.shape[0], weight.shape[0]
    assert votes.is_cuda and votes.dtype == torch.int32 and votes.shape == (n, c)
    assert mean_probs.is_cuda and mean_probs.dtype == torch.float32
    assert mean_probs.shape == (n, c)
    assert mean_entropy.is_cuda and mean_entropy.dtype == torch.float32
    assert mean_entropy.shape == (n,)
    return votes.cpu(), mean_probs.cpu(), mean_entropy.cpu()


def gpu_votes(feats, weight, bias, p, S, seed, row_offset=0):
    return ops.mc_dropout_votes(
        feats.to(DEV), weight.to(DEV), bias.to(DEV), p, S, seed, row_offset
    ).cpu()


def check_against_oracle(got, want, S, c):
    """Votes exact; floats finite and inside the float32 bounds. Prints the
    figures before it asserts."""
    votes, mp, me = got
    w_votes, w_mp, w_me = want
    err_p = float((mp.double() - w_mp.double()).abs().max())
    err_h = float((me.double() - w_me.double()).abs().max())
    err_row = float((mp.double().sum(dim=1) - 1).abs().max())
    print(
        f"S={S} C={c}: mean_probs err {err_p:.3e} (tol {prob_tol(S, c):.3e}), "
        f"mean_entropy err {err_h:.3e} (tol {entropy_tol(S, c):.3e}), "
        f"row sum err {err_row:.3e} (tol {prob_tol(S, c) * c:.3e})"
    )
    assert bool(torch.isfinite(mp).all()) and bool(torch.isfinite(me).all())
    assert torch.equal(votes, w_votes)
    assert err_p <= prob_tol(S, c)
    assert err_h <= entropy_tol(S, c)
    assert err_row <= prob_tol(S, c) * c


def _multi_pass_rows():
    """N* for (D, C) = (64, 10): three passes of the grid-stride row loop,
    the last one partial."""
    from simple_tip_amd.ops import hip_ops

    cfg = hip_ops.mc_dropout_launch_config(64, 10)
    rpp = cfg["rows_per_pass"]
    n = 2 * rpp + rpp // 3 + 5
    assert 2 * rpp < n < 3 * rpp
    return n


CASES = [
    # (N, D, C, S, p); N None -> from the launch constants
    (3, 7, 2, 1, 0.5),             # one sample, 63 idle lanes, C below 4
    (37, 193, 10, 200, 0.5),       # partial chunk, D % 64 != 0, CP = 12
    (37, 193, 10, 200, 0.1),
    (37, 193, 10, 200, 0.9),
    (5, 2048, 16, 257, 0.5),       # last chunk holds one sample; full envelope
    (None, 64, 10, 70, 0.5),       # grid-stride row loop, three passes
]


@pytest.mark.parametrize("n,d,c,S,p", CASES)
def test_against_oracle_on_dyadic_data(n, d, c, S, p):
    if n is None:
        n = _multi_pass_rows()
    feats, weight, bias = dyadic_problem(n, d, c, seed=d + c)
    want = fallback.mc_dropout_stats(feats, weight, bias, p, S, SEED)
    got = gpu_stats(feats, weight, bias, p, S, SEED)
    assert torch.equal(got[0], gpu_votes(feats, weight, bias, p, S, SEED))
    assert torch.equal(got[0].sum(dim=1), torch.full((n,), S, dtype=torch.int32))
    check_against_oracle(got, want, S, c)


def test_saturated_logits():
    """Integer head: margins of tens to hundreds, exponentials underflow."""
    n, d, c, S, p = 19, 50, 7, 33, 0.5
    feats, weight, bias = int_problem(n, d, c, seed=1)
    want = fallback.mc_dropout_stats(feats, weight, bias, p, S, SEED)
    got = gpu_stats(feats, weight, bias, p, S, SEED)
    assert torch.equal(got[0], gpu_votes(feats, weight, bias, p, S, SEED))
    check_against_oracle(got, want, S, c)
    # where every sample of a row is decided by more than 20, the mean
    # softmax is the vote histogram (the other classes hold < 6 e^-20)
    keep = fallback.dropout_keep_mask(SEED, S, n, d, p)
    logits = (
        fallback.dropout_scale(p)
        * torch.matmul(keep.float() * feats[None], weight.t())
        + bias
    )  # exact integers

    def check_histogram(stats, scale):
        top2 = torch.topk(scale * logits, 2, dim=2).values
        decided = ((top2[..., 0] - top2[..., 1]) > 20).all(dim=0)  # [n]
        print(f"head x{scale}: {int(decided.sum())} of {n} rows decided by "
              "> 20 in every sample")
        err = (stats[1] - stats[0].float() / S).abs()[decided]
        if err.numel():
            assert float(err.max()) <= prob_tol(S, c)
        return int(decided.sum())

    check_histogram(got, 1)
    # the same head scaled by 50: every margin that is not an exact tie is at
    # least 50, most exponentials underflow; still finite, still inside the
    # bounds, and most rows are pure vote histograms
    big = gpu_stats(feats, 50 * weight, 50 * bias, p, S, SEED)
    big_want = fallback.mc_dropout_stats(feats, 50 * weight, 50 * bias, p, S, SEED)
    assert torch.equal(big[0], got[0])
    check_against_oracle(big, big_want, S, c)
    assert check_histogram(big, 50) >= n // 2


def test_reproducible_and_batch_invariant_bitwise():
    n, d, c, S, p, seed = 150, 64, 10, 70, 0.5, 21
    feats, weight, bias = dyadic_problem(n, d, c, seed=6)
    full = gpu_stats(feats, weight, bias, p, S, seed)
    again = gpu_stats(feats, weight, bias, p, S, seed)
    for a, b in zip(full, again):
        assert torch.equal(a, b)
    check_against_oracle(
        full, fallback.mc_dropout_stats(feats, weight, bias, p, S, seed), S, c
    )
    for lo, hi in [(0, 64), (64, 150), (37, 101), (149, 150)]:
        part = gpu_stats(feats[lo:hi], weight, bias, p, S, seed, row_offset=lo)
        for got, want in zip(part, full):
            assert torch.equal(got, want[lo:hi]), (lo, hi)
    other = gpu_stats(feats, weight, bias, p, S, seed + 1)
    assert not torch.equal(other[1], full[1])
    assert not torch.equal(other[2], full[2])
    # row ids up to 2^32 - 1
    top_off = 2 ** 32 - n
    top = gpu_stats(feats, weight, bias, p, S, seed, row_offset=top_off)
    check_against_oracle(
        top,
        fallback.mc_dropout_stats(feats, weight, bias, p, S, seed, top_off),
        S, c,
    )
    part = gpu_stats(feats[100:], weight, bias, p, S, seed, row_offset=top_off + 100)
    for got, want in zip(part, top):
        assert torch.equal(got, want[100:])
    with pytest.raises(ValueError):
        gpu_stats(feats, weight, bias, p, S, seed, row_offset=top_off + 1)
    # empty input: no launch, empty tensors
    votes, mp, me = gpu_stats(feats[:0], weight, bias, p, 5, 0)
    assert votes.shape == (0, c) and mp.shape == (0, c) and me.shape == (0,)


@pytest.mark.parametrize("c,d", [(17, 64), (10, 2049)])
def test_outside_envelope_raises(c, d):
    feats, weight, bias = dyadic_problem(4, d, c)
    with pytest.raises(ValueError, match="16.*2048"):
        ops.mc_dropout_stats(
            feats.to(DEV), weight.to(DEV), bias.to(DEV), 0.5, 10, 0
        )


def test_base_model_fused_extras_end_to_end():
    from simple_tip_amd.engine.model_handler import BaseModel
    from simple_tip_amd.models import MnistCNN

    S, c = 200, 10
    tol = entropy_tol(S, c)
    torch.manual_seed(0)
    model = MnistCNN().to(DEV)
    x = torch.randn(300, 1, 28, 28)
    keys = ("VR", "PE", "MI", "MS")
    bm = BaseModel(model, None, predict_batch=30, vr_mode="fused", vr_seed=3,
                   mc_quantifiers=keys)
    _, unc, times = bm.get_pred_and_uncertainty(x)
    for key in keys:
        assert unc[key].shape == (300,) and unc[key].dtype == np.float32
        assert np.isfinite(unc[key]).all()
        assert len(times[key]) == 4 and times[key][1] > 0.0
    vr_only = BaseModel(model, None, predict_batch=30, vr_mode="fused", vr_seed=3)
    _, unc_vr, _ = vr_only.get_pred_and_uncertainty(x)
    assert "PE" not in unc_vr
    assert np.array_equal(unc["VR"], unc_vr["VR"])
    _, unc2, _ = bm.get_pred_and_uncertainty(x)
    for key in keys:
        assert np.array_equal(unc[key], unc2[key]), key
    pe, mi = unc["PE"], unc["MI"]
    print(f"PE [{pe.min():.4f}, {pe.max():.4f}] MI [{mi.min():.3e}, {mi.max():.4f}]")
    assert pe.min() >= 0.0 and pe.max() <= math.log(c) + tol
    assert mi.min() >= -tol
    assert (mi <= pe + tol).all()
    assert pe.std() > 0
    assert unc["MS"].min() >= -1.0 and unc["MS"].max() <= -1.0 / c + prob_tol(S, c)
