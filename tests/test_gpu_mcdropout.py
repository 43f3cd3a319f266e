"""mcdropout.hip on the device against the CPU oracle
(``fallback.mc_dropout_votes``), and ``BaseModel(vr_mode="fused")`` end to
end on the GPU."""

import numpy as np
import pytest
import torch

from simple_tip_amd import ops
from simple_tip_amd.ops import fallback

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def int_problem(n, d, c, seed=0):
    """Integer-valued head: every partial sum is exact in float32, so the
    device votes must equal the oracle's bit for bit (ties included)."""
    g = torch.Generator().manual_seed(seed)
    feats = torch.randint(-3, 4, (n, d), generator=g).float()
    weight = torch.randint(-2, 3, (c, d), generator=g).float()
    bias = torch.randint(-3, 4, (c,), generator=g).float()
    return feats, weight, bias


def gpu_votes(feats, weight, bias, p, S, seed, row_offset=0):
    out = ops.mc_dropout_votes(
        feats.to(DEV), weight.to(DEV), bias.to(DEV), p, S, seed, row_offset
    )
    assert out.is_cuda and out.dtype == torch.int32
    return out.cpu()


def _multi_pass_rows():
    """N* for (D, C) = (64, 10): three passes of the grid-stride row loop,
    the last one partial (a third of a pass plus an odd remainder)."""
    from simple_tip_amd.ops import hip_ops

    cfg = hip_ops.mc_dropout_launch_config(64, 10)
    rpp = cfg["rows_per_pass"]
    assert rpp == cfg["rows_per_block"] * cfg["max_grid"]
    n = 2 * rpp + rpp // 3 + 5
    assert 2 * rpp < n < 3 * rpp
    return n


EXACT_CASES = [
    # (N, D, C, S, p); N None -> from the launch constants
    (3, 7, 2, 1, 0.5),
    (37, 193, 10, 200, 0.5),
    (37, 193, 10, 200, 0.1),
    (37, 193, 10, 200, 0.9),
    (5, 2048, 16, 257, 0.5),
    (130, 1600, 10, 200, 0.5),
    (None, 64, 10, 70, 0.5),
]


@pytest.mark.parametrize("n,d,c,S,p", EXACT_CASES)
def test_exact_on_integer_data(n, d, c, S, p):
    if n is None:
        n = _multi_pass_rows()
    feats, weight, bias = int_problem(n, d, c, seed=d + c)
    want = fallback.mc_dropout_votes(feats, weight, bias, p, S, 1234)
    got = gpu_votes(feats, weight, bias, p, S, 1234)
    assert got.shape == (n, c)
    assert torch.equal(got.sum(dim=1), torch.full((n,), S, dtype=torch.int32))
    assert torch.equal(got, want)


def test_edge_cases_on_device():
    feats, weight, bias = int_problem(19, 50, 7, seed=1)
    # p = 0: every vote on the deterministic argmax
    votes = gpu_votes(feats, weight, bias, 0.0, 33, 9)
    logits = (feats @ weight.t() + bias).numpy()
    want = np.zeros((19, 7), dtype=np.int32)
    want[np.arange(19), np.argmax(logits, axis=1)] = 33
    assert torch.equal(votes, torch.from_numpy(want))
    # all-zero row -> argmax(bias), lowest index on the tie
    feats[2] = 0
    tie_bias = torch.tensor([-1.0, 2.0, 0.5, 2.0, -3.0, 2.0, 0.0])
    votes = gpu_votes(feats, weight, tie_bias, 0.5, 50, 1)
    assert votes[2].tolist() == [0, 50, 0, 0, 0, 0, 0]
    # zero head -> class 0
    zero = gpu_votes(feats, torch.zeros_like(weight), torch.zeros(7), 0.5, 50, 1)
    assert torch.equal(zero[:, 0], torch.full((19,), 50, dtype=torch.int32))
    assert int(zero[:, 1:].sum()) == 0
    # S = 1, row sums, determinism, seeds
    one = gpu_votes(feats, weight, bias, 0.5, 1, 3)
    assert torch.equal(one.sum(dim=1), torch.ones(19, dtype=torch.int32))
    assert torch.equal(one, fallback.mc_dropout_votes(feats, weight, bias, 0.5, 1, 3))
    a = gpu_votes(feats, weight, bias, 0.5, 200, 3)
    b = gpu_votes(feats, weight, bias, 0.5, 200, 3)
    c = gpu_votes(feats, weight, bias, 0.5, 200, 4)
    assert torch.equal(a.sum(dim=1), torch.full((19,), 200, dtype=torch.int32))
    assert torch.equal(a, b)
    assert not torch.equal(a, c)
    # negative features are not assumed away; 64-bit seeds use both halves
    big = (5 << 32) | 7
    assert torch.equal(
        gpu_votes(-feats.abs(), weight, bias, 0.5, 70, big),
        fallback.mc_dropout_votes(-feats.abs(), weight, bias, 0.5, 70, big),
    )
    # empty input
    assert gpu_votes(feats[:0], weight, bias, 0.5, 5, 0).shape == (0, 7)


def test_row_offset_invariance_on_device():
    feats, weight, bias = int_problem(150, 64, 10, seed=6)
    full = gpu_votes(feats, weight, bias, 0.5, 70, 21)
    assert torch.equal(full, fallback.mc_dropout_votes(feats, weight, bias, 0.5, 70, 21))
    for a, b in [(0, 64), (64, 150), (37, 101), (149, 150)]:
        part = gpu_votes(feats[a:b], weight, bias, 0.5, 70, 21, row_offset=a)
        assert torch.equal(part, full[a:b]), (a, b)
    hi = 2 ** 32 - 150
    top = gpu_votes(feats, weight, bias, 0.5, 70, 21, row_offset=hi)
    assert torch.equal(
        top, fallback.mc_dropout_votes(feats, weight, bias, 0.5, 70, 21, hi)
    )
    part = gpu_votes(feats[100:], weight, bias, 0.5, 70, 21, row_offset=hi + 100)
    assert torch.equal(part, top[100:])
    with pytest.raises(ValueError):
        gpu_votes(feats, weight, bias, 0.5, 70, 21, row_offset=hi + 1)


def test_real_valued_data_against_float64_oracle():
    """A device vote may differ from the float64 oracle only where the
    oracle's own top-2 margin is below 1e-4 * max|logit|."""
    n, d, c, S, p, seed = 64, 1600, 10, 200, 0.5, 77
    g = torch.Generator().manual_seed(5)
    feats = torch.relu(torch.randn(n, d, generator=g))
    weight = torch.randn(c, d, generator=g) / d ** 0.5
    bias = 0.1 * torch.randn(c, generator=g)

    keep = fallback.dropout_keep_mask(seed, S, n, d, p)
    scale = fallback.dropout_scale(p)
    logits = (
        scale * torch.matmul(keep.double() * feats.double()[None], weight.double().t())
        + bias.double()
    )  # [S, n, c] float64
    top2 = torch.topk(logits, 2, dim=2).values
    margin = top2[..., 0] - top2[..., 1]
    near_tie = margin < 1e-4 * float(logits.abs().max())
    frac = float(near_tie.double().mean())
    print(f"near-tie (s, n) pairs: {100 * frac:.3f}%")
    assert frac <= 0.002
    best = logits.argmax(dim=2)  # [S, n]

    got = gpu_votes(feats, weight, bias, p, S, seed)
    # votes of the pairs that are not near ties are fixed by the oracle; the
    # near-tie pairs of a row may land anywhere
    sure = torch.zeros(n, c, dtype=torch.int32)
    sure.scatter_add_(
        1, best.t().contiguous(), (~near_tie).t().to(torch.int32).contiguous()
    )
    free = near_tie.sum(dim=0).to(torch.int32)  # [n]
    assert torch.equal(got.sum(dim=1), torch.full((n,), S, dtype=torch.int32))
    assert bool((got >= sure).all())
    assert torch.equal((got - sure).sum(dim=1), free)
    # a near-tie vote can only go to one of that pair's top-2 classes
    top2_idx = torch.topk(logits, 2, dim=2).indices  # [S, n, 2]
    allowed = torch.zeros(n, c, dtype=torch.int32)
    for j in range(2):
        allowed.scatter_add_(
            1,
            top2_idx[..., j].t().contiguous(),
            near_tie.t().to(torch.int32).contiguous(),
        )
    assert bool(((got - sure) <= allowed).all())


@pytest.mark.parametrize("c,d", [(17, 64), (10, 2049)])
def test_outside_envelope_raises(c, d):
    feats, weight, bias = int_problem(4, d, c)
    with pytest.raises(ValueError, match="16.*2048"):
        gpu_votes(feats, weight, bias, 0.5, 10, 0)


def test_base_model_fused_end_to_end():
    from simple_tip_amd.engine.model_handler import BaseModel
    from simple_tip_amd.models import MnistCNN

    torch.manual_seed(0)
    model = MnistCNN().to(DEV)
    x = torch.randn(300, 1, 28, 28)
    # ten equal batches: row offsets are in play, one conv shape per dtype
    fused = BaseModel(model, None, predict_batch=30, vr_mode="fused", vr_seed=3)
    pred, unc, times = fused.get_pred_and_uncertainty(x)
    vr = unc["VR"]
    assert vr.shape == (300,) and vr.dtype == np.float32
    assert vr.min() >= 0.0 and vr.max() <= 1.0
    k = vr.astype(np.float64) * 200
    assert np.allclose(k, np.round(k), atol=1e-3)
    assert vr.std() > 0
    t = times["VR"]
    assert t[0] == 0.0 and t[1] > 0.0 and t[2] >= 0.0 and t[3] == 0.0
    _, unc2, _ = fused.get_pred_and_uncertainty(x)
    assert np.array_equal(vr, unc2["VR"])

    # replay in batches of 5: its 5 x 200 macro-batch keeps the conv
    # library's first-use algorithm search (seconds at 30 x 200) short
    replay = BaseModel(model, None, predict_batch=5, vr_mode="replay")
    pred_r, unc_r, times_r = replay.get_pred_and_uncertainty(x)
    assert set(unc) == set(unc_r) and set(times) == set(times_r)
    for key in unc:
        assert unc[key].shape == unc_r[key].shape
        assert unc[key].dtype == unc_r[key].dtype
    assert len(times["VR"]) == len(times_r["VR"]) == 4
    assert pred.shape == pred_r.shape
