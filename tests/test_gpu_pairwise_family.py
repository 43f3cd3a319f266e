"""Exact invariants between the members of the pairwise kernel family
(ops/hip/pairwise.hip), checked on the compiled extension itself.

The flat, grouped, bf16 and plan-driven kernels share one tile core, one
half-merge and one fold per reduction; these tests pin what that sharing
promises as bit equalities:

  C1  flat rowmin is the reduction of the flat full distance matrix
  C2  grouped fp32 equals the per-class flat call, rowmin and KDE
  C3  the gathered (plan) bf16 path equals the padded bf16 path on the same
      rows and norms, rowmin and KDE

All of them hold on the commit before the kernels were folded together
(profiles/r07_pairwise_refactor.md has that run).
"""

import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FLT_MAX = float(np.finfo(np.float32).max)

TRAIN_ROWS = [130, 60, 0]  # class 2 has no train columns: jcount == 0
TEST_ROWS = [129, 5, 3]    # padded segments 256, 128, 128
TSEG = [0, 256, 384, 512]
NSEG = [0, 130, 190, 190]
JB_MAX = 2                 # ceil(130 / 128)


@pytest.fixture(scope="module")
def ext():
    from simple_tip_amd.ops import _load_compiled

    return _load_compiled()


def _rand(m, k, seed):
    x = np.random.RandomState(seed).randn(m, k).astype(np.float32)
    return torch.from_numpy(x).cuda()


def _i32(values):
    return torch.tensor(values, dtype=torch.int32, device="cuda")


# ---- C1 -------------------------------------------------------------------


@pytest.mark.parametrize("m,n,k", [(130, 200, 37), (5, 60, 64), (129, 257, 32)])
def test_flat_rowmin_is_reduction_of_flat_full(ext, m, n, k):
    a, b = _rand(m, k, 11), _rand(n, k, 12)
    full = ext.pairwise_sqdist(a, b)
    dist, idx = ext.rowmin_l2(a, b)
    rowmin = full.min(dim=1).values
    # lowest index among the columns that attain the row minimum
    cols = torch.arange(n, device="cuda").expand(m, n)
    lowest = torch.where(full == rowmin[:, None], cols, n).min(dim=1).values
    assert torch.equal(idx, lowest)
    assert torch.equal(full[torch.arange(m, device="cuda"), idx], rowmin)
    ulp = (dist.view(torch.int32) - rowmin.sqrt().view(torch.int32)).abs().max()
    print(f"[{m}x{n}x{k}] rowmin dist vs sqrt(full.min): max {int(ulp)} ulp")
    assert torch.equal(dist, rowmin.sqrt())


# ---- C2 -------------------------------------------------------------------


def _grouped_inputs(k, scale):
    """Class-sorted train rows, per-class test rows and the zero-padded,
    class-sorted test matrix."""
    train = _rand(sum(TRAIN_ROWS), k, 21) * scale
    tests = [_rand(r, k, 30 + c) * scale for c, r in enumerate(TEST_ROWS)]
    padded = torch.zeros(TSEG[-1], k, device="cuda")
    for c, rows in enumerate(tests):
        padded[TSEG[c]:TSEG[c] + rows.shape[0]] = rows
    return train, tests, padded


def test_grouped_rowmin_equals_per_class_flat(ext):
    train, tests, padded = _grouped_inputs(37, 1.0)
    dist, idx = ext.grouped_rowmin(
        padded, train, _i32(TSEG), _i32(NSEG), ext.rownorm(train), JB_MAX
    )
    for c, rows in enumerate(tests):
        got = slice(TSEG[c], TSEG[c] + rows.shape[0])
        if TRAIN_ROWS[c] == 0:
            assert bool((idx[got] == -1).all())
            continue
        d_flat, i_flat = ext.rowmin_l2(rows, train[NSEG[c]:NSEG[c + 1]].contiguous())
        assert torch.equal(dist[got], d_flat)
        assert torch.equal(idx[got], i_flat + NSEG[c])


def test_grouped_kde_equals_per_class_flat(ext):
    # scaled as in test_gpu_ops.py so the sums do not underflow
    train, tests, padded = _grouped_inputs(37, 0.3)
    lse = ext.grouped_kde(
        padded, train, _i32(TSEG), _i32(NSEG), ext.rownorm(train), JB_MAX
    )
    for c, rows in enumerate(tests):
        got = slice(TSEG[c], TSEG[c] + rows.shape[0])
        if TRAIN_ROWS[c] == 0:
            # the fold over no partials: empty sum, reported as -FLT_MAX
            assert bool((lse[got] == -FLT_MAX).all())
            continue
        flat = ext.kde_logsumexp(rows, train[NSEG[c]:NSEG[c + 1]].contiguous())
        assert bool(torch.isfinite(flat).all()) and bool((flat > -FLT_MAX).all())
        assert torch.equal(lse[got], flat)


# ---- C3 -------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def _plan_case():
    """Shuffled bf16 source rows of the C2 class layout at K = 40 (a multiple
    of 8, not of 32: the last k step is a tail), their plan and norms."""
    from simple_tip_amd.ops import _load_compiled

    ext = _load_compiled()
    k, c = 40, len(TEST_ROWS)
    b = sum(TEST_ROWS)
    rng = np.random.RandomState(41)
    pred = torch.from_numpy(rng.permutation(np.repeat(np.arange(c), TEST_ROWS))).cuda()
    src = (_rand(b, k, 42) * 0.3).to(torch.bfloat16)
    train = (_rand(sum(TRAIN_ROWS), k, 43) * 0.3).to(torch.bfloat16)
    tseg, rowmap, dest = ext.segment_plan(pred, c)
    assert tseg.tolist() == TSEG
    an = torch.empty(b, device="cuda")
    ext.rownorm_bf16_out(src, an)
    bn = torch.empty(train.shape[0], device="cuda")
    ext.rownorm_bf16_out(train, bn)
    bp = ext.segment_plan_rows(b, c)
    return dict(ext=ext, k=k, b=b, bp=bp, pred=pred, src=src, train=train,
                tseg=tseg, rowmap=rowmap, dest=dest.long(), an=an, bn=bn,
                nseg=_i32(NSEG))


def _nan(*shape):
    return torch.full(shape, float("nan"), device="cuda")


def test_plan_rowmin_equals_padded_bf16():
    p = _plan_case()
    ext, b, bp, dest = p["ext"], p["b"], p["bp"], p["dest"]
    rows = TSEG[-1]
    padded = torch.zeros(rows, p["k"], device="cuda", dtype=torch.bfloat16)
    padded[dest] = p["src"]
    an_p = torch.zeros(rows, device="cuda")
    an_p[dest] = p["an"]
    dist_p, idx_p = ext.grouped_rowmin_bf16(
        padded, p["train"], p["tseg"], p["nseg"], an_p, p["bn"], JB_MAX
    )

    btable = torch.from_numpy(
        np.random.RandomState(44).rand(sum(TRAIN_ROWS)).astype(np.float32) + 0.5
    ).cuda()
    pval = _nan(JB_MAX, bp)
    pidx = torch.full((JB_MAX, bp), -1, dtype=torch.int32, device="cuda")
    dsa, dist = _nan(b), _nan(b)
    idx = torch.full((b,), -7, dtype=torch.int32, device="cuda")
    ext.grouped_rowmin_plan(
        p["src"], p["train"], p["tseg"], p["nseg"], p["rowmap"], p["an"],
        p["bn"], btable, JB_MAX, pval, pidx, dsa, dist, idx,
    )
    assert torch.equal(dist, dist_p[dest])
    assert torch.equal(idx.long(), idx_p[dest])
    has_train = idx >= 0
    assert torch.equal(has_train, p["pred"] != 2)
    assert torch.equal(dsa[has_train],
                       dist[has_train] / btable[idx[has_train].long()])
    # a class without train columns: the final kernel reports +inf
    assert bool((dsa[~has_train] == float("inf")).all())


def test_plan_kde_equals_padded_bf16():
    p = _plan_case()
    ext, b, bp, dest = p["ext"], p["b"], p["bp"], p["dest"]
    c = len(TEST_ROWS)
    # `white` is the whitened workspace in padded layout; here simply the
    # source rows scattered through the plan
    white = torch.zeros(bp, p["k"], device="cuda", dtype=torch.bfloat16)
    white[dest] = p["src"]
    wan = torch.empty(bp, device="cuda")
    ext.rownorm_bf16_out(white, wan)
    lse_p = ext.grouped_kde_bf16(
        white, p["train"], p["tseg"], p["nseg"], wan, p["bn"], JB_MAX
    )

    pkde = _nan(JB_MAX, bp, 2)
    lsa = _nan(b)
    ext.grouped_kde_plan(
        white, p["train"], p["tseg"], p["nseg"], p["rowmap"], wan, p["bn"],
        torch.ones(c, dtype=torch.int32, device="cuda"),
        torch.zeros(c, device="cuda"), JB_MAX, pkde, lsa,
    )
    assert bool(torch.isfinite(lsa).all())
    assert torch.equal(lsa, -lse_p[dest])
