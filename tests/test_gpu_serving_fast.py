"""Sync-free grouped scoring path of FusedPrioritizer (device segment plan,
gathered kernels) against the host-planned bf16 path and the fp32 path.

Each case fits once and runs the old bf16 path, the fast path and the fp32
path in one process; the tests below only read those results.

Measured on MI355X (see profiles/r05_sync_free_scoring.md for the figures).
"""

import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CASES = ["uniform", "skewed"]
SINGLETON, UNSEEN, ABSENT = 8, 7, 5  # skewed case class roles


def _inputs(case):
    rng = np.random.RandomState(0 if case == "uniform" else 2)
    ats = torch.from_numpy(rng.randn(3000, 256).astype(np.float32))
    pred = torch.from_numpy(rng.randint(0, 7, 3000))
    rng_t = np.random.RandomState(1 if case == "uniform" else 3)
    test = torch.from_numpy(rng_t.randn(777, 256).astype(np.float32))
    if case == "uniform":
        tp = torch.from_numpy(rng_t.randint(0, 7, 777))
    else:
        pred[0] = SINGLETON  # one training sample: LSA density 0 (const 0.0)
        tp = np.concatenate([np.full(600, 3), rng_t.randint(0, 3, 177)])
        tp[[10, 20, 700]] = SINGLETON
        tp[[11, 21, 701, 776]] = UNSEEN  # no training sample at all: +inf
        assert not (tp == ABSENT).any()
        tp = torch.from_numpy(tp)
    return ats, pred, test, tp


def _old_rowmin(p, ats, pred):
    """(min distance, argmin) per input row from the host-planned bf16 path."""
    order, dest, tseg_cpu, tseg = p._segment(ats, pred)
    padded = torch.zeros(
        int(tseg_cpu[-1]), ats.shape[1], device=ats.device, dtype=torch.bfloat16
    )
    padded[dest] = ats[order].to(torch.bfloat16)
    pf = padded.float()
    an = (pf * pf).sum(dim=1).contiguous()
    dist, idx = p.ext.grouped_rowmin_bf16(
        padded, p.trainS16, tseg, p.nseg, an, p.bnormS16, p.jb_max
    )
    d = torch.empty(ats.shape[0], device=ats.device)
    i = torch.empty(ats.shape[0], device=ats.device, dtype=torch.int64)
    d[order] = dist[dest]
    i[order] = idx[dest]
    return d, i


def _near_ties(p, test, tp):
    """Rows whose nearest and second-nearest squared distance (fp64, on the
    bf16-rounded inputs) differ by less than 1e-5 relative."""
    train = p.trainS16.double().cpu()
    x = test.to(torch.bfloat16).double().cpu()
    offs = p.nseg.cpu().tolist()
    tie = torch.zeros(x.shape[0], dtype=torch.bool)
    for c in range(p.num_classes):
        rows = torch.nonzero(tp.cpu() == c, as_tuple=True)[0]
        seg = train[offs[c]:offs[c + 1]]
        if rows.numel() == 0 or seg.shape[0] < 2:
            continue
        d2 = torch.cdist(x[rows], seg).pow(2)
        two = torch.topk(d2, 2, dim=1, largest=False).values
        tie[rows] = (two[:, 1] - two[:, 0]) < 1e-5 * two[:, 0]
    return tie


@functools.lru_cache(maxsize=None)
def _run(case):
    from simple_tip_amd.core.surprise import DSA, LSA, MultiModalSA
    from simple_tip_amd.engine.serving import FusedPrioritizer

    dev = torch.device("cuda:0")
    ats, pred, test, tp = _inputs(case)
    dsa = DSA(ats, pred, device=dev)
    lsa = MultiModalSA.build_by_class(
        ats, pred, lambda a, p: LSA(a, max_features=64, device=dev)
    )
    old = FusedPrioritizer(dsa, lsa, dev, pairwise_dtype=torch.bfloat16,
                           fast=False)
    fast = FusedPrioritizer(dsa, lsa, dev, pairwise_dtype=torch.bfloat16)
    fp32 = FusedPrioritizer(dsa, lsa, dev)
    assert fast.fast and not old.fast and not fp32.fast
    assert fast.lsa_ready
    test, tp = test.to(dev), tp.to(dev)
    r = {"fast_obj": fast, "old_obj": old, "test": test, "tp": tp}
    r["old"] = old(test, tp)
    r["fast"] = fast(test, tp)
    ws = fast._ws[(777, 256)]
    r["fast_dist"] = ws["dist"].clone()
    r["fast_idx"] = ws["idx"].clone().long()
    r["fp32"] = fp32(test, tp)
    r["old_dist"], r["old_idx"] = _old_rowmin(old, test, tp)
    r["tie"] = _near_ties(old, test, tp).to(dev)
    return r


def _rankcorr(a, b):
    ra = a.float().argsort().argsort().float()
    rb = b.float().argsort().argsort().float()
    ra = (ra - ra.mean()) / ra.std()
    rb = (rb - rb.mean()) / rb.std()
    return float((ra * rb).mean())


@pytest.mark.parametrize("case", CASES)
def test_shapes_and_dtypes(case):
    r = _run(case)
    for got, ref in zip(r["fast"], r["old"]):
        assert got.shape == ref.shape == (777,)
        assert got.dtype == ref.dtype == torch.float32
        assert got.device == ref.device


@pytest.mark.parametrize("case", CASES)
def test_dsa_min_distance(case):
    """Only the norm summation order differs: rtol 1e-4 on every row."""
    r = _run(case)
    err = ((r["fast_dist"] - r["old_dist"]).abs() / r["old_dist"].abs()).max()
    print(f"[{case}] max rel min-distance deviation {float(err):.3e}")
    assert torch.allclose(r["fast_dist"], r["old_dist"], rtol=1e-4, atol=0.0)


@pytest.mark.parametrize("case", CASES)
def test_dsa_score_and_argmin(case):
    r = _run(case)
    tie = r["tie"]
    n_tie = int(tie.sum())
    print(f"[{case}] near-tie rows excluded: {n_tie} of {tie.numel()}")
    assert n_tie <= 0.01 * tie.numel()
    keep = ~tie
    assert torch.equal(r["fast_idx"][keep], r["old_idx"][keep])
    d_fast, d_old = r["fast"][0][keep], r["old"][0][keep]
    fin = torch.isfinite(d_old)
    assert torch.equal(torch.isfinite(d_fast), fin)
    assert torch.equal(d_fast[~fin], d_old[~fin])  # +inf stays +inf
    assert torch.allclose(d_fast[fin], d_old[fin], rtol=1e-4, atol=0.0)


@pytest.mark.parametrize("case", CASES)
def test_lsa_against_fp32(case):
    """The whiten accumulation order differs from hipBLASLt's, so judge both
    bf16 paths by their deviation from the fp32 path."""
    r = _run(case)
    l_fast, l_old, l_32 = r["fast"][1], r["old"][1], r["fp32"][1]
    fin = torch.isfinite(l_32)
    assert torch.equal(torch.isfinite(l_fast), fin)
    assert torch.equal(torch.isfinite(l_old), fin)
    e_fast = (l_fast[fin] - l_32[fin]).abs().double()
    e_old = (l_old[fin] - l_32[fin]).abs().double()
    stats = {
        name: (float(e.median()), float(torch.quantile(e, 0.99)))
        for name, e in (("fast", e_fast), ("old", e_old))
    }
    corr = _rankcorr(l_fast[fin], l_32[fin])
    print(f"[{case}] |lsa - fp32| median/p99: fast {stats['fast'][0]:.4e}/"
          f"{stats['fast'][1]:.4e} old {stats['old'][0]:.4e}/"
          f"{stats['old'][1]:.4e} rank corr {corr:.5f}")
    assert stats["fast"][0] <= 2.0 * stats["old"][0]
    assert stats["fast"][1] <= 2.0 * stats["old"][1]
    assert corr > 0.98


WIDE_BAD = [5, 650]  # rows of the wide case given out-of-range predictions


@functools.lru_cache(maxsize=None)
def _run_wide():
    """The skewed case with LSA(max_features=200), so that FusedPrioritizer
    itself launches the wide (more than 64 features) whiten instantiation,
    plus two predictions outside the fitted range. The LSA workspaces are
    filled with NaN before the judged call."""
    from simple_tip_amd.core.surprise import DSA, LSA, MultiModalSA
    from simple_tip_amd.engine.serving import FusedPrioritizer
    from test_gpu_lsa_oracles import NAN_BITS

    dev = torch.device("cuda:0")
    ats, pred, test, tp = _inputs("skewed")
    tp = tp.clone()
    n_fused = int(((tp >= 0) & (tp < 7)).sum())
    assert bool(((tp[WIDE_BAD] >= 0) & (tp[WIDE_BAD] < 7)).all()), (
        "the rows given out-of-range predictions must be ordinary fused rows")
    tp[WIDE_BAD] = torch.tensor([-1, 100000])
    dsa = DSA(ats, pred, device=dev)
    lsa = MultiModalSA.build_by_class(
        ats, pred, lambda a, p: LSA(a, max_features=200, device=dev)
    )
    fast = FusedPrioritizer(dsa, lsa, dev, pairwise_dtype=torch.bfloat16)
    assert fast.fast and fast.lsa_ready
    assert fast.lsa_d > 64
    test, tp = test.to(dev), tp.to(dev)
    fast(test, tp)  # allocates the workspaces
    torch.cuda.synchronize()
    ws = fast._ws[tuple(test.shape)]
    ws["white"].view(torch.int16).fill_(NAN_BITS)
    ws["wan"].fill_(float("nan"))
    ws["pkde"].fill_(float("nan"))
    out = fast(test, tp)
    torch.cuda.synchronize()
    return {"fast_obj": fast, "ws": ws, "test": test, "tp": tp, "out": out,
            "n_fused": n_fused - len(WIDE_BAD)}


def test_wide_lsa_stage_oracles():
    """Each LSA stage of a d > 64 call against its float64 oracle
    (tests/test_gpu_lsa_oracles.py), fed the call's own workspaces."""
    from test_gpu_lsa_oracles import (
        NAN_BITS, lsa_score_check, rownorm_check, whiten_check,
    )

    r = _run_wide()
    fast, ws = r["fast_obj"], r["ws"]
    worst_w = whiten_check(
        r["test"].to(torch.bfloat16), ws["rowmap"], ws["tseg"], fast.lsa_nseg,
        fast.lsa_keep, fast.lsa_wt, ws["white"], prefill_bits=NAN_BITS,
    )
    tseg, wseg = ws["tseg"].tolist(), fast.lsa_nseg.tolist()
    worst_n = 0.0
    # `wan` rows of non-fused classes come from the NaN-prefilled `white` rows
    # the whiten kernel skips and are never read: there is no value to judge
    for c in range(fast.num_classes):
        lo, hi = tseg[c], tseg[c + 1]
        if hi > lo and wseg[c + 1] > wseg[c]:
            worst_n = max(worst_n,
                          rownorm_check(ws["white"][lo:hi], ws["wan"][lo:hi]))
    assert bool(torch.isnan(ws["wan"][tseg[-1]:]).all())
    worst_k = lsa_score_check(
        ws["white"], ws["wan"], fast.lsa_wtrainS16, fast.lsa_wnormS16,
        ws["tseg"], fast.lsa_nseg, ws["rowmap"], fast.lsa_cls_fused,
        fast.lsa_cls_const, r["out"][1], float("inf"),
    )
    print(f"[wide d={fast.lsa_d}] worst ratio: whiten {worst_w:.4f} "
          f"rownorm {worst_n:.4f} score {worst_k:.4f}")
    # the const / unseen / out-of-range rows the score oracle pinned exactly
    tp, lsa = r["tp"], r["out"][1]
    assert bool((lsa[tp == SINGLETON] == 0.0).all())
    assert bool((lsa[tp == UNSEEN] == float("inf")).all())
    assert bool((lsa[WIDE_BAD] == float("inf")).all())
    fused = (tp >= 0) & (tp < 7)
    assert int(fused.sum()) == r["n_fused"]
    assert int(fused.sum()) + int((tp == SINGLETON).sum()) + int(
        (tp == UNSEEN).sum()) + len(WIDE_BAD) == tp.numel()
    assert bool(torch.isfinite(lsa[fused]).all())


def test_const_and_unseen_classes_exact():
    r = _run("skewed")
    dsa, lsa = r["fast"]
    tp = r["tp"]
    single, unseen = tp == SINGLETON, tp == UNSEEN
    assert int(single.sum()) == 3 and int(unseen.sum()) == 4
    assert bool((lsa[single] == 0.0).all())
    assert bool(torch.isfinite(dsa[single]).all())
    assert bool((lsa[unseen] == float("inf")).all())
    assert bool((dsa[unseen] == float("inf")).all())
    assert torch.equal(lsa[single | unseen], r["old"][1][single | unseen])


def test_out_of_range_predictions():
    """Predictions outside [0, C) score +inf; every other row is unchanged
    (a row's result does not depend on where the plan places it)."""
    r = _run("uniform")
    fast, test, tp = r["fast_obj"], r["test"], r["tp"].clone()
    bad = torch.tensor([0, 130, 500, 776], device=tp.device)
    tp[bad] = torch.tensor([7, -1, 100000, -5], device=tp.device)
    dsa, lsa = fast(test, tp)
    assert bool((dsa[bad] == float("inf")).all())
    assert bool((lsa[bad] == float("inf")).all())
    ok = torch.ones_like(tp, dtype=torch.bool)
    ok[bad] = False
    assert torch.equal(dsa[ok], r["fast"][0][ok])
    assert torch.equal(lsa[ok], r["fast"][1][ok])


@pytest.mark.parametrize("case", CASES)
def test_stale_workspaces_and_determinism(case):
    r = _run(case)
    fast, test, tp = r["fast_obj"], r["test"], r["tp"]
    d1, l1 = fast(test, tp)
    assert torch.equal(d1, r["fast"][0]) and torch.equal(l1, r["fast"][1])
    torch.cuda.synchronize()
    for ws in fast._ws.values():
        for t in ws.values():
            t.fill_(float("nan") if t.is_floating_point() else -1)
    d2, l2 = fast(test, tp)
    assert torch.equal(d1, d2) and torch.equal(l1, l2)


def test_no_host_sync():
    r = _run("uniform")
    fast, test, tp = r["fast_obj"], r["test"], r["tp"]
    fast(test, tp)  # warm call: workspaces, streams
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        d, l = fast(test, tp)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(d, r["fast"][0]) and torch.equal(l, r["fast"][1])


def test_bf16_activations_equal_fp32_input():
    """bf16 ATs (what the fused forward hands over) are consumed directly."""
    r = _run("uniform")
    fast, test, tp = r["fast_obj"], r["test"], r["tp"]
    d, l = fast(test.to(torch.bfloat16), tp)
    assert torch.equal(d, r["fast"][0]) and torch.equal(l, r["fast"][1])


def test_fallback_selection(monkeypatch):
    from simple_tip_amd.core.surprise import DSA, LSA, MultiModalSA
    from simple_tip_amd.engine.serving import FusedPrioritizer

    r = _run("uniform")
    # fast=False is the old bf16 path: same object type, same results
    again = r["old_obj"](r["test"], r["tp"])
    assert torch.equal(again[0], r["old"][0])
    assert torch.equal(again[1], r["old"][1])

    dev = torch.device("cuda:0")
    rng = np.random.RandomState(11)
    ats = torch.from_numpy(rng.randn(900, 20).astype(np.float32))
    pred = torch.from_numpy(rng.randint(0, 2, 900))
    dsa = DSA(ats, pred, device=dev)
    lsa = MultiModalSA.build_by_class(
        ats, pred, lambda a, p: LSA(a, max_features=15, device=dev)
    )
    narrow = FusedPrioritizer(dsa, lsa, dev, pairwise_dtype=torch.bfloat16)
    assert not narrow.fast  # AT width 20 is not a multiple of 8
    ref = FusedPrioritizer(dsa, lsa, dev)
    assert not ref.fast  # fp32 mode
    test = torch.from_numpy(rng.randn(333, 20).astype(np.float32)).to(dev)
    tp = torch.from_numpy(rng.randint(0, 2, 333)).to(dev)
    d16, l16 = narrow(test, tp)
    d32, l32 = ref(test, tp)
    rel = ((d16 - d32).abs() / d32.abs().clamp_min(1e-3)).median()
    assert float(rel) < 0.02
    assert bool(torch.isfinite(l16).all())

    monkeypatch.setenv("TIP_NO_FAST_SCORING", "1")
    env_off = FusedPrioritizer(*_fit_small(dev), pairwise_dtype=torch.bfloat16)
    assert not env_off.fast
    monkeypatch.delenv("TIP_NO_FAST_SCORING")
    env_on = FusedPrioritizer(*_fit_small(dev), pairwise_dtype=torch.bfloat16)
    assert env_on.fast


@functools.lru_cache(maxsize=None)
def _fit_small(dev):
    from simple_tip_amd.core.surprise import DSA, LSA, MultiModalSA

    rng = np.random.RandomState(5)
    ats = torch.from_numpy(rng.randn(400, 64).astype(np.float32))
    pred = torch.from_numpy(rng.randint(0, 3, 400))
    dsa = DSA(ats, pred, device=dev)
    lsa = MultiModalSA.build_by_class(
        ats, pred, lambda a, p: LSA(a, max_features=32, device=dev)
    )
    return dsa, lsa, dev
