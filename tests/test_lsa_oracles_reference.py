"""CPU proof that the float64 oracles of tests/test_gpu_lsa_oracles.py bite.

Each oracle first judges a torch fp32 emulation of its stage (fp32
accumulation of the bf16 operands, bf16 round-to-nearest-even output; the
KDE with the kernels' structure of 64-column halves, 128-column blocks and a
streaming fold) on the very cases the GPU tests run, and must accept it.
Then it judges mutants of that emulation, and must reject every one:

  whiten
    W1  bf16 truncation instead of round-to-nearest-even
    W2  the last kept column dropped
    W3  the `keep` rows of two classes swapped
    W4  `wt` transposed (M_c instead of M_c^T)
    W5  a pad row of a fused class not zeroed
    W6  a row of the non-fused class written
  row norms
    N1  the last element of every row left out
    N2  a truncating (bf16) accumulator
  KDE
    K1  the last train column of a class omitted
    K2  an empty 64-column half contributing exp(0)
    K3  the norm of the wrong (neighbouring) test row
    K4  a -FLT_MAX result for far rows (every term "underflowed")
    K5  exp and log of bf16 accuracy
    K6  column block 1 lost on far rows (only block 0 folded)
  final score
    F1  +(lse + const) instead of -(lse + const)
    F2  an unplaced row written
    F3  the const of the neighbouring class

A mutant that passed would mean a kernel with that defect passes the GPU
tests too.
"""

import numpy as np
import pytest
import torch

from test_gpu_lsa_oracles import (
    FLT_MAX,
    NAN_BITS,
    SEG,
    WHITEN_TEST_ROWS,
    kde_case_exact,
    kde_case_far,
    kde_case_planted,
    kde_check,
    kde_padded_layout,
    lsa_score_check,
    padded_tseg,
    rownorm_check,
    shuffled_pred,
    whiten_check,
    whiten_inputs,
)

# ---------------------------------------------------------------------------
# fp32 emulations of the stages
# ---------------------------------------------------------------------------


def plan(pred, nclasses):
    """(tseg, rowmap, dest) of the segment plan (stable within a class)."""
    b = pred.shape[0]
    bp = SEG * ((b + SEG - 1) // SEG + nclasses)
    counts = [int((pred == c).sum()) for c in range(nclasses)]
    tseg = padded_tseg(counts)
    rowmap = torch.full((bp,), -1, dtype=torch.int32)
    dest = torch.full((b,), -1, dtype=torch.int32)
    for c in range(nclasses):
        rows = torch.nonzero(pred == c, as_tuple=True)[0]
        rowmap[tseg[c]:tseg[c] + rows.numel()] = rows.int()
        dest[rows] = torch.arange(tseg[c], tseg[c] + rows.numel()).int()
    return torch.tensor(tseg, dtype=torch.int32), rowmap, dest


def truncate_bf16(x32):
    return (x32.view(torch.int32) & -65536).view(torch.float32).bfloat16()


def emulate_whiten(h, tseg, rowmap, mutant=None):
    d, nclasses = h["d"], len(WHITEN_TEST_ROWS)
    keep, wt = h["keep"].long().clone(), h["wt"]
    if mutant == "swap_keep":
        keep[[0, 4]] = keep[[4, 0]]
    white = torch.empty(rowmap.shape[0], d, dtype=torch.bfloat16)
    white.view(torch.int16).fill_(NAN_BITS)
    tseg_l, wseg_l = tseg.tolist(), h["wseg"].tolist()
    for c in range(nclasses):
        lo, hi = tseg_l[c], tseg_l[c + 1]
        if hi <= lo:
            continue
        if wseg_l[c + 1] <= wseg_l[c]:
            if mutant == "write_nonfused":
                white[lo] = 0
            continue
        src = rowmap[lo:hi].long()
        a = h["ats"][src.clamp_min(0)][:, keep[c]].float()
        a[src < 0] = 0
        if mutant == "drop_last_column":
            a[:, -1] = 0
        w = wt[c, :d, :d].float()          # w[n, k]
        acc = a @ (w if mutant == "transpose" else w.t())
        white[lo:hi] = truncate_bf16(acc) if mutant == "truncate" else acc.bfloat16()
        if mutant == "dirty_pad":
            white[hi - 1, 0] = -0.0
    return white


def emulate_rownorm(x, mutant=None):
    f = x.float()
    if mutant == "drop_last":
        f = f[:, :-1]
    if mutant == "bf16_accumulator":
        s = torch.zeros(f.shape[0])
        for k in range(f.shape[1]):
            s = truncate_bf16(s + f[:, k] * f[:, k]).float()
        return s
    return (f * f).sum(dim=1)


def _round_bf16(x):
    return x.bfloat16().float()


def emulate_kde(a, b, an, bn, mutant=None):
    """fp32 lse of rows a against train rows b, structured as the kernels:
    (max, sum) per 64-column half, halves merged per 128-column block, blocks
    folded in ascending order."""
    a, b = a.float(), b.float()
    if mutant == "omit_last_column":
        b, bn = b[:-1], bn[:-1]
    if mutant == "wrong_norm":
        an = torch.roll(an, 1)
    n = b.shape[0]
    d2 = (an[:, None] + bn[None, :] - 2.0 * (a @ b.t())).clamp_min(0.0)
    t = -0.5 * d2
    exp = (lambda x: _round_bf16(torch.exp(x))) if mutant == "coarse_exp" else torch.exp
    log = (lambda x: _round_bf16(torch.log(x))) if mutant == "coarse_exp" else torch.log
    mm = torch.full((a.shape[0],), -FLT_MAX)
    ss = torch.zeros(a.shape[0])
    for col0 in range(0, n, SEG):
        halves = []
        for h0 in (col0, col0 + 64):
            th = t[:, h0:min(h0 + 64, n)]
            if th.shape[1] == 0:
                halves.append((torch.full_like(mm, -FLT_MAX), torch.zeros_like(ss)))
                continue
            m = th.max(dim=1).values
            halves.append((m, exp(th - m[:, None]).sum(dim=1)))
        (m0, s0), (m1, s1) = halves
        if mutant == "empty_half_exp0" and bool((s1 == 0).all()):
            m1, s1 = m0.clone(), torch.ones_like(s0)   # exp(tmax - tmax)
        m = torch.maximum(m0, m1)
        s = s0 * exp(m0 - m) + s1 * exp(m1 - m)
        new = torch.maximum(mm, m)
        ss = ss * exp(mm - new) + s * exp(m - new)
        mm = new
    lse = mm + log(ss)
    if mutant == "underflow_far":
        lse = torch.where(lse < -1000.0, torch.full_like(lse, -FLT_MAX), lse)
    if mutant == "lose_block1_far" and n > SEG:
        first = emulate_kde(a, b[:SEG], an, bn[:SEG])
        lse = torch.where(lse < -1000.0, first, lse)
    return lse


def emulate_grouped_kde(padded, train, an, bn, tseg, nseg, mutant=None):
    lse = torch.zeros(padded.shape[0])
    for c in range(len(tseg) - 1):
        lo, hi = tseg[c], tseg[c + 1]
        if hi > lo:
            lse[lo:hi] = emulate_kde(padded[lo:hi], train[nseg[c]:nseg[c + 1]],
                                     an[lo:hi], bn[nseg[c]:nseg[c + 1]], mutant)
    return lse


def _norms(x):
    f = x.float()
    return (f * f).sum(dim=1)


# ---------------------------------------------------------------------------
# whiten
# ---------------------------------------------------------------------------

WHITEN_WIDTHS = [1, 15, 17, 33, 64, 65, 80, 300, 320]


def _whiten_run(d, mutant=None):
    h = whiten_inputs(d)
    tseg, rowmap, _ = plan(h["pred"], len(WHITEN_TEST_ROWS))
    assert tseg.tolist() == [0, 256, 384, 384, 512, 640]
    white = emulate_whiten(h, tseg, rowmap, mutant)
    return whiten_check(h["ats"], rowmap, tseg, h["wseg"], h["keep"], h["wt"],
                        white, prefill_bits=NAN_BITS)


@pytest.mark.parametrize("d", WHITEN_WIDTHS)
def test_whiten_oracle_accepts_emulation(d):
    worst = _whiten_run(d)
    print(f"[whiten emulation d={d}] worst ratio {worst:.4f}")
    assert worst <= 1.0


@pytest.mark.parametrize("mutant", ["truncate", "drop_last_column", "swap_keep",
                                    "transpose", "dirty_pad", "write_nonfused"])
@pytest.mark.parametrize("d", [17, 64, 65, 300])
def test_whiten_oracle_rejects_mutants(d, mutant):
    with pytest.raises(AssertionError):
        _whiten_run(d, mutant)


def test_whiten_oracle_rejects_single_column_mutants():
    """d = 1: dropping the only column, or truncating, must still show."""
    for mutant in ("truncate", "drop_last_column", "swap_keep"):
        with pytest.raises(AssertionError):
            _whiten_run(1, mutant)


# ---------------------------------------------------------------------------
# row norms
# ---------------------------------------------------------------------------


def _rows(k):
    x = np.random.RandomState(3000 + k).randn(9, k).astype(np.float32)
    return torch.from_numpy(x).bfloat16()


@pytest.mark.parametrize("k", [1, 7, 8, 9, 40, 300, 512, 520])
def test_rownorm_oracle(k):
    x = _rows(k)
    rownorm_check(x, emulate_rownorm(x))
    for mutant in ("drop_last", "bf16_accumulator"):
        if k == 1 and mutant == "bf16_accumulator":
            # one exact square: rounding it to bf16 is the only error there is
            continue
        with pytest.raises(AssertionError):
            rownorm_check(x, emulate_rownorm(x, mutant))


# ---------------------------------------------------------------------------
# KDE
# ---------------------------------------------------------------------------

KDE_CASES = {
    "exact": lambda: kde_case_exact(False),
    "exact_dup": lambda: kde_case_exact(True),
    "planted8": lambda: kde_case_planted(8),
    "planted37": lambda: kde_case_planted(37),
    "planted300": lambda: kde_case_planted(300),
    "far": kde_case_far,
}


def _kde_run(case, dtype, mutant=None):
    padded, train, tseg, nseg = kde_padded_layout(case, dtype)
    an, bn = _norms(padded), _norms(train)
    lse = emulate_grouped_kde(padded, train, an, bn, tseg, nseg, mutant)
    return kde_check(padded, train, an, bn, tseg, nseg, lse,
                     exact=case.get("exact", False))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("name", list(KDE_CASES))
def test_kde_oracle_accepts_emulation(name, dtype):
    worst = _kde_run(KDE_CASES[name](), dtype)
    print(f"[kde emulation {name} {dtype}] worst ratio {worst:.4f}")
    assert worst <= 1.0


def test_kde_oracle_accepts_flat_single_feature():
    case = kde_case_planted(1)
    for te, tr in zip(case["test"], case["train"]):
        an, bn = _norms(te), _norms(tr)
        kde_check(te, tr, an, bn, [0, te.shape[0]], [0, tr.shape[0]],
                  emulate_kde(te, tr, an, bn))


@pytest.mark.parametrize("name,mutant", [
    ("planted8", "omit_last_column"), ("planted37", "omit_last_column"),
    ("planted300", "omit_last_column"), ("exact", "omit_last_column"),
    ("planted37", "empty_half_exp0"), ("exact", "empty_half_exp0"),
    ("far", "empty_half_exp0"),
    ("planted8", "wrong_norm"), ("planted300", "wrong_norm"),
    ("exact", "wrong_norm"),
    ("far", "underflow_far"), ("far", "lose_block1_far"),
    ("exact", "coarse_exp"), ("planted37", "coarse_exp"),
])
def test_kde_oracle_rejects_mutants(name, mutant):
    with pytest.raises(AssertionError):
        _kde_run(KDE_CASES[name](), torch.bfloat16, mutant)


# ---------------------------------------------------------------------------
# final scores
# ---------------------------------------------------------------------------


def _final_run(mutant=None):
    case = kde_case_planted(40)
    rows = [t.shape[0] for t in case["test"]]
    c = len(rows)
    pred = shuffled_pred(rows, 9, [-1, c, 100000, -5])
    b = pred.shape[0]
    src = torch.zeros(b, case["k"])
    for cls, t in enumerate(case["test"]):
        src[pred == cls] = t
    tseg, rowmap, dest = plan(pred, c)
    white = torch.zeros(rowmap.shape[0], case["k"], dtype=torch.bfloat16)
    ok = dest >= 0
    white[dest[ok].long()] = src[ok].bfloat16()
    train = torch.cat(case["train"]).bfloat16()
    nseg = [0] + [int(v) for v in np.cumsum([t.shape[0] for t in case["train"]])]
    wan, bn = _norms(white), _norms(train)
    lse = emulate_grouped_kde(white, train, wan, bn, tseg.tolist(), nseg)
    fused = torch.tensor([1, 0, 1, 1, 0], dtype=torch.int32)
    const = torch.tensor([0.5, float("inf"), 0.0, -1.25, 2.0])
    cls = pred.clamp(0, c - 1)
    used = torch.roll(const, 1) if mutant == "wrong_const" else const
    score = lse[dest.clamp_min(0).long()] + used[cls]
    score = score if mutant == "sign" else -score
    out = torch.where(fused[cls].bool(), score, used[cls])
    out[~ok] = -12345.0
    if mutant == "write_unplaced":
        out[torch.nonzero(~ok)[0]] = 0.0
    return lsa_score_check(white, wan, train, bn, tseg, nseg, rowmap, fused,
                           const, out, -12345.0)


def test_final_score_oracle():
    assert _final_run() <= 1.0
    for mutant in ("sign", "write_unplaced", "wrong_const"):
        with pytest.raises(AssertionError):
            _final_run(mutant)
