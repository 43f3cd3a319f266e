"""Float64 oracles for the LSA half of the sync-free scoring path:
grouped_whiten_bf16_kernel -> rownorm_bf16_kernel ->
grouped_pairwise_bf16_kernel<EPI_KDE> -> grouped_kde_final_kernel
(ops/hip/segment.hip, ops/hip/pairwise.hip).

Every oracle is stage-local: it reads the operand values the kernel read
(the previous stage's own output, bf16 or fp32, widened exactly to float64)
and judges one stage. No row and no element is left out of an assertion.
The oracle functions below are plain functions on tensors of any device;
tests/test_lsa_oracles_reference.py runs them on the CPU against a torch
emulation of each stage and against mutants of it, and
tests/test_gpu_serving_fast.py feeds them a FusedPrioritizer call.

u = 2^-24 is the unit roundoff of fp32 (round to nearest) throughout.

Whiten (whiten_check)
    ref[p, n] = sum_k a[p, k] * w[n, k] in float64 on the bf16 values and
    S[p, n] the same sum over absolute values. A product of two bf16 values
    has 16 significant bits and is exact in fp32; the MFMA adds at most KP of
    them in some order, each addition rounding once, so the fp32 accumulator
    is within E = KP * u * S of ref. The kernel then rounds it to bf16
    (nearest even), which is monotone, hence
        bf16(ref - E') <= got <= bf16(ref + E'),  E' = E + u * |ref|
    where the extra u * |ref| covers the float64 -> float32 step of the
    reference's own float64 -> float32 -> bf16 rounding. The printed figure
    is |got - ref| / (E' + 2^-8 * (|ref| + E')): 2^-8 is half a bf16 ulp.

Row norms (rownorm_check)
    A lane of rownorm_bf16_kernel runs s = fmaf(f, f, s) over n elements:
    n = 8 * ceil(K / 512) on the 16-byte branch (K % 8 == 0: 8 elements per
    trip, lanes 64 * 8 apart), n = ceil(K / 64) on the scalar branch. f * f
    has 16 significant bits, so each fmaf rounds once and the first one
    (s = 0) not at all: n - 1 roundings. The xor tree adds 6 more. Every
    term is non-negative, so each f^2 reaches the result through at most
    n + 5 factors (1 + delta), |delta| <= u, and
        |out - sum f^2| <= ((1 + u)^(n + 5) - 1) * sum f^2
                        <= (n + 6) * u * sum f^2      (n <= 16 here).

KDE (kde_check)
    lse_i = log sum_j exp(-d2_ij / 2), d2_ij = max(an_i + bn_j - 2 a_i.b_j,
    0), in float64 on the operand values and on the fp32 norms the kernel
    was given. Tolerance per row: 0.5 * max_j E_ij + R_i.

    E_ij = (K + 8) * u * (an_i + bn_j + 2 sum_k |a_ik b_jk|) bounds the
    kernel's error in d2_ij (K accumulations, the two norm additions, the
    scaling); lse is 1-Lipschitz in the sup norm of t = -d2 / 2, which gives
    the factor 0.5 and the max; the clamp at 0 is 1-Lipschitz too. Where
    every product, norm and distance is exact in fp32 in any order
    (kde_case_exact) the E term is dropped and R stands alone.

    R_i covers everything after the distances. Write M for the row's final
    maximum of t. The kernel's sum is sum_j exp(t_j - M) * (1 + rho_j), and
    log(sum_j e_j (1 + rho_j)) - log(sum_j e_j) <= sum_j w_j |rho_j| with w
    the softmax weights. rho_j collects, along term j's way to the result:
      * every rescaling exp(x) is __expf(x) = v_exp_f32(x * log2e): the
        subtraction that forms x rounds once (u |x|), the fp32 constant
        log2e is off by 0.23 u relative, the product rounds once: the
        exponent is off by at most 2.25 u |x|, and v_exp_f32 is documented
        to 1 ulp = 2 u relative. Term j is rescaled from its 64-column
        half's maximum to the block's, and on to each larger running maximum
        of the fold. All these x have one sign and telescope to M - t_j, so
        the exponent errors add up to 2.25 u (M - t_j); and
        sum_j w_j (M - t_j) = M - lse + H(w) <= H(w) <= ln N.
      * constants per stage: the in-half exp (2 u) and sum chain (at most
        4 terms in a lane less the exact first addition, then a 4-step xor
        tree on the bf16 kernel; 2 terms and a 5-step tree on the fp32 one:
        7 u); the half merge (exp 2 u, product u, sum u); each fold step
        after the first (exp 2 u, product u, sum u). Together
        (9 + 4 + 4 (jb - 1)) u = (9 + 4 jb) u for jb column blocks.
    The largest term is exp(0) = 1 exactly, so the sum ss lies in [1, N].
    __logf(ss) = v_log_f32(ss) * ln2: v_log_f32 is documented to 1 ulp, taken
    here as 2 u * max(log2 ss, 1) so that no relative accuracy is assumed
    just above ss = 1; the fp32 constant and the product add 2 u * ln ss:
    at most (4 ln N + 1.4) u. The final mm + log rounds once: u * |lse|.
    Terms flushed to zero below 2^-126 and all second-order products are
    below 1e-9 u and sit in the slack of the constant:
        R_i = u * (|lse_i| + 6.25 ln N + 4 jb + 16)
    with N the class's train rows and jb = ceil(N / 128). None of these
    figures comes from a GPU run. The ln N coefficient is 6.25 and not the 2
    of a sum-of-|x_j| argument alone because the logarithm is budgeted
    absolutely here, at 4 ln N, on top of the 2.25 ln N of the exponents.

    A score of the final kernel is -(lse + const), one more fp32 addition:
    score_tol = tol + u * (|score| + tol)   (lsa_score_check).
"""

import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
FLT_MAX = float(np.finfo(np.float32).max)
NAN_BITS = 0x7FC1   # a bf16 quiet NaN the kernels never produce themselves
SEG = 128


# ---------------------------------------------------------------------------
# Oracles (device-agnostic, float64 on the CPU)
# ---------------------------------------------------------------------------


def _cpu64(t):
    return t.detach().to("cpu").double()


def _ints(t):
    if torch.is_tensor(t):
        t = t.detach().to("cpu").tolist()
    return [int(v) for v in t]


def bf16_rne(x64):
    """float64 -> float32 -> bf16, both round-to-nearest-even, as float64."""
    return x64.float().bfloat16().double()


def whiten_check(ats, rowmap, tseg, wseg, keep, wt, white, prefill_bits=None):
    """Judge the whole `white` workspace of one grouped_whiten_bf16 call.

    ats [B, D] bf16, rowmap [bp], tseg / wseg [C+1], keep [C, d] int32,
    wt [C, pad16(d), pad32(d)] bf16, white [bp, d] bf16. Placed rows of a
    fused class (non-empty wseg range) must lie in the bf16 interval of the
    module docstring, their pad rows must be +0.0, and with `prefill_bits`
    every other row must still hold that bit pattern. Returns the worst
    error-to-bound figure; raises AssertionError on any violation."""
    a_all = _cpu64(ats)
    w_all = _cpu64(wt)
    got_bits = white.detach().to("cpu").contiguous().view(torch.int16)
    got_all = _cpu64(white)
    rowmap, tseg, wseg = _ints(rowmap), _ints(tseg), _ints(wseg)
    keep = keep.detach().to("cpu").long()
    nclasses, d = keep.shape
    kp = w_all.shape[2]
    b = a_all.shape[0]
    assert tuple(w_all.shape[:2]) == (nclasses, (d + 15) // 16 * 16)
    assert got_all.shape == (len(rowmap), d)
    seen = torch.zeros(len(rowmap), dtype=torch.bool)
    worst = 0.0
    for c in range(nclasses):
        lo, hi = tseg[c], tseg[c + 1]
        if hi <= lo or wseg[c + 1] <= wseg[c]:
            continue
        seen[lo:hi] = True
        src = torch.tensor(rowmap[lo:hi])
        placed = (src >= 0) & (src < b)
        pad_bits = got_bits[lo:hi][~placed]
        assert bool((pad_bits == 0).all()), (
            f"class {c}: a pad row of `white` is not +0.0")
        if not bool(placed.any()):
            continue
        a = a_all[src[placed]][:, keep[c]]
        w = w_all[c, :d, :d]                 # w[n, k]
        ref = a @ w.t()
        e = kp * U * (a.abs() @ w.abs().t()) + U * ref.abs()
        got = got_all[lo:hi][placed]
        lo_b, hi_b = bf16_rne(ref - e), bf16_rne(ref + e)
        inside = (lo_b <= got) & (got <= hi_b)
        denom = e + 2.0 ** -8 * (ref.abs() + e)
        diff = (got - ref).abs()
        ratio = torch.where(diff == 0, torch.zeros_like(diff), diff / denom)
        ratio = torch.nan_to_num(ratio, nan=float("inf"))
        worst = max(worst, float(ratio.max()))
        assert bool(inside.all()), (
            f"class {c}: {int((~inside).sum())} of {inside.numel()} elements "
            f"outside the bf16 interval, worst ratio {float(ratio.max()):.3f}")
    if prefill_bits is not None:
        want = torch.tensor(prefill_bits, dtype=torch.int32).to(torch.int16)
        untouched = got_bits[~seen]
        assert bool((untouched == want).all()), (
            "a row of a non-fused class or past tseg[C] was written")
    return worst


def rownorm_chain(k):
    """Per-lane fmaf chain length of rownorm_bf16_kernel at width k."""
    if k % 8 == 0:
        return 8 * math.ceil(k / 512)
    return math.ceil(k / 64)


def rownorm_check(x, out):
    """out [rows] fp32 against the float64 sum of squares of x [rows, K]
    bf16; every row. Returns the worst error-to-bound ratio."""
    f = _cpu64(x)
    ref = (f * f).sum(dim=1)
    got = _cpu64(out)
    bound = (rownorm_chain(x.shape[1]) + 6) * U * ref
    diff = (got - ref).abs()
    ratio = torch.where(diff == 0, torch.zeros_like(diff), diff / bound)
    ratio = torch.nan_to_num(ratio, nan=float("inf"))
    assert bool((ratio <= 1.0).all()), (
        f"K={x.shape[1]}: worst ratio {float(ratio.max()):.3f}")
    return float(ratio.max()) if ratio.numel() else 0.0


def kde_reference(a, b, an, bn, exact=False):
    """(lse, tol) in float64 of test rows a [m, K] against the train rows
    b [N, K] of one class, with the fp32 norms the kernel was given. With
    `exact` the caller vouches that the kernel's distances carry no rounding
    at all (kde_case_exact) and the tolerance is R alone."""
    a, b, an, bn = _cpu64(a), _cpu64(b), _cpu64(an), _cpu64(bn)
    n, k = b.shape
    nn = an[:, None] + bn[None, :]
    d2 = (nn - 2.0 * (a @ b.t())).clamp_min(0.0)
    lse = torch.logsumexp(-0.5 * d2, dim=1)
    e = (k + 8) * U * (nn + 2.0 * (a.abs() @ b.abs().t()))
    jb = (n + SEG - 1) // SEG
    r = U * (lse.abs() + 6.25 * math.log(n) + 4 * jb + 16)
    return lse, (0.0 if exact else 0.5) * e.max(dim=1).values + r


def kde_check(test, train, an, bn, tseg, nseg, lse, exact=False):
    """Judge lse [rows] of a grouped KDE call: test [rows, K] in padded
    class-sorted layout (tseg), train class-concatenated (nseg), norms as
    given to the kernel. The flat call is the one-class layout
    tseg = [0, M], nseg = [0, N]. Every row below tseg[C] is judged, pad
    rows included (their operand is the zero row); a class without train
    rows must report -FLT_MAX. Returns the worst error-to-tolerance ratio."""
    tseg, nseg = _ints(tseg), _ints(nseg)
    got_all = _cpu64(lse)
    worst = 0.0
    for c in range(len(tseg) - 1):
        lo, hi = tseg[c], tseg[c + 1]
        if hi <= lo:
            continue
        got = got_all[lo:hi]
        if nseg[c + 1] <= nseg[c]:
            assert bool((got == -FLT_MAX).all()), f"class {c}: empty train set"
            continue
        ref, tol = kde_reference(test[lo:hi], train[nseg[c]:nseg[c + 1]],
                                 an[lo:hi], bn[nseg[c]:nseg[c + 1]], exact)
        assert bool(torch.isfinite(got).all()) and bool((got > -FLT_MAX).all()), (
            f"class {c}: non-finite lse")
        ratio = (got - ref).abs() / tol
        worst = max(worst, float(ratio.max()))
        assert bool((ratio <= 1.0).all()), (
            f"class {c}: {int((ratio > 1.0).sum())} of {ratio.numel()} rows "
            f"outside the tolerance, worst ratio {float(ratio.max()):.3f} at "
            f"row {lo + int(ratio.argmax())}")
    return worst


def lsa_score_check(white, wan, wtrain, wnorm, tseg, wseg, rowmap, cls_fused,
                    cls_const, out, unplaced, exact=False):
    """Judge the final scores out [B] of grouped_kde_plan against the KDE
    oracle fed the call's own workspaces: fused classes within score_tol of
    -(lse + const), the other classes exactly their const, rows the plan
    placed nowhere exactly `unplaced`. Returns the worst ratio."""
    tseg_l, wseg_l, rowmap_l = _ints(tseg), _ints(wseg), _ints(rowmap)
    fused, const = _ints(cls_fused), _cpu64(cls_const)
    got_all = _cpu64(out)
    b = got_all.shape[0]
    seen = torch.zeros(b, dtype=torch.bool)
    worst = 0.0
    for c in range(len(tseg_l) - 1):
        lo, hi = tseg_l[c], tseg_l[c + 1]
        src = torch.tensor(rowmap_l[lo:hi], dtype=torch.long)
        placed = (src >= 0) & (src < b)
        if not bool(placed.any()):
            continue
        rows = src[placed]
        assert not bool(seen[rows].any())
        seen[rows] = True
        got = got_all[rows]
        if not fused[c]:
            assert bool((got == const[c]).all()), f"class {c}: const score"
            continue
        assert wseg_l[c + 1] > wseg_l[c]
        ref, tol = kde_reference(
            white[lo:hi][placed.to(white.device)],
            wtrain[wseg_l[c]:wseg_l[c + 1]], wan[lo:hi][placed.to(wan.device)],
            wnorm[wseg_l[c]:wseg_l[c + 1]], exact)
        score = -(ref + const[c])
        tol = tol + U * (score.abs() + tol)
        assert bool(torch.isfinite(got).all()), f"class {c}: non-finite score"
        ratio = (got - score).abs() / tol
        worst = max(worst, float(ratio.max()))
        assert bool((ratio <= 1.0).all()), (
            f"class {c}: {int((ratio > 1.0).sum())} of {ratio.numel()} scores "
            f"outside the tolerance, worst ratio {float(ratio.max()):.3f}")
    rest = got_all[~seen]
    assert bool((rest == unplaced).all()), "an unplaced row was written"
    return worst


# ---------------------------------------------------------------------------
# Case builders (host tensors; shared by the CPU reference tests)
# ---------------------------------------------------------------------------

WHITEN_TEST_ROWS = [129, 5, 0, 3, 70]
WHITEN_TRAIN_ROWS = [7, 3, 2, 0, 5]      # class 3 is not fused
OUT_OF_RANGE = [-1, len(WHITEN_TEST_ROWS), 100000, -5]
WHITEN_WIDTHS_NT4 = [1, 15, 16, 17, 31, 32, 33, 64]
WHITEN_WIDTHS_NT20 = [65, 80, 96, 97, 300, 320]


def shuffled_pred(rows, seed, out_of_range=OUT_OF_RANGE):
    """Class ids of `rows` rows per class, shuffled, with the out-of-range
    ids inserted at random places."""
    rng = np.random.RandomState(seed)
    pred = np.repeat(np.arange(len(rows)), rows).astype(np.int64)
    pred = rng.permutation(np.concatenate([pred, np.array(out_of_range)]))
    return torch.from_numpy(pred)


def padded_tseg(rows):
    seg = [0]
    for r in rows:
        seg.append(seg[-1] + (r + SEG - 1) // SEG * SEG)
    return seg


def whiten_inputs(d, seed=0):
    """Host tensors of the whiten layout at width d: pred [211], ats [211, D]
    bf16, wseg, keep [5, d], wt [5, pad16(d), pad32(d)] bf16."""
    rng = np.random.RandomState(1000 + d + seed)
    c = len(WHITEN_TEST_ROWS)
    pred = shuffled_pred(WHITEN_TEST_ROWS, 77 + d)
    dfull = d + 11
    ats = torch.from_numpy(
        rng.randn(pred.shape[0], dfull).astype(np.float32)).bfloat16()
    keep = np.zeros((c, d), dtype=np.int32)
    ends = [0, dfull - 1]
    for cls in range(c):
        if d == 1:
            # one column each: the classes share out the two end columns
            keep[cls, 0] = ends[cls] if cls < 2 else 1 + cls
        else:
            mid = rng.choice(np.arange(1, dfull - 1), d - 2, replace=False)
            keep[cls] = np.sort(np.concatenate([ends, mid]))
    np_, kp = (d + 15) // 16 * 16, (d + 31) // 32 * 32
    wt = torch.zeros(c, np_, kp, dtype=torch.bfloat16)
    for cls in range(c):
        # asymmetric M_c [k, n]; the table holds wt[c, n, k] = M_c[k, n]
        m = torch.from_numpy(
            (rng.randn(d, d) / math.sqrt(d)).astype(np.float32)).bfloat16()
        wt[cls, :d, :d] = m.t()
    wseg = torch.tensor(np.concatenate([[0], np.cumsum(WHITEN_TRAIN_ROWS)]),
                        dtype=torch.int32)
    return dict(pred=pred, ats=ats, keep=torch.from_numpy(keep), wt=wt,
                wseg=wseg, d=d)


KDE_TRAIN_ROWS = [130, 1, 64, 65, 129]


def _norm_rows(rng, rows, k):
    return torch.from_numpy(rng.randn(rows, k).astype(np.float32))


def kde_case_planted(k, seed=0):
    """Per class: train rows N(0, 1) and as many test rows, test row i being
    train row j(i) = i (every column once, first and last included) plus
    0.01 * noise; every other train row is far away."""
    rng = np.random.RandomState(2000 + k + seed)
    train = [_norm_rows(rng, n, k) for n in KDE_TRAIN_ROWS]
    test = [t + 0.01 * _norm_rows(rng, t.shape[0], k) for t in train]
    return dict(k=k, train=train, test=test)


def kde_case_exact(duplicate):
    """Entries from {-2..2} / 4 at K = 40: products, norms and distances are
    multiples of 1/16 below 2^8, exact in fp32 in any order, so E = 0 in
    effect and only R is under test. `duplicate` makes one test row of every
    class equal to a train row (d2 = 0, where the clamp sits)."""
    rng = np.random.RandomState(2100 + int(duplicate))
    k = 40
    train = [torch.from_numpy(rng.randint(-2, 3, (n, k)).astype(np.float32)) / 4
             for n in KDE_TRAIN_ROWS]
    rows = [129, 5, 3, 70, 64]
    test = [torch.from_numpy(rng.randint(-2, 3, (m, k)).astype(np.float32)) / 4
            for m in rows]
    if duplicate:
        for t, tr in zip(test, train):
            t[t.shape[0] // 2] = tr[tr.shape[0] - 1]
    return dict(k=k, train=train, test=test, exact=True)


FAR_ROWS = 20


def kde_case_far(seed=0):
    """Class 0: 130 train rows, the last two (column block 1, whose upper
    64-column half is empty) shifted by +0.5; its first FAR_ROWS test rows are
    shifted by +30 in every coordinate, so d2 is about 1e5. The shift of the
    two block-1 rows lowers their d2 / 2 by K (30 - 0.25) / 2 = 1785 on average,
    against a spread of about 60 sqrt(K) / 2 = 330 per train row (the
    nearest of 128 lies some 900 below the mean): for every
    far row the nearest train row is in block 1 and all of block 0 is at
    least 100 (here about 870 to 920) further in d2 / 2. That is
    asserted below, on the fp32 and on the bf16 values. Class 1 is an
    ordinary small class."""
    rng = np.random.RandomState(2200 + seed)
    k = 120
    tr0 = _norm_rows(rng, 130, k)
    tr0[128:] += 0.5
    te0 = _norm_rows(rng, 25, k)
    te0[:FAR_ROWS] += 30.0
    for dtype in (torch.float32, torch.bfloat16):
        t = -0.5 * torch.cdist(te0[:FAR_ROWS].to(dtype).double(),
                               tr0.to(dtype).double()).pow(2)
        assert bool((t.argmax(dim=1) >= SEG).all()), "nearest row not in block 1"
        gap = t[:, SEG:].max(dim=1).values - t[:, :SEG].max(dim=1).values
        assert float(gap.min()) >= 100.0, f"block 0 only {float(gap.min())} further"
    return dict(k=k, train=[tr0, _norm_rows(rng, 64, k)],
                test=[te0, _norm_rows(rng, 3, k)])


def kde_far_gap(case):
    """(min, max) over the far rows of how much further block 0 is in d2 / 2
    than block 1, on the bf16 values."""
    te = case["test"][0][:FAR_ROWS].bfloat16().double()
    t = -0.5 * torch.cdist(te, case["train"][0].bfloat16().double()).pow(2)
    gap = t[:, SEG:].max(dim=1).values - t[:, :SEG].max(dim=1).values
    return float(gap.min()), float(gap.max())


def kde_padded_layout(case, dtype):
    """Class-sorted padded test matrix, concatenated train matrix and the
    segment tables of a case, values rounded to `dtype`."""
    rows = [t.shape[0] for t in case["test"]]
    tseg = padded_tseg(rows)
    nseg = [0] + list(np.cumsum([t.shape[0] for t in case["train"]]))
    padded = torch.zeros(tseg[-1], case["k"], dtype=dtype)
    for c, t in enumerate(case["test"]):
        padded[tseg[c]:tseg[c] + t.shape[0]] = t.to(dtype)
    train = torch.cat(case["train"]).to(dtype).contiguous()
    return padded, train, tseg, [int(v) for v in nseg]


# ---------------------------------------------------------------------------
# GPU tests
# ---------------------------------------------------------------------------


@pytest.fixture(scope="module")
def ext():
    from simple_tip_amd.ops import _load_compiled

    return _load_compiled()


def _i32(values):
    return torch.tensor([int(v) for v in values], dtype=torch.int32,
                        device="cuda")


def _nan(*shape):
    return torch.full(shape, float("nan"), device="cuda")


def _prefilled_bf16(rows, cols):
    w = torch.empty(rows, cols, dtype=torch.bfloat16, device="cuda")
    w.view(torch.int16).fill_(NAN_BITS)
    return w


def _norms_bf16(ext, x):
    out = torch.empty(x.shape[0], device="cuda")
    ext.rownorm_bf16_out(x, out)
    return out


# ---- 1. whiten ------------------------------------------------------------


@pytest.mark.parametrize("d", WHITEN_WIDTHS_NT4 + WHITEN_WIDTHS_NT20)
def test_whiten_against_float64(ext, d):
    h = whiten_inputs(d)
    c = len(WHITEN_TEST_ROWS)
    pred, ats = h["pred"].cuda(), h["ats"].cuda()
    b = pred.shape[0]
    assert b == 211
    tseg, rowmap, dest = ext.segment_plan(pred, c)
    assert tseg.tolist() == padded_tseg(WHITEN_TEST_ROWS) == [0, 256, 384, 384, 512, 640]
    placed = rowmap[rowmap >= 0].long()
    assert placed.numel() == sum(WHITEN_TEST_ROWS)
    bp = ext.segment_plan_rows(b, c)
    assert rowmap.numel() == bp and bp > tseg.tolist()[-1]
    keep = h["keep"].cuda()
    assert int(keep.min()) == 0 and int(keep.max()) == ats.shape[1] - 1
    assert bool((keep[:, 1:] > keep[:, :-1]).all())
    white = _prefilled_bf16(bp, d)
    ext.grouped_whiten_bf16(ats, rowmap, tseg, h["wseg"].cuda(), keep,
                            h["wt"].cuda(), white)
    torch.cuda.synchronize()
    worst = whiten_check(ats, rowmap, tseg, h["wseg"], keep, h["wt"], white,
                         prefill_bits=NAN_BITS)
    print(f"[whiten d={d} NT={'4' if (d + 15) // 16 * 16 <= 64 else '20'}] "
          f"worst |got - ref| / (E' + 2^-8 (|ref| + E')) = {worst:.4f}")
    assert worst <= 1.0  # implied by the interval; the interval is the test


# ---- 2. row norms ---------------------------------------------------------


ROWNORM_KS = [1, 7, 8, 9, 40, 300, 512, 520]
ROWNORM_ROWS = 9


def _rownorm_rows(k):
    x = np.random.RandomState(3000 + k).randn(ROWNORM_ROWS, k)
    return torch.from_numpy(x.astype(np.float32)).bfloat16().cuda()


@pytest.mark.parametrize("k", ROWNORM_KS)
def test_rownorm_bf16_against_float64(ext, k):
    x = _rownorm_rows(k)
    out = _nan(ROWNORM_ROWS)
    ext.rownorm_bf16_out(x, out)
    worst = rownorm_check(x, out)
    print(f"[rownorm K={k} chain n={rownorm_chain(k)}] worst ratio {worst:.4f}")


@pytest.mark.parametrize("k", ROWNORM_KS)
@pytest.mark.parametrize("limit", [0, 5, ROWNORM_ROWS])
def test_rownorm_bf16_limit(ext, k, limit):
    x = _rownorm_rows(k)
    out = _nan(ROWNORM_ROWS)
    # the limit is the LAST entry of tseg; the others must not matter
    ext.rownorm_bf16_out(x, out, _i32([ROWNORM_ROWS, 0, limit]))
    assert bool(torch.isnan(out[limit:]).all())
    assert out[limit:].numel() == ROWNORM_ROWS - limit
    full = _nan(ROWNORM_ROWS)
    ext.rownorm_bf16_out(x, full)
    assert torch.equal(out[:limit], full[:limit])
    rownorm_check(x[:limit], out[:limit])


# ---- 3. KDE ---------------------------------------------------------------


def _run_flat(ext, case):
    """ext.kde_logsumexp per class on the fp32 values; worst ratio."""
    worst = 0.0
    for te, tr in zip(case["test"], case["train"]):
        te, tr = te.cuda().contiguous(), tr.cuda().contiguous()
        lse = ext.kde_logsumexp(te, tr)
        worst = max(worst, kde_check(
            te, tr, ext.rownorm(te), ext.rownorm(tr),
            [0, te.shape[0]], [0, tr.shape[0]], lse,
            exact=case.get("exact", False)))
    return worst


def _run_padded_bf16(ext, case):
    padded, train, tseg, nseg = kde_padded_layout(case, torch.bfloat16)
    padded, train = padded.cuda(), train.cuda()
    an, bn = _norms_bf16(ext, padded), _norms_bf16(ext, train)
    jb_max = max((b - a + SEG - 1) // SEG for a, b in zip(nseg, nseg[1:]))
    lse = ext.grouped_kde_bf16(padded, train, _i32(tseg), _i32(nseg), an, bn,
                               jb_max)
    return kde_check(padded, train, an, bn, tseg, nseg, lse,
                     exact=case.get("exact", False))


def _plan_workspace(ext, case, seed):
    """Source rows of a case shuffled behind a segment plan (with the four
    out-of-range predictions), scattered into a NaN-prefilled padded `white`
    whose pad rows are zeroed as the whiten kernel leaves them."""
    rows = [t.shape[0] for t in case["test"]]
    c = len(rows)
    oor = [-1, c, 100000, -5]
    pred = shuffled_pred(rows, seed, oor)
    b = pred.shape[0]
    src = torch.zeros(b, case["k"])
    for cls, t in enumerate(case["test"]):
        src[pred == cls] = t
    pred, src = pred.cuda(), src.bfloat16().cuda()
    tseg, rowmap, dest = ext.segment_plan(pred, c)
    assert tseg.tolist() == padded_tseg(rows)
    bp = ext.segment_plan_rows(b, c)
    white = _prefilled_bf16(bp, case["k"])
    white[: tseg.tolist()[-1]] = 0
    ok = dest >= 0
    assert int((~ok).sum()) == len(oor)
    white[dest[ok].long()] = src[ok]
    wan = _nan(bp)
    ext.rownorm_bf16_out(white, wan, tseg)
    train = torch.cat(case["train"]).bfloat16().cuda().contiguous()
    nseg = [0] + [int(v) for v in np.cumsum([t.shape[0] for t in case["train"]])]
    jb_max = max((hi - lo + SEG - 1) // SEG for lo, hi in zip(nseg, nseg[1:]))
    return dict(b=b, c=c, bp=bp, pred=pred, tseg=tseg, rowmap=rowmap, dest=dest,
                ok=ok, white=white, wan=wan, train=train,
                bn=_norms_bf16(ext, train), nseg=_i32(nseg), jb_max=jb_max)


def _run_plan(ext, case, cls_fused=None, cls_const=None, seed=5):
    p = _plan_workspace(ext, case, seed)
    c = p["c"]
    fused = _i32(cls_fused if cls_fused is not None else [1] * c)
    const = torch.tensor(cls_const if cls_const is not None else [0.0] * c,
                         dtype=torch.float32, device="cuda")
    sentinel = -12345.0
    out = torch.full((p["b"],), sentinel, device="cuda")
    pkde = _nan(p["jb_max"], p["bp"], 2)
    ext.grouped_kde_plan(p["white"], p["train"], p["tseg"], p["nseg"],
                         p["rowmap"], p["wan"], p["bn"], fused, const,
                         p["jb_max"], pkde, out)
    torch.cuda.synchronize()
    worst = lsa_score_check(p["white"], p["wan"], p["train"], p["bn"],
                            p["tseg"], p["nseg"], p["rowmap"], fused, const,
                            out, sentinel, exact=case.get("exact", False))
    return worst, p, out, fused, const


ENTRIES = {"flat_fp32": _run_flat, "padded_bf16": _run_padded_bf16,
           "plan_bf16": lambda ext, case: _run_plan(ext, case)[0]}


@pytest.mark.parametrize("entry", list(ENTRIES))
@pytest.mark.parametrize("duplicate", [False, True])
def test_kde_exact_arithmetic(ext, entry, duplicate):
    """E = 0 by construction: only R is under test."""
    worst = ENTRIES[entry](ext, kde_case_exact(duplicate))
    print(f"[kde exact dup={int(duplicate)} {entry}] worst ratio {worst:.4f}")


@pytest.mark.parametrize("entry,k", [
    ("flat_fp32", 1), ("flat_fp32", 8), ("flat_fp32", 37), ("flat_fp32", 40),
    ("flat_fp32", 300),
    ("padded_bf16", 8), ("padded_bf16", 37), ("padded_bf16", 40),
    ("padded_bf16", 300),
    ("plan_bf16", 8), ("plan_bf16", 37), ("plan_bf16", 40), ("plan_bf16", 300),
])
def test_kde_planted_neighbour(ext, entry, k):
    worst = ENTRIES[entry](ext, kde_case_planted(k))
    print(f"[kde planted K={k} {entry}] worst ratio {worst:.4f}")


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_kde_far_rows(ext, entry):
    """kde_check also asserts every lse finite and above -FLT_MAX."""
    case = kde_case_far()
    worst = ENTRIES[entry](ext, case)
    lo, hi = kde_far_gap(case)
    print(f"[kde far rows {entry}] worst ratio {worst:.4f} "
          f"(block 0 further by {lo:.0f} .. {hi:.0f} in d2/2)")


def test_kde_final_kernel(ext):
    """-(lse + const) bit for bit from the padded call's lse on the same
    workspace, const classes, untouched unplaced rows."""
    consts = [0.5, float("inf"), 0.0, -1.25, 2.0]
    fused_l = [1, 0, 1, 1, 0]
    worst, p, out, fused, const = _run_plan(
        ext, kde_case_planted(40), fused_l, consts, seed=9)
    print(f"[kde final kernel] worst score ratio {worst:.4f}")
    lse = ext.grouped_kde_bf16(p["white"], p["train"], p["tseg"], p["nseg"],
                               p["wan"], p["bn"], p["jb_max"])
    pred, ok, dest = p["pred"], p["ok"], p["dest"].long()
    assert bool((out[~ok] == -12345.0).all())
    for cls in range(p["c"]):
        rows = torch.nonzero(pred == cls, as_tuple=True)[0]
        assert rows.numel() > 0
        if fused_l[cls]:
            want = -(lse[dest[rows]] + const[cls])
            assert want.dtype == torch.float32
            assert torch.equal(out[rows], want)
        else:
            assert bool((out[rows] == consts[cls]).all())
