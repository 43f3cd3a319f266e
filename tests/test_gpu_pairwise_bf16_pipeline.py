"""Pipelined bf16 grouped row-min (grouped_rowmin_bf16_pipe_kernel) against
the generic kernel it stands in for, on the compiled extension.

Both kernels run the same MFMA chain per accumulator (k ascending in steps
of 32) and share the epilogue, so every comparison between them is a bit
equality. `ext.rowmin_bf16_force_generic` switches kernels inside one
process; `ext.rowmin_bf16_pipelined_launches` says which one a call took.
"""

import functools
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "rowmin_bf16_parent.npz")

# class c has TEST_ROWS[c] test rows and TRAIN_ROWS[c] train rows: an empty
# train class (+inf), a row in exactly one column, column tails inside a
# tile, several column blocks, an empty test class
TEST_ROWS = [129, 1, 127, 128, 300, 0, 129]
TRAIN_ROWS = [0, 1, 127, 128, 129, 257, 513]
OUT_OF_RANGE = len(TEST_ROWS)  # the prediction of one extra row

# the shipped K-tile and buffer count (test_geometry pins them to the build)
BK, NBUF = 64, 2
# prologue only, one swap, odd parity, a full ring plus one
K_MULTIPLES = sorted({1, 2, 3, NBUF + 1, 2 * NBUF + 1})


@pytest.fixture(scope="module")
def ext():
    from simple_tip_amd.ops import _load_compiled

    e = _load_compiled()
    yield e
    e.rowmin_bf16_force_generic(False)


def _golden_module():
    path = os.path.join(os.path.dirname(HERE), "scripts", "make_rowmin_golden.py")
    spec = importlib.util.spec_from_file_location("make_rowmin_golden", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _case(k, seed=7, test_rows=TEST_ROWS, train_rows=TRAIN_ROWS, extra_pred=()):
    """GPU tensors of one grouped case; rows in shuffled order."""
    dev = torch.device("cuda")
    rng = np.random.RandomState(seed)
    c = len(test_rows)
    pred = rng.permutation(
        np.concatenate([np.repeat(np.arange(c), test_rows), list(extra_pred)])
    ).astype(np.int64)
    b, n = pred.shape[0], sum(train_rows)
    src = torch.from_numpy((rng.randn(b, k) * 0.3).astype(np.float32))
    train = torch.from_numpy((rng.randn(n, k) * 0.3).astype(np.float32))
    btable = torch.from_numpy(rng.rand(n).astype(np.float32) + 0.5)
    nseg = np.concatenate([[0], np.cumsum(train_rows)])
    return dict(
        k=k, c=c, b=b, pred=torch.from_numpy(pred).to(dev),
        src=src.to(torch.bfloat16).to(dev),
        train=train.to(torch.bfloat16).to(dev), btable=btable.to(dev),
        nseg=torch.tensor(nseg, dtype=torch.int32, device=dev),
        jb_max=max(1, (max(train_rows) + 127) // 128),
    )


def _norms(ext, x):
    out = torch.empty(x.shape[0], device=x.device)
    ext.rownorm_bf16_out(x, out)
    return out


def _nan(*shape):
    return torch.full(shape, float("nan"), device="cuda")


def _plan(ext, case, src=None, train=None):
    """Gathered entry point: (dist, idx, dsa) per source row."""
    src = case["src"] if src is None else src
    train = case["train"] if train is None else train
    b, c, jb = case["b"], case["c"], case["jb_max"]
    tseg, rowmap, _ = ext.segment_plan(case["pred"], c)
    bp = ext.segment_plan_rows(b, c)
    pval = _nan(jb, bp)
    pidx = torch.full((jb, bp), -1, dtype=torch.int32, device="cuda")
    dsa, dist = _nan(b), _nan(b)
    idx = torch.full((b,), -7, dtype=torch.int32, device="cuda")
    ext.grouped_rowmin_plan(
        src, train, tseg, case["nseg"], rowmap, _norms(ext, src),
        _norms(ext, train), case["btable"], jb, pval, pidx, dsa, dist, idx,
    )
    return dist, idx, dsa


def _padded(ext, case, src=None, train=None):
    """Padded entry point on the plan's layout: (dist, idx) per padded row,
    and the padded row of every placed source row."""
    src = case["src"] if src is None else src
    train = case["train"] if train is None else train
    tseg, _, dest = ext.segment_plan(case["pred"], case["c"])
    placed = dest >= 0
    rows = int(tseg[-1])
    padded = torch.zeros(rows, case["k"], device="cuda", dtype=torch.bfloat16)
    padded[dest[placed].long()] = src[placed]
    an = torch.zeros(rows, device="cuda")
    an[dest[placed].long()] = _norms(ext, src)[placed]
    dist, idx = ext.grouped_rowmin_bf16(
        padded, train, tseg, case["nseg"], an, _norms(ext, train),
        case["jb_max"],
    )
    return dist, idx, dest


def _on_both(ext, fn, pipelined_calls):
    """fn() on the default dispatch and with the generic kernel forced;
    `pipelined_calls` is how many launches of the first run must have taken
    the pipelined kernel (the forced run: none)."""
    n0 = ext.rowmin_bf16_pipelined_launches()
    got = fn()
    n1 = ext.rowmin_bf16_pipelined_launches()
    ext.rowmin_bf16_force_generic(True)
    try:
        ref = fn()
    finally:
        ext.rowmin_bf16_force_generic(False)
    n2 = ext.rowmin_bf16_pipelined_launches()
    assert n1 - n0 == pipelined_calls, (n0, n1)
    assert n2 == n1
    return got, ref


def _assert_same(got, ref):
    for g, r in zip(got, ref):
        # NaN never appears in a placed row; equal_nan covers unplaced ones
        assert torch.equal(torch.nan_to_num(g.float(), nan=-123.0),
                           torch.nan_to_num(r.float(), nan=-123.0))
        assert g.dtype == r.dtype


# ---- bit equality ----------------------------------------------------------


def test_geometry(ext):
    assert ext.rowmin_bf16_pipeline_bk() == BK
    assert ext.rowmin_bf16_pipeline_nbuf() == NBUF


@pytest.mark.parametrize("mult", K_MULTIPLES)
def test_pipelined_equals_generic(ext, mult):
    """K = BK, 2 BK, 3 BK, (NBUF+1) BK, (2 NBUF+1) BK (duplicates collapse),
    both entry points, every class shape of TEST_ROWS x TRAIN_ROWS."""
    case = _case(mult * BK, extra_pred=[OUT_OF_RANGE])

    got, ref = _on_both(ext, lambda: _plan(ext, case), 1)
    _assert_same(got, ref)
    dist, idx, dsa = got
    pred = case["pred"]
    bad = pred == OUT_OF_RANGE
    assert int(bad.sum()) == 1
    # the out-of-range row is not placed: its outputs keep their pre-fill
    assert bool(torch.isnan(dist[bad]).all()) and int(idx[bad][0]) == -7
    empty = pred == 0  # class 0 has no train rows
    assert bool((dsa[empty] == float("inf")).all())
    assert bool((idx[empty] == -1).all())
    ok = ~bad & ~empty
    assert bool(torch.isfinite(dist[ok]).all())
    lo = case["nseg"][pred[ok]]
    hi = case["nseg"][pred[ok] + 1]
    assert bool(((idx[ok] >= lo) & (idx[ok] < hi)).all())
    assert torch.equal(dsa[ok], dist[ok] / case["btable"][idx[ok].long()])

    gotp, refp = _on_both(ext, lambda: _padded(ext, case), 1)
    _assert_same(gotp[:2], refp[:2])
    dist_p, idx_p, dest = gotp
    placed = dest >= 0
    assert torch.equal(placed, ~bad)
    # gathered == padded on the same rows (the generic kernels' C3 invariant)
    assert torch.equal(dist[ok], dist_p[dest[ok].long()])
    assert torch.equal(idx[ok].long(), idx_p[dest[ok].long()])


def test_determinism(ext):
    case = _case(3 * BK, seed=8)
    first = _plan(ext, case)
    second = _plan(ext, case)
    _assert_same(first, second)


# ---- ties ------------------------------------------------------------------


def test_ties_take_the_lowest_index_and_exact_zero(ext):
    """Train row 5 of the 300-row class is repeated at 9 (same column block)
    and at 200 (another column block); the test row equals it. Its values
    are multiples of 1/2 of magnitude at most 1, so every product and every
    partial sum (norms, the MFMA chain in any order) is exact in fp32: the
    distance is exactly 0, three times, and the lowest index must win."""
    k = 2 * BK
    case = _case(k, seed=9, test_rows=[40, 3], train_rows=[300, 140])
    rng = np.random.RandomState(10)
    row = torch.from_numpy(rng.randint(-2, 3, k).astype(np.float32) / 2)
    row = row.to(torch.bfloat16).cuda()
    train = case["train"].clone()
    base = int(case["nseg"][0])
    for j in (5, 9, 200):
        train[base + j] = row
    src = case["src"].clone()
    target = int(torch.nonzero(case["pred"] == 0)[0])
    src[target] = row

    got, ref = _on_both(ext, lambda: _plan(ext, case, src, train), 1)
    _assert_same(got, ref)
    dist, idx, _ = got
    assert float(dist[target]) == 0.0
    assert int(idx[target]) == base + 5
    gotp, refp = _on_both(ext, lambda: _padded(ext, case, src, train), 1)
    _assert_same(gotp[:2], refp[:2])
    dist_p, idx_p, dest = gotp
    assert float(dist_p[dest[target]]) == 0.0
    assert int(idx_p[dest[target]]) == base + 5


# ---- dispatch boundary -----------------------------------------------------


def _misaligned(t):
    """A copy of bf16 matrix `t` whose storage starts 8 bytes past a 16-byte
    boundary."""
    buf = torch.empty(t.numel() + 4, dtype=t.dtype, device=t.device)
    out = buf[4:].view(t.shape)
    out.copy_(t)
    assert out.data_ptr() % 16 == 8 and out.is_contiguous()
    return out


def test_dispatch_boundary(ext):
    bk = BK
    small = dict(test_rows=[130, 5], train_rows=[140, 60])
    # K = BK: pipelined
    case = _case(bk, seed=11, **small)
    got, ref = _on_both(ext, lambda: _plan(ext, case), 1)
    _assert_same(got, ref)
    # K = BK + 8: generic (no launch counted), same bits as forced generic
    case8 = _case(bk + 8, seed=11, **small)
    got, ref = _on_both(ext, lambda: _plan(ext, case8), 0)
    _assert_same(got, ref)
    got, ref = _on_both(ext, lambda: _padded(ext, case8), 0)
    _assert_same(got[:2], ref[:2])
    # a 16-byte-misaligned operand, either side: generic, and the result is
    # the aligned (pipelined) one
    aligned = _plan(ext, case)
    for src, train in ((_misaligned(case["src"]), None),
                       (None, _misaligned(case["train"]))):
        got, ref = _on_both(ext, lambda: _plan(ext, case, src, train), 0)
        _assert_same(got, ref)
        _assert_same(got, aligned)


# ---- parent golden ---------------------------------------------------------


@functools.lru_cache(maxsize=None)
def _golden_case():
    mod = _golden_module()
    return mod, mod.golden_inputs()


def test_parent_golden(ext):
    """Both kernels reproduce what the commit before the pipelined kernel
    computed (scripts/make_rowmin_golden.py wrote the file on that build)."""
    mod, case = _golden_case()
    want = np.load(GOLDEN)
    got, ref = _on_both(ext, lambda: mod.run_plan(ext, case), 1)
    for name, arrays in (("pipelined", got), ("generic", ref)):
        for key, arr in zip(("dist", "idx", "dsa"), arrays):
            assert np.array_equal(arr, want[key]), (name, key)


# ---- float64 ---------------------------------------------------------------


def test_against_float64(ext):
    """Squared distances against float64 `an + bn - 2 a.b` from the same fp32
    norms, on the golden case (K = 192), so that both kernels cannot be wrong
    together.

    Bound on |dist^2 - ref| per (row, column). Products of two bf16 values
    are exact in fp32. The dot product is K fp32 accumulations in hardware
    order, each off by at most 2^-23 of the running magnitude, which
    sum |a_k b_k| = S bounds: |dot - exact| <= K 2^-23 S, doubled by the
    factor 2. The combination rounds three times (an + bn, the subtraction,
    the square root; 2 * dot is exact): 2^-24 (an + bn) + 2^-24 d for the
    first two, and squaring the rounded root costs 2 * 2^-24 d more. In all
      bound = 2 K 2^-23 S + 2^-24 (an + bn) + 3 * 2^-24 d.
    The row minimum moves by at most the largest bound among the class's
    columns. The arg-min must equal float64's on every row whose best and
    second-best float64 distances are more than two bounds apart; at most
    1 % of the rows may be closer than that."""
    mod, case = _golden_case()
    dist, idx, _ = mod.run_plan(ext, case)
    k = case["src"].shape[1]
    a = case["src"].double().numpy()
    bt = case["train"].double().numpy()
    an = _norms(ext, case["src"].cuda()).cpu().double().numpy()
    bn = _norms(ext, case["train"].cuda()).cpu().double().numpy()
    nseg = case["nseg"].numpy()
    pred = case["pred"].numpy()
    skipped, worst, ratios = 0, 0.0, []
    for c in range(len(nseg) - 1):
        rows = np.nonzero(pred == c)[0]
        lo, hi = int(nseg[c]), int(nseg[c + 1])
        ref = an[rows, None] + bn[None, lo:hi] - 2.0 * a[rows] @ bt[lo:hi].T
        s = np.abs(a[rows]) @ np.abs(bt[lo:hi]).T
        bound = (2.0 * k * 2.0 ** -23 * s
                 + 2.0 ** -24 * (an[rows, None] + bn[None, lo:hi])
                 + 3 * 2.0 ** -24 * np.abs(ref)).max(axis=1)
        best = ref.min(axis=1)
        err = np.abs(dist[rows].astype(np.float64) ** 2 - best)
        worst = max(worst, float((err / bound).max()))
        ratios.append(bound / best)
        assert (err <= bound).all(), (c, float((err / bound).max()))
        two = np.partition(ref, 1, axis=1)[:, :2]
        clear = (two[:, 1] - two[:, 0]) > 2.0 * bound
        skipped += int((~clear).sum())
        assert np.array_equal(idx[rows][clear], lo + ref.argmin(axis=1)[clear])
    ratios = np.concatenate(ratios)
    print(f"float64: worst err/bound {worst:.3f}; bound / distance median "
          f"{np.median(ratios):.2e}, max {ratios.max():.2e}; near-tie rows "
          f"skipped {skipped} of {pred.shape[0]}")
    assert skipped <= 0.01 * pred.shape[0]


# ---- serving ---------------------------------------------------------------


def test_serving_fast_call_equals_forced_generic(ext):
    """A FusedPrioritizer fast call at D = 128 takes the pipelined kernel and
    scores `dsa` and `pc-lsa` exactly as with the generic kernel forced."""
    from simple_tip_amd.core.surprise import DSA, LSA, MultiModalSA
    from simple_tip_amd.engine.serving import FusedPrioritizer

    dev = torch.device("cuda:0")
    rng = np.random.RandomState(12)
    ats = torch.from_numpy(rng.randn(1500, 128).astype(np.float32))
    pred = torch.from_numpy(rng.randint(0, 5, 1500))
    dsa = DSA(ats, pred, device=dev)
    lsa = MultiModalSA.build_by_class(
        ats, pred, lambda a, p: LSA(a, max_features=32, device=dev)
    )
    fast = FusedPrioritizer(dsa, lsa, dev, pairwise_dtype=torch.bfloat16)
    assert fast.fast and fast.lsa_ready
    test = torch.from_numpy(rng.randn(401, 128).astype(np.float32)).to(dev)
    tp = torch.from_numpy(rng.randint(0, 5, 401)).to(dev)

    def call():
        out = fast(test, tp)
        torch.cuda.synchronize()
        return out[0].clone(), out[1].clone()

    (d_new, l_new), (d_gen, l_gen) = _on_both(ext, call, 1)
    assert bool(torch.isfinite(d_new).all())
    assert torch.equal(d_new, d_gen)
    assert torch.equal(l_new, l_gen)
