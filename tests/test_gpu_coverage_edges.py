"""coverage.hip, cam.hip and scores.hip at their edges.

tests/test_gpu_ops.py gives these kernels one Gaussian input and one shape
each: no ties, no value on a boundary, no special value, one code path. The
tests here put activations exactly on (and one float either side of) every
comparison the kernels make, tie the values they rank, and pick the shapes
at which the kernels change path.

Every oracle is ops/fallback.py, a stable sort written out here, or float64.
The GPU tests carry the ``gpu`` marker one by one; the unmarked tests at the
end check the oracles and the inputs themselves and run without a GPU.
"""

import functools

import numpy as np
import pytest
import torch

from simple_tip_amd.ops import fallback

gpu = pytest.mark.gpu

NAN = float("nan")
INF = float("inf")


@pytest.fixture(scope="module")
def ext():
    from simple_tip_amd.ops import hip_ops

    return hip_ops


def _f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


def _below(a):
    return np.nextafter(a, np.float32(-np.inf), dtype=np.float32)


def _above(a):
    return np.nextafter(a, np.float32(np.inf), dtype=np.float32)


# ---------------------------------------------------------------------------
# KMNC section boundaries
# ---------------------------------------------------------------------------

KMNC_K = 130  # K*S never fills the last word for the sections below
KMNC_SECTIONS = [2, 3, 5, 10, 1000]


def _kmnc_tested_boundaries(sections):
    if sections <= 10:
        return list(range(sections + 1))
    return [0, 1, 2, 3, 7, 500, 999, 1000]


@functools.lru_cache(maxsize=None)
def _kmnc_bounds():
    rng = np.random.RandomState(100)
    mins = rng.randn(KMNC_K).astype(np.float32)
    mins[mins == 0] = np.float32(0.5)
    maxs = (mins + np.abs(rng.randn(KMNC_K)).astype(np.float32) + np.float32(0.1))
    maxs = maxs.astype(np.float32)
    maxs[7] = mins[7]  # a constant neuron: every section is empty
    return _f32(mins), _f32(maxs)


def _kmnc_oracle_boundary(mins, maxs, sections, s):
    """Boundary s exactly as fallback.kmnc_profile forms it (two roundings)."""
    jumps = (maxs - mins) / sections
    return mins + jumps * s


def _kmnc_fused_boundary(mins, maxs, sections, s):
    """The same boundary with the product and the sum rounded once: what a
    contracted ``v_fma_f32`` returns."""
    jumps = (maxs - mins) / sections
    return (mins.double() + jumps.double() * s).float()


def _kmnc_fused_differs(sections, boundaries):
    mins, maxs = _kmnc_bounds()
    return sum(
        int(
            (
                _kmnc_oracle_boundary(mins, maxs, sections, s)
                != _kmnc_fused_boundary(mins, maxs, sections, s)
            ).sum()
        )
        for s in boundaries
    )


@functools.lru_cache(maxsize=None)
def _kmnc_case(sections):
    """(acts, mins, maxs, want words, index of the all-NaN row)."""
    mins, maxs = _kmnc_bounds()
    rng = np.random.RandomState(101 + sections)
    rows = []
    for s in _kmnc_tested_boundaries(sections):
        b = _kmnc_oracle_boundary(mins, maxs, sections, s).numpy()
        rows += [b, _below(b), _above(b)]
    lo, hi = mins.numpy(), maxs.numpy()
    rows.append(lo - np.float32(1.0))  # below every section
    rows.append(hi + np.float32(1.0))  # above every section
    rows.append(hi.copy())  # exactly max
    inside = (lo + (hi - lo) * rng.rand(KMNC_K).astype(np.float32)).astype(np.float32)
    rows.append(inside)
    mixed = inside.copy()
    mixed[[0, 3, 64, 129]] = NAN  # NaN beside ordinary neighbours
    rows.append(mixed)
    nan_row = len(rows)
    rows.append(np.full(KMNC_K, NAN, dtype=np.float32))
    acts = _f32(np.stack(rows))
    want = fallback.kmnc_profile(acts, mins, maxs, sections)
    return acts, mins, maxs, want, nan_row


# sections 2 and 3 check the layout only: jump*1 and jump*2 are exact, so
# no interior boundary can differ between the fused and the separately
# rounded form there (with 3 sections the upper end, jump*3, still can).
@gpu
@pytest.mark.parametrize("sections", KMNC_SECTIONS)
def test_kmnc_on_section_boundaries(ext, sections):
    acts, mins, maxs, want, nan_row = _kmnc_case(sections)
    got = ext.kmnc_profile(acts.cuda(), mins.cuda(), maxs.cuda(), sections).cpu()
    assert not want[nan_row].any()  # a NaN activation sets no bit
    diff = got != want
    print(
        f"kmnc sections={sections}: rows={acts.shape[0]} "
        f"words differing={int(diff.sum())} rows differing={int(diff.any(dim=1).sum())}"
    )
    assert torch.equal(got, want)


# ---------------------------------------------------------------------------
# NAC / SNAC / NBC / pack / popcount
# ---------------------------------------------------------------------------

SMALL_ROWS = [1, 5]  # below one block of 4 waves, and just past it
SMALL_K = [1, 63, 64, 65]


def _edge_acts(rows, k, e1, e2, seed):
    """[rows, k] activations built around two per-column edge values.

    Row 0 cycles e1, e2, NaN, random over the columns. With five rows the
    others are: all e1, all e2, one float off e1 (below on even columns,
    above on odd ones), one float off e2 (the other way round)."""
    rng = np.random.RandomState(seed)
    rnd = rng.randn(rows, k).astype(np.float32)
    acts = rnd.copy()
    col = np.arange(k)
    acts[0] = np.where(col % 4 == 0, e1, acts[0])
    acts[0] = np.where(col % 4 == 1, e2, acts[0])
    acts[0] = np.where(col % 4 == 2, np.float32(NAN), acts[0])
    if rows >= 5:
        acts[1] = e1
        acts[2] = e2
        acts[3] = np.where(col % 2 == 0, _below(e1), _above(e1))
        acts[4] = np.where(col % 2 == 0, _above(e2), _below(e2))
    return _f32(acts)


def _bounds(k, seed):
    rng = np.random.RandomState(seed)
    hi = rng.randn(k).astype(np.float32)
    lo = (hi - np.abs(rng.randn(k)).astype(np.float32) - np.float32(0.1)).astype(np.float32)
    return lo, hi


@gpu
@pytest.mark.parametrize("k", SMALL_K)
@pytest.mark.parametrize("rows", SMALL_ROWS)
@pytest.mark.parametrize("thr", [0.25, 0.3])  # 0.3 is no float32: pins the cast
def test_nac_at_threshold(ext, rows, k, thr):
    t = np.full(k, thr, dtype=np.float32)
    acts = _edge_acts(rows, k, t, _above(t), 200 + k)
    got = ext.nac_profile(acts.cuda(), thr).cpu()
    assert torch.equal(got, fallback.nac_profile(acts, thr))


@gpu
@pytest.mark.parametrize("k", SMALL_K)
@pytest.mark.parametrize("rows", SMALL_ROWS)
def test_snac_at_bound(ext, rows, k):
    _, hi = _bounds(k, 210 + k)
    acts = _edge_acts(rows, k, hi, _below(hi), 220 + k)
    got = ext.snac_profile(acts.cuda(), _f32(hi).cuda()).cpu()
    assert torch.equal(got, fallback.snac_profile(acts, _f32(hi)))


@gpu
@pytest.mark.parametrize("k", SMALL_K)
@pytest.mark.parametrize("rows", SMALL_ROWS)
def test_nbc_at_bounds(ext, rows, k):
    lo, hi = _bounds(k, 230 + k)
    acts = _edge_acts(rows, k, hi, lo, 240 + k)
    got = ext.nbc_profile(acts.cuda(), _f32(lo).cuda(), _f32(hi).cuda()).cpu()
    assert torch.equal(got, fallback.nbc_profile(acts, _f32(lo), _f32(hi)))


@gpu
@pytest.mark.parametrize("k", SMALL_K)
@pytest.mark.parametrize("rows", SMALL_ROWS)
def test_pack_small_shapes(ext, rows, k):
    bools = torch.from_numpy(np.random.RandomState(250 + k).rand(rows, k) < 0.5)
    bools[-1] = True  # an all-ones row, tail bits included
    words = ext.pack_bits(bools.cuda())
    assert torch.equal(words.cpu(), fallback.pack_bits(bools))
    assert torch.equal(ext.popcount_rows(words).cpu(), bools.sum(dim=1).long())


@gpu
def test_popcount_rows_past_one_wave_of_words(ext):
    # W = 130: lanes 0 and 1 take a third word; all-ones words and sign bits
    rng = np.random.RandomState(260)
    words = rng.randint(0, 2 ** 63, size=(7, 130), dtype=np.int64)
    words[::2] ^= np.int64(-(2 ** 63))
    words[0] = -1
    words[3, 128:] = -1
    words[5] = 0
    words = torch.from_numpy(words)
    got = ext.popcount_rows(words.cuda()).cpu()
    want = fallback.popcount_rows(words)
    assert int(want[0]) == 130 * 64 and int(want[5]) == 0
    assert torch.equal(got, want)


@gpu
def test_fused_popcount_equals_popcount_rows(ext):
    acts, mins, maxs, want, _ = _kmnc_case(5)
    words, scores = ext._ext.profile(
        ext._PROF_KMNC, acts.cuda(), mins.cuda(), maxs.cuda(), 0.0, 5, KMNC_K * 5
    )
    assert torch.equal(scores, ext.popcount_rows(words))
    assert torch.equal(scores.cpu(), fallback.popcount_rows(want))


# ---------------------------------------------------------------------------
# TKNC ordering
# ---------------------------------------------------------------------------

TKNC_LAYERS = [[1], [63], [64], [65], [77, 1000]]


def _tknc_oracle(layers, k):
    """Descending value (NaN greatest), then ascending column."""
    parts = []
    for flat in layers:
        kk = min(k, flat.shape[1])
        idx = torch.sort(flat, dim=1, descending=True, stable=True).indices[:, :kk]
        prof = torch.zeros_like(flat, dtype=torch.bool)
        prof.scatter_(1, idx, True)
        parts.append(prof)
    return fallback.pack_bits(torch.cat(parts, dim=1))


def _tie_rows(k_cols, seed):
    """Finite rows with ties at the top-k cut. Columns past the layer's width
    are dropped, so every layer gets the same number of rows."""
    rng = np.random.RandomState(seed)
    rows = []

    def zeros():
        return np.zeros(k_cols, dtype=np.float32)

    def put(row, cols, value):
        for c in cols:
            if 0 <= c < k_cols:
                row[c] = value
        return row

    rows.append(zeros())
    for c in (0, 63, 64, k_cols - 1):  # one positive value among zeros
        rows.append(put(zeros(), [c], 1.0))
    base = rng.randn(k_cols).astype(np.float32)
    # the top value twice, in neighbouring lanes
    rows.append(put(base.copy(), [3, 4], 5.0))
    rows.append(put(base.copy(), [k_cols - 2, k_cols - 1], 5.0))
    rows.append(put(base.copy(), [62, 63, 64, 65], 5.0))
    # the top value twice and three times in one lane (columns c, c+64, c+128)
    rows.append(put(base.copy(), [0, 64], 5.0))
    rows.append(put(base.copy(), [5, 69], 5.0))
    rows.append(put(base.copy(), [10, 74, 138], 5.0))
    rows.append(put(base.copy(), [901, 965, 837, 773, 709], 5.0))  # five in one lane
    # zeros above negative values: the tie at the cut is among the zeros
    rows.append(put(-np.abs(base) - 1, [2, 40, 66, k_cols - 1], 0.0))
    # -0.0 beside 0.0: equal, so the column decides
    signed = zeros()
    signed[::2] = -0.0
    rows.append(signed)
    rows.append(put(put(-np.abs(base) - 1, [5], 0.0), [2, 70], -0.0))
    rows.append(np.full(k_cols, 2.5, dtype=np.float32))  # all equal, non-zero
    rows.append(base)  # no tie at all
    return _f32(np.stack(rows))


def _nonfinite_rows(k_cols, seed):
    rng = np.random.RandomState(seed)
    base = rng.randn(k_cols).astype(np.float32)
    rows = []

    def put(row, cols, value):
        for c in cols:
            if 0 <= c < k_cols:
                row[c] = value
        return row

    ninf = np.full(k_cols, -INF, dtype=np.float32)
    rows.append(ninf.copy())  # every entry -inf: the lowest columns win
    rows.append(put(ninf.copy(), [k_cols - 1], 0.5))  # fewer finite values than k
    rows.append(put(ninf.copy(), [1, 64], -3.0e38))
    rows.append(put(base.copy(), [0, 7, 63, 64], -INF))
    rows.append(put(base.copy(), [6], NAN))  # NaN ranks greatest
    rows.append(put(base.copy(), [70, 6], NAN))  # two NaNs: by column
    rows.append(put(put(base.copy(), [2], INF), [9], NAN))  # NaN above +inf
    negnan = np.array([0xFFC00000], dtype=np.uint32).view(np.float32)[0]
    rows.append(put(put(base.copy(), [4], negnan), [1], INF))  # sign of NaN ignored
    rows.append(np.full(k_cols, NAN, dtype=np.float32))
    rows.append(put(np.full(k_cols, NAN, dtype=np.float32), [0, 1], 1.0))
    rows.append(put(ninf.copy(), [k_cols - 1], NAN))
    rows.append(put(ninf.copy(), [3, 67], -np.float32(3.4e38)))
    return _f32(np.stack(rows))


@gpu
@pytest.mark.parametrize("k", [1, 2, 3, 4])
@pytest.mark.parametrize("widths", TKNC_LAYERS, ids=lambda w: "x".join(map(str, w)))
def test_tknc_ties_take_the_lowest_column(ext, widths, k):
    layers = [_tie_rows(w, 300 + i) for i, w in enumerate(widths)]
    got = ext.tknc_profile([l.cuda() for l in layers], k).cpu()
    want = _tknc_oracle(layers, k)
    assert torch.equal(fallback.popcount_rows(want), torch.full(
        (layers[0].shape[0],), sum(min(k, w) for w in widths), dtype=torch.long))
    assert torch.equal(got, want)


@gpu
@pytest.mark.parametrize("k", [1, 2, 3, 4])
@pytest.mark.parametrize("widths", TKNC_LAYERS, ids=lambda w: "x".join(map(str, w)))
def test_tknc_orders_inf_and_nan(ext, widths, k):
    layers = [_nonfinite_rows(w, 310 + i) for i, w in enumerate(widths)]
    got = ext.tknc_profile([l.cuda() for l in layers], k).cpu()
    assert torch.equal(got, _tknc_oracle(layers, k))


@gpu
def test_tknc_rejects_k_above_four(ext):
    layer = _tie_rows(65, 320).cuda()
    with pytest.raises(RuntimeError, match="k in"):
        ext.tknc_profile([layer], 5)


# ---------------------------------------------------------------------------
# CAM greedy cover
# ---------------------------------------------------------------------------


def _sparse_words(rng, rows, nbits, density, first_bit=0):
    """[rows, ceil(nbits/64)] uint64 with about density*(nbits-first_bit)
    random bits per row, all in [first_bit, nbits)."""
    w = (nbits + 63) // 64
    words = np.zeros((rows, w), dtype=np.uint64)
    per_row = max(1, int(density * (nbits - first_bit)))
    for r in range(rows):
        pos = rng.randint(first_bit, nbits, size=per_row).astype(np.uint64)
        np.bitwise_or.at(words[r], (pos >> np.uint64(6)).astype(np.int64),
                         np.uint64(1) << (pos & np.uint64(63)))
    return words


def _dup_scores(rng, rows):
    # four distinct values only: the leftover order is decided by stability
    return _f32(rng.randint(0, 4, size=rows))


def _cam_no_tail(rng):
    return _sparse_words(rng, 70, 128, 0.1), 128


def _cam_garbage_tail(rng):
    words = _sparse_words(rng, 70, 100, 0.1)
    garbage = rng.randint(0, 2 ** 28, size=70).astype(np.uint64) << np.uint64(36)
    assert garbage.any()
    words[:, 1] |= garbage  # bits 100..127: not part of the profile
    return words, 100


def _cam_ties_everywhere(rng):
    # 12 patterns tiled over 16384 + 2048 + 5 rows: equal rows sit in other
    # lanes, waves and blocks, and (row, row + 16384) in the same thread
    rows = 16384 + 2048 + 5
    patterns = _sparse_words(rng, 12, 96, 0.3)
    patterns[5] = patterns[2]
    which = (np.arange(rows) % 16384) % 12
    return np.ascontiguousarray(patterns[which]), 96


def _cam_past_lds(rng):
    return _sparse_words(rng, 64, 2049 * 64 - 3, 0.02), 2049 * 64 - 3


def _cam_past_grid(rng):
    # W = 16400 > 64 blocks * 256 threads; the odd rows have bits only in
    # the 16 words past 16384 (drawn denser there, or they would be empty)
    nbits = 16400 * 64 - 17
    words = _sparse_words(rng, 48, nbits, 0.01)
    words[1::2] = _sparse_words(rng, 24, nbits, 0.3, first_bit=16384 * 64)
    assert not words[1::2, :16384].any() and words[1::2, 16384:].any()
    return words, nbits


def _cam_all_zero(rng):
    return np.zeros((300, 4), dtype=np.uint64), 200


def _cam_identical_rows(rng):
    return np.repeat(_sparse_words(rng, 1, 500, 0.2), 100, axis=0), 500


def _cam_single_row(rng):
    return _sparse_words(rng, 1, 70, 0.3), 70


CAM_CASES = {
    "no_tail": _cam_no_tail,
    "garbage_tail": _cam_garbage_tail,
    "ties_everywhere": _cam_ties_everywhere,
    "past_lds_w2049": _cam_past_lds,
    "past_grid_w16400": _cam_past_grid,
    "all_zero": _cam_all_zero,
    "identical_rows": _cam_identical_rows,
    "single_row": _cam_single_row,
}


@functools.lru_cache(maxsize=None)
def _cam_case(name):
    rng = np.random.RandomState(400 + sorted(CAM_CASES).index(name))
    words, nbits = CAM_CASES[name](rng)
    assert words.shape[1] == (nbits + 63) // 64
    words = torch.from_numpy(words.view(np.int64))
    scores = _dup_scores(rng, words.shape[0])
    want = fallback.cam_order(scores, words, nbits)
    return scores, words, nbits, want


@gpu
@pytest.mark.parametrize("name", list(CAM_CASES))
def test_cam_order_edges(ext, name):
    scores, words, nbits, want = _cam_case(name)
    first = ext.cam_order(scores.cuda(), words.cuda(), nbits).cpu()
    second = ext.cam_order(scores.cuda(), words.cuda(), nbits).cpu()
    assert sorted(want.tolist()) == list(range(scores.shape[0]))
    assert torch.equal(first, want)
    assert torch.equal(second, first)


# ---------------------------------------------------------------------------
# Softmax scores
# ---------------------------------------------------------------------------

SCORE_CLASSES = [1, 2, 10, 64]
SCORE_ROWS = 257  # one block of 256 threads and one row more


@functools.lru_cache(maxsize=None)
def _score_probs(c):
    """float32 [257, C]; the row kind cycles with the row index."""
    rng = np.random.RandomState(500 + c)
    logits = rng.randn(SCORE_ROWS, c)

    def softmax(z):
        e = np.exp(z - z.max(axis=1, keepdims=True))
        return e / e.sum(axis=1, keepdims=True)

    # float64 softmax rounded to float32: keeps the denormals of the confident rows
    plain = softmax(logits).astype(np.float32)
    confident = softmax(30.0 * logits).astype(np.float32)
    probs = plain.copy()
    for i in range(SCORE_ROWS):
        kind = i % 6
        if kind == 1:
            probs[i] = confident[i]
        elif kind == 2:  # exact one-hot
            probs[i] = 0
            probs[i, rng.randint(c)] = 1
        elif kind == 3:  # exact uniform
            probs[i] = np.float32(1.0) / np.float32(c)
        elif kind in (4, 5):  # the top value two or three times
            cols = rng.permutation(c)[: kind - 2]
            probs[i, cols] = probs[i].max()
    if c >= 2:
        probs[1, np.argmin(probs[1])] = np.float32(1e-40)  # a denormal for sure
    return _f32(probs)


def _entropy_gini_f64(probs):
    p = probs.double()
    plogp = torch.where(p > 0, p * torch.log(p), torch.zeros_like(p))
    sq = (p * p).sum(dim=1)
    c = probs.shape[1]
    ent_bound = (c + 4) * 2.0 ** -23 * plogp.abs().sum(dim=1) + c * 2.0 ** -149
    gini_bound = (c + 2) * 2.0 ** -24 * sq.clamp_min(1.0)
    return -plogp.sum(dim=1), ent_bound, 1.0 - sq, gini_bound


def _check_scores(got, probs, label):
    """softmax/pcs bit-equal to the fallback; entropy and gini within the
    derived float32 bounds of their float64 values. Returns the largest
    error/bound ratios."""
    want = fallback.softmax_uncertainties(probs)
    for name in ("softmax", "pcs", "softmax_entropy", "deep_gini"):
        assert got[name].shape == (SCORE_ROWS,)
        assert torch.isfinite(got[name]).all(), name
    ent, ent_bound, gini, gini_bound = _entropy_gini_f64(probs)
    ent_err = (got["softmax_entropy"].double() - ent).abs()
    gini_err = (got["deep_gini"].double() - gini).abs()
    ent_ratio = float((ent_err / ent_bound.clamp_min(1e-300)).max())
    gini_ratio = float((gini_err / gini_bound).max())
    print(
        f"scores {label} C={probs.shape[1]}: entropy max err {float(ent_err.max()):.3e} "
        f"(max err/bound {ent_ratio:.3f}), gini max err {float(gini_err.max()):.3e} "
        f"(max err/bound {gini_ratio:.3f})"
    )
    assert torch.equal(got["softmax"], want["softmax"])
    assert torch.equal(got["pcs"], want["pcs"])
    assert (ent_err <= ent_bound).all()
    assert (gini_err <= gini_bound).all()
    return ent_ratio, gini_ratio


@gpu
@pytest.mark.parametrize("c", SCORE_CLASSES)
def test_softmax_scores_edges(ext, c):
    probs = _score_probs(c)
    got = {k: v.cpu() for k, v in ext.softmax_uncertainties(probs.cuda()).items()}
    _check_scores(got, probs, "hip")


# ---------------------------------------------------------------------------
# Without a GPU: the oracles and the inputs themselves
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("sections", KMNC_SECTIONS)
def test_kmnc_inputs_tell_fused_boundaries_apart(sections):
    """Teeth: a kernel that contracts lo + jump*s into one fma moves enough
    boundaries for the rows above to land in another section."""
    interior = range(1, sections)
    n = _kmnc_fused_differs(sections, interior)
    print(f"kmnc sections={sections}: {n} of {KMNC_K * (sections - 1)} interior "
          f"boundaries differ when fused")
    if sections in (2, 3):
        assert n == 0  # jump*1 and jump*2 are exact: layout checks only
    if sections in (5, 10):
        assert n >= 10
    if sections == 1000:
        assert _kmnc_fused_differs(sections, _kmnc_tested_boundaries(sections)) >= 1
    # and the profile of the rows above changes if fused boundaries are used
    acts, mins, maxs, want, _ = _kmnc_case(sections)
    fused = torch.zeros(acts.shape[0], KMNC_K, sections, dtype=torch.bool)
    for s in range(sections):
        lo = _kmnc_fused_boundary(mins, maxs, sections, s)
        hi = _kmnc_fused_boundary(mins, maxs, sections, s + 1)
        fused[..., s] = (lo <= acts) & (acts < hi)
    fused = fallback.pack_bits(fused.reshape(acts.shape[0], -1))
    if sections == 2:
        assert torch.equal(fused, want)
    if sections >= 5:  # (with 3 only the upper end, jump*3, can move)
        assert not torch.equal(fused, want)


@pytest.mark.parametrize("k", [1, 2, 3, 4])
@pytest.mark.parametrize("widths", TKNC_LAYERS, ids=lambda w: "x".join(map(str, w)))
def test_tknc_fallback_ties_take_the_lowest_column(widths, k):
    for build, seed in ((_tie_rows, 300), (_nonfinite_rows, 310)):
        layers = [build(w, seed + i) for i, w in enumerate(widths)]
        assert torch.equal(fallback.tknc_profile(layers, k), _tknc_oracle(layers, k))


def test_tknc_fallback_single_one_among_zeros():
    # torch.topk takes columns [70, 66, 65] here; the rule is [70, 0, 1]
    row = torch.zeros(1, 100)
    row[0, 70] = 1.0
    prof = fallback.unpack_bits(fallback.tknc_profile([row], 3), 100)
    assert prof[0].nonzero().flatten().tolist() == [0, 1, 70]


@pytest.mark.parametrize("c", SCORE_CLASSES)
def test_score_inputs_and_fallback_within_bounds(c):
    probs = _score_probs(c)
    tiny = float(np.finfo(np.float32).tiny)
    if c >= 2:
        assert ((probs > 0) & (probs < tiny)).any()  # denormals present
        top2 = torch.topk(probs, 2, dim=1).values
        assert (top2[:, 0] == top2[:, 1]).any()  # exact ties for the top
    if c >= 10:
        assert (probs == 0).any()  # and underflow to zero
        assert (probs.max(dim=1).values > 1 - 1e-6).any()  # confident rows
    _check_scores(fallback.softmax_uncertainties(probs), probs, "fallback")
