"""cam_many.hip on the GPU: one persistent launch orders several CAM problems,
one team of blocks each.

The oracle is ``fallback.cam_order`` on the CPU throughout, computed once per
problem. The shapes are the ones at which the kernel takes another path: the
edge shapes of the single-problem kernel side by side (so ties cross lanes,
waves, blocks and teams), more problems than one launch takes, one long
problem beside many that finish at once (teams exit while others run), and
widths and densities on both sides of the kernel's two switches, which are
imported from the extension.
"""

import functools

import numpy as np
import pytest
import torch

from simple_tip_amd.ops import fallback

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ext():
    from simple_tip_amd.ops import hip_ops

    return hip_ops


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


def _no_tail(rng):
    return _sparse_words(rng, 70, 128, 0.1), 128


def _garbage_tail(rng):
    words = _sparse_words(rng, 70, 100, 0.1)
    garbage = rng.randint(1, 2 ** 28, size=70).astype(np.uint64) << np.uint64(36)
    words[:, 1] |= garbage  # bits 100..127: not part of the profile
    return words, 100


def _ties_everywhere(rng):
    # 12 patterns tiled over 16384 + 2048 + 5 rows: equal rows sit in other
    # lanes, waves, blocks and teams
    rows = 16384 + 2048 + 5
    patterns = _sparse_words(rng, 12, 96, 0.3)
    patterns[5] = patterns[2]
    which = (np.arange(rows) % 16384) % 12
    return np.ascontiguousarray(patterns[which]), 96


def _past_lds(rng):
    return _sparse_words(rng, 64, 2049 * 64 - 3, 0.02), 2049 * 64 - 3


def _past_grid(rng):
    # W = 16400; the odd rows have bits only in the 16 words past 16384
    nbits = 16400 * 64 - 17
    words = _sparse_words(rng, 48, nbits, 0.01)
    words[1::2] = _sparse_words(rng, 24, nbits, 0.3, first_bit=16384 * 64)
    assert not words[1::2, :16384].any() and words[1::2, 16384:].any()
    return words, nbits


def _all_zero(rng):
    return np.zeros((300, 4), dtype=np.uint64), 200


def _identical_rows(rng):
    return np.repeat(_sparse_words(rng, 1, 500, 0.2), 100, axis=0), 500


def _single_row(rng):
    return _sparse_words(rng, 1, 70, 0.3), 70


EDGE_CASES = [
    _no_tail, _garbage_tail, _ties_everywhere, _past_lds, _past_grid,
    _all_zero, _identical_rows, _single_row,
]


def _finish(rng, words, nbits):
    """(scores, int64 words, nbits, oracle order); four score values only, so
    the leftover order is decided by stability."""
    assert words.shape[1] == (nbits + 63) // 64
    words = torch.from_numpy(np.ascontiguousarray(words).view(np.int64))
    scores = torch.from_numpy(rng.randint(0, 4, size=words.shape[0]).astype(np.float32))
    want = fallback.cam_order(scores, words, nbits)
    assert sorted(want.tolist()) == list(range(scores.shape[0]))
    return scores, words, nbits, want


@functools.lru_cache(maxsize=None)
def _edge_batch():
    out = []
    for i, build in enumerate(EDGE_CASES):
        rng = np.random.RandomState(1300 + i)
        out.append(_finish(rng, *build(rng)))
    return out


def _run(ext, problems):
    """cam_order_many of (scores, words, nbits, ...) tuples, back on the CPU."""
    got = ext.cam_order_many(
        [p[0].cuda() for p in problems],
        [p[1].cuda() for p in problems],
        [p[2] for p in problems],
    )
    assert len(got) == len(problems)
    assert all(g.is_cuda and g.dtype == torch.int64 for g in got)
    return [g.cpu() for g in got]


def test_edge_batch(ext):
    batch = _edge_batch()
    first = _run(ext, batch)
    second = _run(ext, batch)
    for i, (p, a, b) in enumerate(zip(batch, first, second)):
        assert torch.equal(a, p[3]), EDGE_CASES[i].__name__
        assert torch.equal(b, a), EDGE_CASES[i].__name__


def test_batch_independence(ext):
    batch = _edge_batch()
    target = batch[3]
    alone = _run(ext, [target])[0]
    first_of_two = _run(ext, [target, batch[0]])[0]
    last_of_eight = _run(ext, batch[:3] + batch[4:] + [target])[-1]
    reversed_ = _run(ext, batch[::-1])[len(batch) - 1 - 3]
    assert torch.equal(alone, target[3])
    for other in (first_of_two, last_of_eight, reversed_):
        assert torch.equal(other, alone)
    # P == 1 is the single-problem kernel's answer, for every edge shape
    for p in batch:
        single = ext.cam_order(p[0].cuda(), p[1].cuda(), p[2]).cpu()
        assert torch.equal(_run(ext, [p])[0], single)


def test_chunking_past_one_launch(ext):
    cap = ext.cam_many_max_problems()
    assert cap == 32
    problems = []
    for i in range(cap + 1):
        rng = np.random.RandomState(1400 + i)
        problems.append(_finish(rng, _sparse_words(rng, 64, 130, 0.1), 130))
    got = _run(ext, problems)
    for i, (p, g) in enumerate(zip(problems, got)):
        assert torch.equal(g, p[3]), i
    # the orders differ between the problems: a mix-up would show
    assert len({tuple(g.tolist()) for g in got}) > cap // 2


def test_empty_problems_inside_a_batch(ext):
    rng = np.random.RandomState(1450)
    real = _finish(rng, _sparse_words(rng, 64, 130, 0.1), 130)
    none = (torch.zeros(0), torch.zeros(0, 3, dtype=torch.int64), 130)
    got = _run(ext, [none, real, none])
    assert got[0].numel() == 0 and got[2].numel() == 0
    assert torch.equal(got[1], real[3])
    assert ext.cam_order_many([], [], []) == []


@functools.lru_cache(maxsize=None)
def _uneven_batch():
    rng = np.random.RandomState(1500)
    big = _finish(rng, _sparse_words(rng, 4096, 2560, 0.02), 2560)
    small = []
    for i in range(16):
        r = np.random.RandomState(1501 + i)
        small.append(_finish(r, _sparse_words(r, 8, 70, 0.2), 70))
    return [big] + small


def _pick_count(problem):
    """Rows of the oracle order that added coverage."""
    _, words, nbits, want = problem
    w = words.numpy().view(np.uint64)
    unc = np.full(w.shape[1], ~np.uint64(0), dtype=np.uint64)
    if nbits % 64:
        unc[-1] = np.uint64((1 << (nbits % 64)) - 1)
    n = 0
    for row in want.tolist():
        newly = w[row] & unc
        if not newly.any():
            break
        unc &= ~newly
        n += 1
    return n


def test_uneven_teams(ext):
    """One team runs for over a hundred picks while sixteen single-block teams
    finish after a handful and exit."""
    batch = _uneven_batch()
    assert _pick_count(batch[0]) >= 100
    assert all(_pick_count(p) <= 8 for p in batch[1:])
    # the long problem has a team of several blocks, the others one block
    plan = ext.cam_many_plan(
        [p[1].shape[0] for p in batch], [p[1].shape[1] for p in batch], 256
    )
    assert plan[0] > 1 and set(plan[1:]) == {1}
    for _ in range(2):
        got = _run(ext, batch)
        for i, (p, g) in enumerate(zip(batch, got)):
            assert torch.equal(g, p[3]), i
    # the long problem last: its team starts past the finished ones
    got = _run(ext, batch[1:] + batch[:1])
    assert torch.equal(got[-1], batch[0][3])


def _list_lengths(problem):
    """Non-zero words of ``newly`` for every pick of the oracle order."""
    _, words, nbits, want = problem
    w = words.numpy().view(np.uint64)
    unc = np.full(w.shape[1], ~np.uint64(0), dtype=np.uint64)
    if nbits % 64:
        unc[-1] = np.uint64((1 << (nbits % 64)) - 1)
    lengths = []
    for row in want.tolist():
        newly = w[row] & unc
        if not newly.any():
            break
        unc &= ~newly
        lengths.append(int(np.count_nonzero(newly)))
    return lengths


@functools.lru_cache(maxsize=None)
def _form_batch(wide_words):
    """The same bits at a width one word below the wave-per-row threshold
    and, padded with empty words, one word above it.

    Three rows of density 0.3 come first in the greedy order and change every
    word (long lists: full re-sweeps). Then rows with many bits in two
    adjacent words (short lists: the incremental update) alternate with rows
    of 30 bits spread over the width (lists around the switch), and rows of
    three bits make the long sparse tail."""
    rng = np.random.RandomState(1600)
    narrow_w = wide_words - 1
    nbits = narrow_w * 64 - 5
    dense = _sparse_words(rng, 3, nbits, 0.3)
    clustered = np.zeros((40, narrow_w), dtype=np.uint64)
    for r in range(40):
        w0 = rng.randint(0, narrow_w - 2)
        clustered[r, w0:w0 + 2] = _sparse_words(rng, 1, 128, 0.5)[0]
    spread = _sparse_words(rng, 200, nbits, 30 / nbits)
    sparse = _sparse_words(rng, 357, nbits, 3 / nbits)
    base = np.concatenate([dense, clustered, spread, sparse])
    base = base[rng.permutation(base.shape[0])]
    padded = np.zeros((base.shape[0], wide_words + 1), dtype=np.uint64)
    padded[:, :narrow_w] = base
    # one bit in the very last word, or the padding would be dead weight
    padded[7, -1] = np.uint64(1) << np.uint64(40)
    narrow = _finish(np.random.RandomState(1601), base, nbits)
    wide = _finish(np.random.RandomState(1601), padded, (wide_words + 1) * 64 - 9)
    return narrow, wide


def test_both_sweep_forms_and_both_update_forms(ext):
    wide_words = ext.CAM_MANY_WIDE_WORDS  # cam_many.h: CAM_MANY_WIDE_WORDS = 64
    incr_div = ext.CAM_MANY_INCR_DIV      # cam_many.h: CAM_MANY_INCR_DIV = 8
    assert (wide_words, incr_div, ext.CAM_MANY_LIST_CAP) == (64, 8, 1024)
    narrow, wide = _form_batch(wide_words)
    assert narrow[1].shape[1] == wide_words - 1  # a thread per row
    assert wide[1].shape[1] == wide_words + 1    # a wave per row
    for p in (narrow, wide):
        w = p[1].shape[1]
        lengths = _list_lengths(p)
        assert len(lengths) >= 200
        full = [n * incr_div > w for n in lengths]
        # both update forms run, the switch is crossed in both directions,
        # and lists sit exactly on either side of it
        assert sum(full) >= 20 and len(full) - sum(full) >= 100
        assert sum(a and not b for a, b in zip(full, full[1:])) >= 5
        assert sum(b and not a for a, b in zip(full, full[1:])) >= 5
        assert w // incr_div in lengths and w // incr_div + 1 in lengths
        assert max(lengths) >= wide_words - 1  # the dense early phase
    got = _run(ext, [narrow, wide])
    assert torch.equal(got[0], narrow[3])
    assert torch.equal(got[1], wide[3])
    # and each alone, where its team is larger
    assert torch.equal(_run(ext, [narrow])[0], narrow[3])
    assert torch.equal(_run(ext, [wide])[0], wide[3])


@functools.lru_cache(maxsize=None)
def _list_cap_problem():
    # W = 16400: rows of 1500 bits have lists between CAM_MANY_LIST_CAP and
    # W / CAM_MANY_INCR_DIV, rows of 200 bits lists below both
    rng = np.random.RandomState(1650)
    nbits = 16400 * 64 - 17
    words = _sparse_words(rng, 40, nbits, 200 / nbits)
    words[::2] = _sparse_words(rng, 20, nbits, 1500 / nbits)
    return _finish(rng, words, nbits)


def test_list_cap_on_a_very_wide_profile(ext):
    """Where W / CAM_MANY_INCR_DIV exceeds CAM_MANY_LIST_CAP, a list between
    the two does not fit and must fall back to a full sweep."""
    p = _list_cap_problem()
    w = p[1].shape[1]
    cap = ext.CAM_MANY_LIST_CAP
    assert w // ext.CAM_MANY_INCR_DIV > cap
    lengths = _list_lengths(p)
    assert sum(cap < n <= w // ext.CAM_MANY_INCR_DIV for n in lengths) >= 10
    assert sum(n <= cap for n in lengths) >= 10
    assert torch.equal(_run(ext, [p])[0], p[3])
    assert torch.equal(_run(ext, [p, _edge_batch()[0]])[0], p[3])


def test_error_contract(ext):
    rng = np.random.RandomState(1700)
    s, w, nbits, _ = _finish(rng, _sparse_words(rng, 16, 130, 0.1), 130)
    sc, wc = s.cuda(), w.cuda()
    with pytest.raises(ValueError, match="device"):
        ext.cam_order_many([sc, s], [wc, w], [nbits, nbits])
    with pytest.raises(ValueError, match="contiguous int64"):
        ext.cam_order_many([sc], [wc.t().contiguous().t()], [nbits])
    with pytest.raises(ValueError, match="contiguous int64"):
        ext.cam_order_many([sc], [wc.int()], [nbits])
    with pytest.raises(ValueError, match="contiguous int64"):
        ext.cam_order_many([sc], [wc[0]], [nbits])
    with pytest.raises(ValueError, match="nbits"):
        ext.cam_order_many([sc], [wc], [nbits + 64])
    with pytest.raises(ValueError, match="rows"):
        ext.cam_order_many([sc[:-1]], [wc], [nbits])


def test_worker_batched_mode_equals_the_default_on_gpu(monkeypatch):
    from simple_tip_amd import ops
    from simple_tip_amd.core import prioritizers
    from simple_tip_amd.engine.coverage_handler import CoverageWorker
    from simple_tip_amd.engine.model_handler import BaseModel
    from simple_tip_amd.models import MnistCNN

    monkeypatch.delenv("TIP_CAM_MODE", raising=False)
    monkeypatch.delenv("TIP_NC_MODE", raising=False)
    torch.manual_seed(0)
    model = MnistCNN().eval().cuda()
    rng = np.random.RandomState(0)
    train = rng.rand(96, 1, 28, 28).astype(np.float32)
    test = rng.rand(96, 1, 28, 28).astype(np.float32)
    many_calls = []
    real = ops.cam_order_many

    def spy(scores, words, nbits):
        many_calls.append([w.is_cuda for w in words])
        return real(scores, words, nbits)

    monkeypatch.setattr(prioritizers.ops, "cam_order_many", spy)

    def run(**kw):
        worker = CoverageWorker(
            BaseModel(model, [0, 1, 2, 3], device=torch.device("cuda:0"), predict_batch=32),
            train, **kw,
        )
        return worker.evaluate_all(test, "nominal")

    _, s_def, o_def = run()
    assert many_calls == []
    t_bat, s_bat, o_bat = run(cam_mode="batched")
    assert many_calls == [[True] * 12]
    assert list(s_bat) == list(s_def) and len(s_def) == 12
    for metric_id in s_def:
        assert np.array_equal(s_bat[metric_id], s_def[metric_id]), metric_id
        assert o_bat[metric_id] == o_def[metric_id], metric_id
        assert sorted(o_bat[metric_id]) == list(range(96))
        assert len(t_bat[metric_id]) == 4
    assert len({t_bat[m][3] for m in t_bat}) == 1
