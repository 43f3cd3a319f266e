"""Segment plan: the class-sorted, 128-padded batch layout as an index plan.

The torch reference (ops/fallback.py) is checked against a brute-force loop
on the CPU; the HIP kernel must equal the reference exactly (all integers).
"""

import numpy as np
import pytest
import torch

from simple_tip_amd.ops import fallback

SIZES = [1, 127, 128, 129, 777, 4099]
CLASSES = [1, 7, 10, 64]


def _brute(pred, c):
    """Row-by-row construction of (tseg, rowmap, dest)."""
    pred = [int(v) for v in pred]
    b = len(pred)
    counts = [0] * c
    for v in pred:
        if 0 <= v < c:
            counts[v] += 1
    tseg = [0]
    for n in counts:
        tseg.append(tseg[-1] + (n + 127) // 128 * 128)
    rowmap = [-1] * (128 * ((b + 127) // 128 + c))
    dest = [-1] * b
    placed = [0] * c
    for i, v in enumerate(pred):
        if 0 <= v < c:
            p = tseg[v] + placed[v]
            placed[v] += 1
            rowmap[p] = i
            dest[i] = p
    return tseg, rowmap, dest


def _special_cases():
    rng = np.random.RandomState(7)
    cases = {}
    cases["one_class"] = (np.full(777, 3), 7)
    absent = rng.randint(0, 7, 777)
    absent[absent == 2] = 5
    cases["absent_class"] = (absent, 7)
    exact = np.concatenate(
        [np.full(128, 0), np.full(129, 1), np.full(1, 2), np.full(256, 4)]
    )
    rng.shuffle(exact)
    cases["exact_128_129"] = (exact, 10)
    oor = rng.randint(0, 10, 777)
    oor[[0, 5, 300, 776]] = [10, -1, 64, 12345678901]
    cases["out_of_range"] = (oor, 10)
    return cases


def _random_case(b, c):
    rng = np.random.RandomState(1000 * c + b)
    return rng.randint(0, c, b)


def _check_equal(got, want):
    for g, w, name in zip(got, want, ("tseg", "rowmap", "dest")):
        g = torch.as_tensor(g).cpu().to(torch.int64)
        w = torch.as_tensor(w).cpu().to(torch.int64)
        assert g.shape == w.shape, name
        assert torch.equal(g, w), name


@pytest.mark.parametrize("c", CLASSES)
@pytest.mark.parametrize("b", SIZES)
def test_reference_matches_brute_force(b, c):
    pred = _random_case(b, c)
    got = fallback.segment_plan(torch.from_numpy(pred), c)
    assert all(t.dtype == torch.int32 for t in got)
    _check_equal(got, _brute(pred, c))


@pytest.mark.parametrize("name", sorted(_special_cases()))
def test_reference_special_cases(name):
    pred, c = _special_cases()[name]
    got = fallback.segment_plan(torch.from_numpy(pred), c)
    _check_equal(got, _brute(pred, c))
    tseg, rowmap, dest = got
    # rows past the last segment and every pad row are -1; each placed input
    # appears exactly once
    assert bool((rowmap[int(tseg[-1]):] == -1).all())
    placed = rowmap[rowmap >= 0].to(torch.int64)
    assert placed.numel() == int((dest >= 0).sum())
    assert torch.equal(dest[placed].to(torch.int64),
                       torch.nonzero(rowmap >= 0, as_tuple=True)[0])


def _device_plan(pred, c):
    from simple_tip_amd.ops import _load_compiled

    ext = _load_compiled()
    dev = torch.device("cuda:0")
    return ext.segment_plan(torch.from_numpy(np.asarray(pred)).to(dev), c)


@pytest.mark.gpu
@pytest.mark.parametrize("c", CLASSES)
def test_kernel_equals_reference(c):
    for b in SIZES:
        pred = _random_case(b, c)
        want = fallback.segment_plan(torch.from_numpy(pred), c)
        _check_equal(_device_plan(pred, c), want)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(_special_cases()))
def test_kernel_special_cases(name):
    pred, c = _special_cases()[name]
    want = fallback.segment_plan(torch.from_numpy(pred), c)
    _check_equal(_device_plan(pred, c), want)


@pytest.mark.gpu
def test_kernel_overwrites_stale_workspaces():
    """The *_out form fully defines its outputs whatever they held."""
    from simple_tip_amd.ops import _load_compiled

    ext = _load_compiled()
    dev = torch.device("cuda:0")
    pred = _random_case(777, 10)
    want = fallback.segment_plan(torch.from_numpy(pred), 10)
    tseg = torch.full((11,), 12345, dtype=torch.int32, device=dev)
    rowmap = torch.full((ext.segment_plan_rows(777, 10),), 7, dtype=torch.int32,
                        device=dev)
    dest = torch.full((777,), 9, dtype=torch.int32, device=dev)
    ext.segment_plan_out(torch.from_numpy(pred).to(dev), 10, tseg, rowmap, dest)
    _check_equal((tseg, rowmap, dest), want)
