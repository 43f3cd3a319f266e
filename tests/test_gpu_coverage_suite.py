"""coverage_suite.hip against the per-metric HIP ops and ops/fallback.py.

Every comparison is ``torch.equal`` on words and scores: the suite makes the
same comparisons as the per-metric kernels, so there is no tolerance. The
inputs put activations exactly on, one float below and one float above every
quantity a kernel compares with, mix in NaN, +-inf and -0.0, and keep every
third row mostly exact zeros so that the TKNC cut falls inside a tie. The
shapes put layer and chunk boundaries inside words.
"""

import functools

import numpy as np
import pytest
import torch

from simple_tip_amd.ops import fallback

pytestmark = pytest.mark.gpu

POOL_ROWS = 67  # three row tiles of the kernel, the last one ragged
NAC_THRESHOLDS = (0.0, 0.75, 0.3)  # 0.3 is no float32: pins the cast
SCALERS = (0.0, 0.5, 1.0)
KMNC_SECTIONS = (2, 3, 5, 16)
TKNC_KS = (1, 2, 3, 4)
FAMILIES = fallback.COVERAGE_SUITE_FAMILIES


@pytest.fixture(scope="module")
def ext():
    from simple_tip_amd.ops import hip_ops

    return hip_ops


def _chunk():
    from simple_tip_amd.ops import hip_ops

    return hip_ops.coverage_suite_chunk()


def _shapes():
    c = _chunk()
    return {
        "canon_small": [70, 64, 1, 130],
        "chunk_minus_1": [c - 1],
        "chunk": [c],
        "chunk_plus_1": [c + 1],
        "straddle": [c - 30, 95, 2 * c + 65],
        "width_1": [1],
    }


SHAPE_NAMES = [
    "canon_small", "chunk_minus_1", "chunk", "chunk_plus_1", "straddle", "width_1",
]


def _f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


@functools.lru_cache(maxsize=None)
def _case(name):
    """Tables, the 67-row pool of layers and the fallback's answer for it."""
    widths = _shapes()[name]
    k = sum(widths)
    rng = np.random.RandomState(700 + SHAPE_NAMES.index(name))
    mins = rng.randn(k).astype(np.float32)
    mins[mins == 0] = np.float32(0.5)
    maxs = (mins + np.abs(rng.randn(k)).astype(np.float32) + np.float32(0.1))
    maxs = maxs.astype(np.float32)
    if k > 8:
        maxs[7] = mins[7]  # a constant neuron: every KMNC section is empty
    stds = rng.rand(k).astype(np.float32)
    upper = np.stack([maxs + np.float32(s) * stds for s in SCALERS]).astype(np.float32)
    lower = np.stack([mins - np.float32(s) * stds for s in SCALERS]).astype(np.float32)

    # every quantity an activation is compared with, as a [K] vector
    compared = [np.full(k, t, dtype=np.float32) for t in NAC_THRESHOLDS]
    compared += list(upper) + list(lower)
    tmins, tmaxs = _f32(mins), _f32(maxs)
    for sections in KMNC_SECTIONS:
        jumps = (tmaxs - tmins) / sections
        for s in range(sections + 1):  # as fallback.kmnc_profile forms them
            compared.append((tmins + jumps * s).numpy())
    variants = []
    for q in compared:
        variants += [
            q,
            np.nextafter(q, np.float32(-np.inf), dtype=np.float32),
            np.nextafter(q, np.float32(np.inf), dtype=np.float32),
        ]
    for special in (np.nan, np.inf, -np.inf, -0.0, 0.0):
        variants.append(np.full(k, special, dtype=np.float32))
    variants = np.stack(variants)  # [V, K]

    rows = np.arange(POOL_ROWS)[:, None]
    cols = np.arange(k)[None, :]
    acts = variants[(rows * 5 + cols) % variants.shape[0], cols]
    # every third row: exact zeros (some negative) but for a few entries
    sparse = rng.rand(POOL_ROWS, k) < 0.97
    sparse[np.arange(POOL_ROWS) % 3 != 2] = False
    acts = np.where(sparse, np.where(cols % 2 == 0, 0.0, -0.0), acts)
    acts = acts.astype(np.float32)
    layers, at = [], 0
    for w in widths:
        layers.append(_f32(acts[:, at:at + w]))
        at += w
    tables = dict(
        nac_thresholds=NAC_THRESHOLDS,
        upper_bounds=_f32(upper),
        nbc_lower=_f32(lower),
        nbc_upper=_f32(upper),
        kmnc_mins=tmins,
        kmnc_maxs=tmaxs,
        kmnc_sections=KMNC_SECTIONS,
        tknc_ks=TKNC_KS,
    )
    want = fallback.coverage_suite(layers, **tables)
    return layers, tables, want


def _cuda_tables(tables):
    return {
        key: v.cuda() if isinstance(v, torch.Tensor) else v
        for key, v in tables.items()
    }


def _per_metric(ext, layers, tables):
    """The existing HIP ops on the concatenated input."""
    acts = torch.cat(layers, dim=1)
    t = tables
    return {
        "nac": [ext.nac_profile(acts, thr) for thr in t["nac_thresholds"]],
        "snac": [ext.snac_profile(acts, u) for u in t["upper_bounds"]],
        "nbc": [
            ext.nbc_profile(acts, l, u)
            for l, u in zip(t["nbc_lower"], t["nbc_upper"])
        ],
        "kmnc": [
            ext.kmnc_profile(acts, t["kmnc_mins"], t["kmnc_maxs"], s)
            for s in t["kmnc_sections"]
        ],
        "tknc": [ext.tknc_profile(layers, k) for k in t["tknc_ks"]],
    }


ROW_SETS = {1: [2], 5: [0, 2, 21, 44, 66], 67: list(range(POOL_ROWS))}


@pytest.mark.parametrize("n", [1, 5, 67])
@pytest.mark.parametrize("name", SHAPE_NAMES)
def test_suite_equals_per_metric_ops_and_fallback(ext, name, n):
    layers, tables, want = _case(name)
    pick = ROW_SETS[n]
    dev_layers = [l[pick].contiguous().cuda() for l in layers]
    dev_tables = _cuda_tables(tables)
    got = ext.coverage_suite(dev_layers, **dev_tables)
    hip = _per_metric(ext, dev_layers, dev_tables)
    assert list(got) == list(FAMILIES)
    for fam in FAMILIES:
        assert len(got[fam]) == len(want[fam]) == len(hip[fam]) == (
            3 if fam in ("nac", "snac", "nbc") else 4
        )
        for i, (words, scores) in enumerate(got[fam]):
            assert words.dtype == torch.int64 and scores.dtype == torch.int64
            assert words.is_contiguous() and scores.shape == (n,)
            assert torch.equal(words, hip[fam][i]), (fam, i, "per-metric op")
            assert torch.equal(words.cpu(), want[fam][i][0][pick]), (fam, i, "fallback")
            assert torch.equal(scores, ext.popcount_rows(words)), (fam, i)
            assert torch.equal(scores.cpu(), want[fam][i][1][pick]), (fam, i)


def test_inputs_reach_the_edges():
    """The pool holds what the docstring promises (no GPU work)."""
    layers, tables, want = _case("straddle")
    acts = torch.cat(layers, dim=1)
    assert torch.isnan(acts).any() and torch.isinf(acts).any()
    assert (acts == tables["upper_bounds"][1]).any()
    assert (acts == tables["nbc_lower"][2]).any()
    assert (acts == 0.75).any()
    signs = torch.signbit(acts) & (acts == 0)
    assert signs.any()
    # a sparse row has fewer positive entries in some layer than k = 4
    assert ((layers[1][2] > 0).sum() < 4) and (layers[1][2] == 0).sum() > 4
    # KMNC: sections 5 and 16 have boundaries that a fused multiply-add moves
    lo, hi = tables["kmnc_mins"], tables["kmnc_maxs"]
    moved = 0
    for sections in (5, 16):
        jumps = (hi - lo) / sections
        for s in range(1, sections):
            moved += int(((lo + jumps * s) != (lo.double() + jumps.double() * s).float()).sum())
    assert moved >= 10
    assert int(want["kmnc"][3][1].max()) > 0


def test_rows_do_not_depend_on_the_batch(ext):
    layers, tables, _ = _case("straddle")
    dev_tables = _cuda_tables(tables)
    full = ext.coverage_suite([l.cuda() for l in layers], **dev_tables)
    for row in (0, 2, 31, 32, 65, 66):
        one = ext.coverage_suite(
            [l[row:row + 1].contiguous().cuda() for l in layers], **dev_tables
        )
        for fam in FAMILIES:
            for (w_full, s_full), (w_one, s_one) in zip(full[fam], one[fam]):
                assert torch.equal(w_one[0], w_full[row]), (fam, row)
                assert torch.equal(s_one[0], s_full[row]), (fam, row)


@pytest.mark.parametrize("family", FAMILIES)
def test_any_family_alone(ext, family):
    layers, tables, want = _case("canon_small")
    keys = {
        "nac": ["nac_thresholds"],
        "snac": ["upper_bounds"],
        "nbc": ["nbc_lower", "nbc_upper"],
        "kmnc": ["kmnc_mins", "kmnc_maxs", "kmnc_sections"],
        "tknc": ["tknc_ks"],
    }[family]
    only = _cuda_tables({key: tables[key] for key in keys})
    got = ext.coverage_suite([l.cuda() for l in layers], **only)
    for fam in FAMILIES:
        if fam != family:
            assert got[fam] == []
    for (words, scores), (w, s) in zip(got[family], want[family]):
        assert torch.equal(words.cpu(), w) and torch.equal(scores.cpu(), s)


def test_layer_of_width_one_with_k_three(ext):
    # one real entry, three asked for: the empty slots set nothing
    layers = [_f32([[0.5], [np.nan], [-np.inf]]), _f32(np.zeros((3, 2)))]
    got = ext.coverage_suite([l.cuda() for l in layers], tknc_ks=(3,))
    words, scores = got["tknc"][0]
    assert torch.equal(words.cpu(), fallback.tknc_profile(layers, 3))
    assert scores.tolist() == [3, 3, 3] and words.cpu()[:, 0].tolist() == [7, 7, 7]


def test_envelope_violations_raise_value_error(ext):
    k = 40
    layer = torch.zeros(3, k, device="cuda")
    table = torch.zeros(5, k, device="cuda")
    vec = torch.zeros(k, device="cuda")
    bad = [
        dict(layers=[layer[:, :4].contiguous()] * 9, nac_thresholds=(0.0,)),
        dict(layers=[layer], nac_thresholds=(0.0, 0.1, 0.2, 0.3, 0.4)),
        dict(layers=[layer], upper_bounds=table),
        dict(layers=[layer], nbc_lower=table, nbc_upper=table),
        dict(layers=[layer], kmnc_mins=vec, kmnc_maxs=vec, kmnc_sections=(1, 2, 3, 4, 5)),
        dict(layers=[layer], tknc_ks=(1, 2, 3, 4, 1)),
        dict(layers=[layer], kmnc_mins=vec, kmnc_maxs=vec, kmnc_sections=(0,)),
        dict(layers=[layer], kmnc_mins=vec, kmnc_maxs=vec, kmnc_sections=(17,)),
        dict(layers=[layer], tknc_ks=(0,)),
        dict(layers=[layer], tknc_ks=(5,)),
        dict(layers=[layer, torch.zeros(4, 2, device="cuda")], nac_thresholds=(0.0,)),
        dict(layers=[layer], upper_bounds=table[:2, :k - 1].contiguous()),
        dict(layers=[layer], nbc_lower=table[:2, :k - 1].contiguous(),
             nbc_upper=table[:2, :k - 1].contiguous()),
        dict(layers=[layer], nbc_lower=table[:2], nbc_upper=table[:3]),
        dict(layers=[layer], kmnc_mins=vec[:-1], kmnc_maxs=vec, kmnc_sections=(2,)),
        dict(layers=[layer], kmnc_mins=vec, kmnc_maxs=vec[:-1], kmnc_sections=(2,)),
    ]
    for kw in bad:
        layers = kw.pop("layers")
        with pytest.raises(ValueError):
            ext.coverage_suite(layers, **kw)
    # the limits themselves are inside
    ok = ext.coverage_suite(
        [layer[:, :5].contiguous()] * 8, nac_thresholds=(0.0,) * 4,
        upper_bounds=table[:4], nbc_lower=table[:4], nbc_upper=table[:4],
        kmnc_mins=vec, kmnc_maxs=vec, kmnc_sections=(1, 16, 16, 16),
        tknc_ks=(1, 4, 4, 4),
    )
    assert [len(ok[f]) for f in FAMILIES] == [4, 4, 4, 4, 4]


def test_worker_fused_mode_equals_the_default_on_gpu(monkeypatch):
    from simple_tip_amd import ops
    from simple_tip_amd.engine.coverage_handler import CoverageWorker
    from simple_tip_amd.engine.model_handler import BaseModel
    from simple_tip_amd.models import MnistCNN

    monkeypatch.delenv("TIP_NC_MODE", raising=False)
    torch.manual_seed(0)
    model = MnistCNN().eval().cuda()
    rng = np.random.RandomState(0)
    train = rng.rand(96, 1, 28, 28).astype(np.float32)
    test = rng.rand(96, 1, 28, 28).astype(np.float32)
    suite_calls = []
    real = ops.coverage_suite

    def spy(layers, **kw):
        suite_calls.append(layers[0].is_cuda)
        return real(layers, **kw)

    monkeypatch.setattr(ops, "coverage_suite", spy)

    def run(**kw):
        worker = CoverageWorker(
            BaseModel(model, [0, 1, 2, 3], device=torch.device("cuda:0"), predict_batch=32),
            train, **kw,
        )
        return worker.evaluate_all(test, "nominal")

    _, s_def, o_def = run()
    assert suite_calls == []
    t_fus, s_fus, o_fus = run(nc_mode="fused")
    assert suite_calls == [True, True, True]
    assert list(s_fus) == list(s_def) and len(s_def) == 12
    for metric_id in s_def:
        assert np.array_equal(s_fus[metric_id], s_def[metric_id]), metric_id
        assert o_fus[metric_id] == o_def[metric_id], metric_id
        assert len(t_fus[metric_id]) == 4
