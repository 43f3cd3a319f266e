"""Grouped Gaussian scoring on the GPU: grouped_center / grouped_quad /
grouped_gauss_final against the float64 fallback, with bounds derived from
the arithmetic (not tuned), bit-exact batch invariance, and the fuse() and
FusedPrioritizer.score_all layers on top.

Error model. The oracle is the fallback in float64 on the same fp32-rounded
x, means and mats. Per row and component the kernel's quadratic form q^
satisfies |q^ - q| <= 2 * gamma * (|d|^T |M| |d|) with gamma = (D + 72) *
2^-24: the fmaf chain of the tile core is D long, and the 72 covers the
centring subtraction (which enters twice), the 32-lane tree, the two-half
merge and the column-block fold. For the mixture the bound is half the
largest component bound plus 16 * 2^-24 * max(|nll|, max_j |c_j - q_j / 2|)
for the accurate expf / logf, the subtraction of the maximum and the sum
over at most 8 slots. Inputs follow M = Q diag(logspace(0, 3, D)) Q^T and
rows mu + randn, for which the Mahalanobis bound stays below 2e-3 * q on
every row (asserted), so the check cannot pass on a kernel that is off by
more than a fraction of a percent.
"""

import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DIMS = [7, 64, 160, 333]
COUNTS = [0, 1, 129, 300]      # rows per group: empty, single, two row blocks
MIX_COMPONENTS = [1, 3, 2, 1]  # components per group in mixture mode
EPS = 2.0 ** -24


def _dev():
    return torch.device("cuda:0")


def _precision(gen, d):
    q, _ = torch.linalg.qr(torch.randn(d, d, generator=gen, dtype=torch.float64))
    lam = torch.logspace(0, 3, d, dtype=torch.float64)
    m = (q * lam) @ q.t()
    return (0.5 * (m + m.t())).float()  # exactly symmetric in fp32


def _make(d, components, counts, seed, stray=4):
    """fp32 tables and rows; rows of group g sit around its first mean."""
    gen = torch.Generator().manual_seed(seed)
    off = np.concatenate([[0], np.cumsum(components)])
    j = int(off[-1])
    means = torch.randn(j, d, generator=gen).float()
    mats = torch.stack([_precision(gen, d) for _ in range(j)]).contiguous()
    logc = torch.randn(j, generator=gen).float()
    group = np.concatenate(
        [np.full(c, g) for g, c in enumerate(counts)]
        + [np.full(stray, -1), np.full(stray, len(counts))]
    )
    group = torch.from_numpy(group)[torch.randperm(len(group), generator=gen)]
    first = torch.from_numpy(off[:-1])[group.clamp(0, len(counts) - 1)]
    x = means[first] + torch.randn(len(group), d, generator=gen).float()
    return {
        "off": torch.from_numpy(off).to(torch.int32), "means": means,
        "mats": mats, "logc": logc, "group": group.long(), "x": x,
    }


def _oracle(x, group, off, means, mats, logc):
    """float64 oracle (the fallback op) and the derived bound, per row.
    Also returns q of slot 0 (for the non-vacuity condition)."""
    from simple_tip_amd.ops import fallback

    x, means, mats = x.double().cpu(), means.double().cpu(), mats.double().cpu()
    logc = None if logc is None else logc.double().cpu()
    group, offl = group.cpu(), off.cpu().tolist()
    n, d = x.shape
    gamma = (d + 72) * EPS
    smax = max(b - a for a, b in zip(offl[:-1], offl[1:]))
    qb = torch.zeros(n, smax, dtype=torch.float64)
    q0 = torch.zeros(n, dtype=torch.float64)
    tabs = torch.zeros(n, smax, dtype=torch.float64)
    for g in range(len(offl) - 1):
        rows = torch.nonzero(group == g, as_tuple=True)[0]
        for s, j in enumerate(range(offl[g], offl[g + 1])):
            dd = x[rows] - means[j]
            q = ((dd @ mats[j]) * dd).sum(dim=1)
            qb[rows, s] = 2 * gamma * ((dd.abs() @ mats[j].abs()) * dd.abs()).sum(dim=1)
            if s == 0:
                q0[rows] = q
            if logc is not None:
                tabs[rows, s] = (logc[j] - 0.5 * q).abs()
    want = fallback.grouped_gaussian_scores(x, group, off, means, mats, logc)
    if logc is None:
        bound = qb[:, 0]
    else:
        scale = torch.maximum(
            torch.where(torch.isfinite(want), want.abs(), torch.zeros_like(want)),
            tabs.max(dim=1).values,
        )
        bound = 0.5 * qb.max(dim=1).values + 16 * EPS * scale
    return want, bound, q0


def _check(got, want, bound, label):
    got = got.double().cpu()
    assert got.shape == want.shape
    placed = torch.isfinite(want)
    assert int(placed.sum()) > 0
    # unplaced rows (group id outside [0, G)) are exactly +inf
    assert torch.equal(got[~placed], want[~placed]), label
    err = (got[placed] - want[placed]).abs()
    ratio = float((err / bound[placed]).max())
    print(f"{label}: worst error / bound = {ratio:.3e}")
    assert bool((err <= bound[placed]).all()), (label, ratio)


@functools.lru_cache(maxsize=None)
def _case(d):
    """Tables, rows, oracle and GPU result per mode for one D (computed once
    and left unchanged)."""
    from simple_tip_amd import ops

    dev = _dev()
    r = {}
    for mode, comps in (("maha", [1] * len(COUNTS)), ("mix", MIX_COMPONENTS)):
        t = _make(d, comps, COUNTS, seed=100 + d)
        logc = t["logc"] if mode == "mix" else None
        t["want"], t["bound"], t["q0"] = _oracle(
            t["x"], t["group"], t["off"], t["means"], t["mats"], logc
        )
        t["args"] = (
            t["off"], t["means"].to(dev), t["mats"].to(dev),
            None if logc is None else logc.to(dev),
        )
        t["xd"], t["gd"] = t["x"].to(dev), t["group"].to(dev)
        t["got"] = ops.grouped_gaussian_scores(t["xd"], t["gd"], *t["args"])
        r[mode] = t
    return r


@pytest.mark.parametrize("d", DIMS)
def test_mahalanobis_within_derived_bound(d):
    t = _case(d)["maha"]
    assert t["got"].dtype == torch.float32 and t["got"].is_cuda
    placed = torch.isfinite(t["want"])
    assert int((~placed).sum()) == 8  # the stray ids -1 and G
    # non-vacuity: the bound itself is tight relative to the score
    worst = float((t["bound"][placed] / t["q0"][placed]).max())
    print(f"D={d}: worst bound / q = {worst:.3e}")
    assert worst <= 2e-3
    _check(t["got"], t["want"], t["bound"], f"mahalanobis D={d}")


@pytest.mark.parametrize("d", DIMS)
def test_mixture_within_derived_bound(d):
    t = _case(d)["mix"]
    _check(t["got"], t["want"], t["bound"], f"mixture D={d}")


def test_single_group_five_rows():
    from simple_tip_amd import ops

    dev = _dev()
    t = _make(160, [1], [5], seed=7, stray=0)
    want, bound, q0 = _oracle(t["x"], t["group"], t["off"], t["means"], t["mats"], None)
    got = ops.grouped_gaussian_scores(
        t["x"].to(dev), t["group"].to(dev), t["off"], t["means"].to(dev),
        t["mats"].to(dev),
    )
    assert float((bound / q0).max()) <= 2e-3
    _check(got, want, bound, "G=1, 5 rows")


@pytest.mark.parametrize("mode", ["maha", "mix"])
def test_bf16_rows(mode):
    """bf16 x is widened exactly; the oracle sees the bf16-rounded values."""
    from simple_tip_amd import ops

    t = _case(160)[mode]
    x16 = t["xd"].to(torch.bfloat16)
    logc = t["logc"] if mode == "mix" else None
    want, bound, _ = _oracle(
        x16.float(), t["group"], t["off"], t["means"], t["mats"], logc
    )
    got = ops.grouped_gaussian_scores(x16, t["gd"], *t["args"])
    _check(got, want, bound, f"bf16 rows, {mode}")
    # and it is the fp32 kernel on the widened rows, bit for bit
    same = ops.grouped_gaussian_scores(x16.float(), t["gd"], *t["args"])
    assert torch.equal(got, same)


@pytest.mark.parametrize("d,mode", [(333, "mix"), (333, "maha"), (7, "mix")])
def test_batch_invariance_bit_for_bit(d, mode):
    from simple_tip_amd import ops

    t = _case(d)[mode]
    x, g, args, full = t["xd"], t["gd"], t["args"], t["got"]
    n = x.shape[0]
    h = n // 2
    halves = torch.cat([
        ops.grouped_gaussian_scores(x[:h], g[:h], *args),
        ops.grouped_gaussian_scores(x[h:], g[h:], *args),
    ])
    assert torch.equal(halves, full)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(3)).to(x.device)
    shuffled = ops.grouped_gaussian_scores(x[perm], g[perm], *args)
    assert torch.equal(shuffled, full[perm])


@pytest.mark.parametrize("mode", ["maha", "mix"])
def test_workspace_cap_chunks_invisibly(monkeypatch, mode):
    from simple_tip_amd import ops
    from simple_tip_amd.ops import hip_ops

    t = _case(160)[mode]
    monkeypatch.setattr(hip_ops, "GAUSS_WORKSPACE_BYTES", 1)
    tables = hip_ops.GaussianTables(*t["args"], _dev())
    assert tables.chunk_rows() == 128 < t["xd"].shape[0]
    got = ops.grouped_gaussian_scores(t["xd"], t["gd"], *t["args"])
    assert torch.equal(got, t["got"])


def test_envelope_errors_on_gpu():
    from simple_tip_amd import ops

    dev = _dev()
    x = torch.zeros(4, 8, device=dev)
    g = torch.zeros(4, dtype=torch.int64, device=dev)
    eye = torch.eye(8, device=dev)

    def call(components, mats=None, logc=True):
        j = sum(components)
        off = torch.tensor(np.concatenate([[0], np.cumsum(components)]), dtype=torch.int32)
        m = eye.repeat(j, 1, 1) if mats is None else mats
        lc = torch.zeros(j, device=dev) if logc else None
        return ops.grouped_gaussian_scores(x, g, off, torch.zeros(j, 8, device=dev), m, lc)

    with pytest.raises(ValueError):
        call([9])
    with pytest.raises(ValueError):
        call([1] * 257)
    with pytest.raises(ValueError):
        call([2], mats=torch.randn(2, 8, 16, device=dev)[:, :, ::2])
    with pytest.raises(ValueError):
        call([2], logc=False)
    # inside the envelope: two unit components at the origin, nll = -log 2
    torch.testing.assert_close(
        call([2]).cpu(), torch.full((4,), -float(np.log(2.0))), rtol=1e-6, atol=0.0
    )


# --- layers: MultiModalSA.fuse() and FusedPrioritizer.score_all --------------

AT_DIM = 16


def _structured(seed, n, classes=3):
    rng = np.random.RandomState(seed)
    pred = rng.randint(0, classes, size=n)
    centers = np.random.RandomState(99).randn(classes, AT_DIM) * 3.0
    ats = centers[pred] + rng.randn(n, AT_DIM) * (1.0 + 0.3 * pred[:, None])
    return torch.from_numpy(ats.astype(np.float32)), torch.from_numpy(pred)


@functools.lru_cache(maxsize=None)
def _fits():
    from simple_tip_amd.core.surprise import DSA, LSA, MDSA, MLSA, MultiModalSA

    dev = _dev()
    ats, pred = _structured(0, 900)
    ats_d, pred_d = ats.to(dev), pred.to(dev)
    gauss = {
        "pc-mdsa": MultiModalSA.build_by_class(ats_d, pred_d, lambda a, p: MDSA(a)),
        "pc-mlsa": MultiModalSA.build_by_class(
            ats_d, pred_d, lambda a, p: MLSA(a, num_components=2)
        ),
        "pc-mmdsa": MultiModalSA.build_with_kmeans(
            ats_d, pred_d, lambda a, p: MDSA(a),
            potential_k=range(2, 4), n_init=2, max_iter=50,
        ),
    }
    dsa = DSA(ats, pred, device=dev)
    lsa = MultiModalSA.build_by_class(
        ats, pred, lambda a, p: LSA(a, max_features=8, device=dev)
    )
    test, tp = _structured(1, 389)
    return {
        "gauss": gauss, "dsa": dsa, "lsa": lsa,
        "test": test.to(dev), "tp": tp.to(dev),
        "fused": {k: v.fuse(dev) for k, v in gauss.items()},
    }


@pytest.mark.parametrize("name", ["pc-mdsa", "pc-mlsa", "pc-mmdsa"])
def test_fuse_within_derived_bound(name):
    f = _fits()
    fused, test, tp = f["fused"][name], f["test"], f["tp"]
    got = fused(test, tp)
    assert got.dtype == torch.float32 and got.is_cuda and got.shape == (389,)
    group = fused.groups_of(fused.mode_ids(test, tp))
    want, bound, _ = _oracle(
        test, group, fused.comp_off, fused.means, fused.mats, fused.logc
    )
    assert bool(torch.isfinite(want).all())
    _check(got, want, bound, f"fuse {name}")
    # the per-mode loop (fp32 torch) is the same quantity, to its own rounding
    per_mode = f["gauss"][name](test, tp).double().cpu()
    assert float(((per_mode - want).abs() / want.abs().clamp_min(1.0)).max()) < 1e-2


def test_fuse_unseen_mode_on_gpu():
    from simple_tip_amd.core import surprise

    f = _fits()
    fused, test = f["fused"]["pc-mdsa"], f["test"]
    tp = f["tp"].clone()
    tp[::9] = 6
    with pytest.warns(UserWarning, match="No modal found for modal id 6"):
        got = fused(test, tp)
    assert bool(torch.isinf(got[::9]).all()) and bool((got[::9] > 0).all())
    keep = torch.ones_like(tp, dtype=torch.bool)
    keep[::9] = False
    assert torch.equal(got[keep], fused(test, f["tp"])[keep])
    prev = surprise.set_strict_modes(True)
    try:
        with pytest.raises(ValueError, match="No modal found"):
            fused(test, tp)
    finally:
        surprise.set_strict_modes(prev)


def test_fuse_without_the_check_makes_no_host_copy():
    f = _fits()
    test, tp = f["test"], f["tp"]
    for name in ("pc-mlsa", "pc-mmdsa"):
        fused = f["gauss"][name].fuse(_dev())
        fused.check_unseen = False
        ref = fused(test, tp)  # warm call: tables, workspaces
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            got = fused(test, tp)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert torch.equal(got, ref)
        assert torch.equal(got, f["fused"][name](test, tp))


@functools.lru_cache(maxsize=None)
def _prioritizers(path):
    from simple_tip_amd.engine.serving import FusedPrioritizer

    f = _fits()
    kw = dict(pairwise_dtype=torch.bfloat16, fast=(path == "fast"))
    with_g = FusedPrioritizer(f["dsa"], f["lsa"], _dev(), gaussian=f["gauss"], **kw)
    plain = FusedPrioritizer(f["dsa"], f["lsa"], _dev(), **kw)
    assert with_g.fast == plain.fast == (path == "fast")
    return with_g, plain


@pytest.mark.parametrize("path", ["fast", "slow"])
def test_score_all_layers(path):
    f = _fits()
    test, tp = f["test"], f["tp"]
    with_g, plain = _prioritizers(path)
    res = with_g.score_all(test, tp)
    assert list(res) == ["dsa", "pc-lsa", "pc-mdsa", "pc-mlsa", "pc-mmdsa"]
    dsa, lsa = plain(test, tp)
    assert torch.equal(res["dsa"], dsa) and torch.equal(res["pc-lsa"], lsa)
    again = with_g(test, tp)  # __call__ keeps its return type
    assert isinstance(again, tuple) and len(again) == 2
    assert torch.equal(again[0], dsa) and torch.equal(again[1], lsa)
    for name, fused in f["fused"].items():
        assert torch.equal(res[name], fused(test, tp)), name
    # stale workspaces: nothing read into an output depends on them
    torch.cuda.synchronize()
    spaces = list(getattr(with_g, "_ws", {}).values())
    spaces += [ws for g in with_g.gaussian.values() for ws in g.tables(_dev())._ws.values()]
    assert spaces
    for ws in spaces:
        for t in ws.values():
            t.fill_(float("nan") if t.is_floating_point() else -1)
    res2 = with_g.score_all(test, tp)
    for k in res:
        assert torch.equal(res[k], res2[k]), k


def test_score_all_fast_path_makes_no_host_copy():
    f = _fits()
    with_g, _ = _prioritizers("fast")
    ref = with_g.score_all(f["test"], f["tp"])  # warm call
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        res = with_g.score_all(f["test"], f["tp"])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for k in ref:
        assert torch.equal(res[k], ref[k]), k
