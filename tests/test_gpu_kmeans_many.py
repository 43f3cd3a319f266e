"""Batched k-means kernels on the GPU (kmeans_many.hip, the silhouette
epilogue of pairwise.hip): the assign is bit-equal to rowmin_l2, the update is
reproducible and independent of the other problems, the silhouette cluster
sums stay inside a derived rounding bound, and the batched discovery agrees
with the looped one end to end.

Shapes: N in {129, 300} (a row and a column tile tail) and D in {37, 64} (the
scalar K-tail and the float4 path); problems of k = 2, 3, 5 and 16 centres
(C = 26, two Gram passes of the silhouette kernel)."""

import numpy as np
import pytest
import torch

from simple_tip_amd import ops

pytestmark = pytest.mark.gpu

KS = (2, 3, 5, 16)
SEG = [0, 2, 5, 10, 26]
SHAPES = [(129, 37), (300, 64), (300, 37), (129, 64)]


def _dev():
    return torch.device("cuda:0")


def _case(n, d):
    """Rows (two of them identical), stacked centres (one x row twice in a
    problem, one centre far from every row) and per-problem labels (row 3
    alone in cluster 15 of the k = 16 problem)."""
    rng = np.random.RandomState(n * 100 + d)
    x = rng.randn(n, d).astype(np.float32)
    x[11] = x[10]
    centers = np.concatenate(
        [x[rng.choice(n, k, replace=False)] + 0.1 * rng.randn(k, d) for k in KS]
    ).astype(np.float32)
    centers[6] = x[20]  # problem k = 5 holds x[20] twice: local 1 and 3
    centers[8] = x[20]
    centers[9] = 1e3    # claims no row
    labels = np.stack([rng.randint(0, min(k, 15), n) for k in KS])
    labels[:, :40] = 0
    labels[3, 3] = 15
    dev = _dev()
    return (
        torch.from_numpy(x).to(dev),
        torch.from_numpy(centers).to(dev),
        torch.tensor(SEG, dtype=torch.int32, device=dev),
        torch.from_numpy(labels.astype(np.int32)).to(dev),
    )


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: f"N{s[0]}-D{s[1]}")
def case(request):
    return _case(*request.param)


def test_assign_bit_equal_to_rowmin(case):
    x, centers, seg, _ = case
    labels, mind = ops.lloyd_assign_many(x, centers, seg)
    again = ops.lloyd_assign_many(x, centers, seg, SEG, ops.row_sqnorms(x))
    assert labels.dtype == torch.int32 and labels.shape == (len(KS), x.shape[0])
    for p in range(len(KS)):
        d, idx = ops.rowmin_l2(x, centers[SEG[p] : SEG[p + 1]])
        assert torch.equal(labels[p].long(), idx), p
        assert torch.equal(mind[p], d), p
    assert torch.equal(again[0], labels) and torch.equal(again[1], mind)
    # x[20] sits at local centres 1 and 3 of the k = 5 problem: lowest wins,
    # at a distance that is zero up to the rounding of the Gram form
    e = (x.shape[1] + 3) * 2.0 ** -23 * 2.0 * float(x[20].double().pow(2).sum())
    assert labels[2, 20].item() == 1 and mind[2, 20].item() <= e ** 0.5


def _update(x, labels, centers, seg, active=None, tol=1e-4):
    c = centers.clone()
    p = seg.shape[0] - 1
    a = (
        torch.ones(p, dtype=torch.int32, device=x.device)
        if active is None
        else active.clone()
    )
    shift, counts = ops.lloyd_update_many(x, labels, c, seg, a, tol=tol)
    return c, shift, counts, a


def test_update_matches_float64_means(case):
    x, centers, seg, _ = case
    labels, _ = ops.lloyd_assign_many(x, centers, seg)
    new, shift, counts, _ = _update(x, labels, centers, seg)
    xd, worst = x.double().cpu(), 0.0
    for p in range(len(KS)):
        lab = labels[p].cpu()
        for c in range(KS[p]):
            rows = xd[lab == c]
            cnt = rows.shape[0]
            got = new[SEG[p] + c].double().cpu()
            assert counts[SEG[p] + c].item() == cnt
            if cnt == 0:
                assert torch.equal(new[SEG[p] + c], centers[SEG[p] + c])
                continue
            bound = (cnt + 2) * 2.0 ** -24 * rows.abs().sum(dim=0)
            err = (got - rows.mean(dim=0)).abs()
            worst = max(worst, float((err / bound).max()))
            assert bool((err <= bound).all()), (p, c)
        want = (new[SEG[p] : SEG[p + 1]] - centers[SEG[p] : SEG[p + 1]]).double().pow(2).sum()
        assert float(shift[p]) == pytest.approx(float(want), rel=1e-5)
    print(f"update: worst error / bound = {worst:.3e}")
    assert counts[9].item() == 0  # the far centre stayed empty


def test_update_reproducible_and_independent(case):
    x, centers, seg, _ = case
    labels, _ = ops.lloyd_assign_many(x, centers, seg)
    c1, s1, n1, _ = _update(x, labels, centers, seg)
    c2, s2, n2, _ = _update(x, labels, centers, seg)
    assert torch.equal(c1, c2) and torch.equal(s1, s2) and torch.equal(n1, n2)
    for p in range(len(KS)):
        a, b = SEG[p], SEG[p + 1]
        seg1 = torch.tensor([0, b - a], dtype=torch.int32, device=x.device)
        alone, sh, cnt, _ = _update(
            x, labels[p : p + 1].contiguous(), centers[a:b].contiguous(), seg1
        )
        assert torch.equal(alone, c1[a:b]), p
        assert torch.equal(sh[0], s1[p]) and torch.equal(cnt, n1[a:b]), p


def test_update_inactive_and_tol(case):
    x, centers, seg, _ = case
    labels, _ = ops.lloyd_assign_many(x, centers, seg)
    active = torch.tensor([1, 0, 1, 0], dtype=torch.int32, device=x.device)
    new, shift, counts, act = _update(x, labels, centers, seg, active, tol=0.0)
    full, fshift, _, _ = _update(x, labels, centers, seg, tol=0.0)
    for p in (1, 3):
        a, b = SEG[p], SEG[p + 1]
        assert torch.equal(new[a:b], centers[a:b])
        assert float(shift[p]) == 0.0 and int(counts[a:b].abs().sum()) == 0
    for p in (0, 2):
        a, b = SEG[p], SEG[p + 1]
        assert torch.equal(new[a:b], full[a:b]) and torch.equal(shift[p], fshift[p])
    assert act.tolist() == [1, 0, 1, 0]
    # active is cleared exactly when shift <= tol
    s = fshift.tolist()
    order = sorted(range(len(KS)), key=lambda p: s[p])
    assert s[order[0]] > 0 and s[order[0]] < s[order[1]]
    _, _, _, act = _update(x, labels, centers, seg, tol=s[order[1]])
    want = [0 if s[p] <= s[order[1]] else 1 for p in range(len(KS))]
    assert act.tolist() == want and sum(want) == len(KS) - 2
    below = float(np.nextafter(np.float32(s[order[0]]), np.float32(0)))
    _, _, _, act = _update(x, labels, centers, seg, tol=below)
    assert act.tolist() == [1, 1, 1, 1]


def _silhouette_oracle(x, labels):
    """float64 cluster sums on the host and their rounding bound.

    Per pair e_ij = (D + 3) * 2^-23 * (|x_i|^2 + |x_j|^2) bounds the error of
    the fp32 Gram form of d_ij^2 (two norms, the dot product, two adds), so a
    term is off by at most min(sqrt(e_ij), e_ij / d_ij); adding count_bin
    terms in fp32 costs at most count_bin * 2^-24 * sum_j d_ij. The diagonal
    term is exact."""
    xd = x.double().cpu()
    n, d = xd.shape
    dist = (xd[:, None, :] - xd[None, :, :]).pow(2).sum(-1).sqrt()
    dist.fill_diagonal_(0.0)
    nrm = xd.pow(2).sum(dim=1)
    e = (d + 3) * 2.0 ** -23 * (nrm[:, None] + nrm[None, :])
    term = torch.minimum(e.sqrt(), e / dist.clamp_min(1e-300))
    term.fill_diagonal_(0.0)
    lab = labels.cpu()
    sums = torch.zeros(n, SEG[-1], dtype=torch.float64)
    bound = torch.zeros(n, SEG[-1], dtype=torch.float64)
    for p in range(len(KS)):
        for c in range(KS[p]):
            m = lab[p] == c
            col = dist[:, m].sum(dim=1)
            sums[:, SEG[p] + c] = col
            bound[:, SEG[p] + c] = term[:, m].sum(dim=1) + int(m.sum()) * 2.0 ** -24 * col
    return sums, bound


def test_silhouette_sums_within_derived_bound(case):
    x, _, seg, labels = case
    got = ops.silhouette_cluster_sums(x, labels, seg)
    again = ops.silhouette_cluster_sums(x, labels, seg, SEG)
    assert got.shape == (x.shape[0], SEG[-1]) and torch.equal(got, again)
    sums, bound = _silhouette_oracle(x, labels)
    err = (got.double().cpu() - sums).abs()
    live = bound > 0
    ratio = float((err[live] / bound[live]).max())
    print(f"silhouette sums: worst error / bound = {ratio:.3e}")
    assert ratio <= 1.0
    # a bin without other rows holds an exact zero
    assert float(err[~live].max()) == 0.0
    tight = float((bound[live] / sums[live]).max())
    print(f"silhouette sums: worst bound / sum = {tight:.3e}")
    assert tight < 1e-3
    # row 3 is alone in cluster 15 of the k = 16 problem: only its own,
    # exactly zero, diagonal term
    assert got[3, SEG[3] + 15].item() == 0.0
    assert (got[:, SEG[3] + 15] > 0).sum().item() == x.shape[0] - 1


def test_silhouette_sums_ignore_out_of_range_labels(case):
    x, _, seg, labels = case
    bad = labels.clone()
    bad[0, 5], bad[1, 6], bad[3, 7] = -1, 3, 16
    got = ops.silhouette_cluster_sums(x, bad, seg)
    ref = ops.silhouette_cluster_sums(x, labels, seg)
    xd = x.double().cpu()
    for p, j in ((0, 5), (1, 6), (3, 7)):
        col = SEG[p] + int(labels[p, j])
        drop = (xd - xd[j]).pow(2).sum(dim=1).sqrt()
        torch.testing.assert_close(
            got[:, col].double().cpu(), ref[:, col].double().cpu() - drop,
            rtol=1e-5, atol=1e-4,
        )


@pytest.fixture(scope="module")
def far_blobs():
    """Five blobs whose centres are 20 apart, unit variance, N = 300, D = 37."""
    rng = np.random.RandomState(3)
    mus = np.zeros((5, 37))
    mus[np.arange(5), np.arange(5)] = 20.0 / np.sqrt(2.0)
    x = np.concatenate([mus[i] + rng.randn(60, 37) for i in range(5)])
    rng.shuffle(x)
    return torch.from_numpy(x.astype(np.float32))


def test_fit_many_gpu_labels_equal_cpu(far_blobs):
    from simple_tip_amd.core.kmeans import kmeans_fit_many

    ks = (2, 3, 4, 5)
    cpu = kmeans_fit_many(far_blobs, ks, n_init=3, seed=0)
    stats = {}
    gpu = kmeans_fit_many(far_blobs.to(_dev()), ks, n_init=3, seed=0, stats=stats)
    assert 1 <= stats["lloyd_iterations"] <= 300
    for k in ks:
        assert torch.equal(gpu[k][1].cpu(), cpu[k][1]), k
        torch.testing.assert_close(gpu[k][0].cpu(), cpu[k][0], rtol=1e-5, atol=1e-5)
        assert gpu[k][2] == pytest.approx(cpu[k][2], rel=1e-5)


def test_discriminator_and_multimodal_batched_match_looped(far_blobs):
    from simple_tip_amd.core.surprise import MDSA, MultiModalSA, _KmeansDiscriminator

    x = far_blobs.to(_dev())
    kw = dict(potential_k=range(2, 6), n_init=3)
    looped = _KmeansDiscriminator(x, **kw)
    batched = _KmeansDiscriminator(x, kmeans_mode="batched", **kw)
    assert batched.best_k == looped.best_k == 5
    assert batched.best_score == pytest.approx(looped.best_score, abs=1e-5)

    make = lambda a, p: MDSA(a)  # noqa: E731
    sa_l = MultiModalSA.build_with_kmeans(x, None, make, **kw)
    sa_b = MultiModalSA.build_with_kmeans(x, None, make, kmeans_mode="batched", **kw)
    rng = np.random.RandomState(9)
    held = far_blobs[:64] + torch.from_numpy(rng.randn(64, 37).astype(np.float32)) * 0.5
    got, want = sa_b(held.to(_dev())), sa_l(held.to(_dev()))
    torch.testing.assert_close(got, want, rtol=1e-4, atol=0)


def test_envelope_raises():
    dev = _dev()
    x = torch.randn(64, 8, device=dev)

    def seg_of(sizes):
        return torch.tensor(np.cumsum([0] + list(sizes)), dtype=torch.int32, device=dev)

    def call_all(xx, sizes, seg=None):
        seg = seg_of(sizes) if seg is None else seg
        p, c = len(sizes), int(sum(sizes))
        centers = torch.randn(c, 8, device=dev)
        labels = torch.zeros(p, 64, dtype=torch.int32, device=dev)
        active = torch.ones(p, dtype=torch.int32, device=dev)
        for fn in (
            lambda: ops.lloyd_assign_many(xx, centers, seg),
            lambda: ops.lloyd_update_many(xx, labels, centers, seg, active),
            lambda: ops.silhouette_cluster_sums(xx, labels, seg),
        ):
            with pytest.raises(ValueError):
                fn()

    call_all(x, [2] * 65)                     # P = 65
    call_all(x, [2, 17])                      # 17 centres in a problem
    call_all(x, [16] * 17)                    # C = 272
    call_all(x.t().contiguous().t(), [2, 3])  # non-contiguous x
    call_all(x.double(), [2, 3])              # not float32
    call_all(x, [2, 3], seg=torch.tensor([0, 5, 2], dtype=torch.int32, device=dev))
    call_all(x, [2, 3], seg=torch.tensor([0, 2, 5], dtype=torch.int32))  # seg on CPU
