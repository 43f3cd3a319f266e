"""Stage-resident ResNet-20 forward (3 launches) vs the per-block chain (GPU).

The stage kernels reuse the per-block conv code unchanged, so the activation
planes must be bit-identical to the chain of stem / block / down launches;
only the logits may differ, by fp32 summation order.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

BATCHES = (1, 3, 130)


def _special_images():
    """[3, 32, 32, 3]: all-zero, large magnitude (+-100), bf16 rounding ties."""
    g = torch.Generator().manual_seed(7)
    zero = torch.zeros(32, 32, 3)
    sign = torch.randint(0, 2, (32, 32, 3), generator=g).float() * 2 - 1
    large = sign * 100.0
    # 1 + 2**-8 lies halfway between the bf16 neighbours 1 and 1 + 2**-7
    # (rounds to even: 1); 1 + 3 * 2**-8 halfway between 1 + 2**-7 and
    # 1 + 2**-6 (rounds to even: 1 + 2**-6)
    pick = torch.randint(0, 2, (32, 32, 3), generator=g).bool()
    ties = torch.where(pick, torch.tensor(1 + 2.0 ** -8), torch.tensor(1 + 3 * 2.0 ** -8))
    ties = ties * sign
    return torch.stack([zero, large, ties])


def _inputs(b):
    g = torch.Generator().manual_seed(100 + b)
    x = torch.randn(b, 32, 32, 3, generator=g)
    if b >= 3:
        x[:3] = _special_images()
    return x


def _chain(fused, x_nhwc):
    """The per-block chain on an NHWC input of <= 8 channels, op by op:
    returns (stage-1 plane, stage-2 plane, ATs, logits)."""
    ext = fused.ext
    b = x_nhwc.shape[0]
    nhwc = torch.zeros(b, 32, 32, 8, device=x_nhwc.device, dtype=torch.bfloat16)
    nhwc[..., : x_nhwc.shape[-1]] = x_nhwc.to(torch.bfloat16)
    cur = ext.resnet_stem(
        nhwc.reshape(b, -1).contiguous(), fused.stem_w.reshape(-1, 8), fused.stem_b
    )
    planes = []
    for i, blk in enumerate(fused.blocks):
        args = [t.reshape(-1, 8) if t.dtype == torch.bfloat16 else t for t in blk[2:]]
        op = ext.resnet_block if blk[0] == "res" else ext.resnet_down
        cur = op(blk[1], cur, *args)
        if i in (3, 6, 8):
            planes.append(cur)
    pooled = cur.reshape(b, 64, 64).float().mean(dim=1)
    logits = pooled @ fused.fc_w.t() + fused.fc_b
    return planes[0], planes[1], planes[2], logits


@pytest.fixture(scope="module")
def fused():
    from simple_tip_amd.models import ResNet20
    from simple_tip_amd.models.fuse import fold_bn_inference
    from simple_tip_amd.models.resnet_fused import FusedResNet20

    torch.manual_seed(0)
    m = ResNet20()
    # randomize BN stats so folding is non-trivial
    for mod in m.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.running_mean.normal_(0, 0.2)
            mod.running_var.uniform_(0.5, 2.0)
            mod.weight.data.uniform_(0.5, 1.5)
            mod.bias.data.normal_(0, 0.2)
    return FusedResNet20(fold_bn_inference(m), torch.device("cuda:0"))


@pytest.fixture(scope="module")
def runs(fused):
    """Per batch size: the input, the chain's results and the new path's,
    computed once and left unchanged."""
    out = {}
    for b in BATCHES:
        x = _inputs(b).cuda()
        calls = fused.stage_fused_calls
        ats, logits = fused.forward_nhwc(x)
        assert fused.stage_fused_calls == calls + 1
        out[b] = dict(x=x, chain=_chain(fused, x), ats=ats, logits=logits)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("b", BATCHES)
def test_ats_equal_chain(runs, b):
    r = runs[b]
    assert r["ats"].shape == (b, 4096) and r["ats"].dtype == torch.bfloat16
    assert r["logits"].shape == (b, 10) and r["logits"].dtype == torch.float32
    assert torch.equal(r["ats"], r["chain"][2])
    assert r["ats"].float().abs().sum() > 0


@pytest.mark.parametrize("b", BATCHES)
def test_each_stage_equals_its_chain(fused, runs, b):
    """Each stage op alone, fed the chain's plane: a failure names its stage."""
    r = runs[b]
    p1, p2, p3, _ = r["chain"]
    s1 = fused.ext.resnet_stage1(r["x"], fused.stage_params[0])
    assert torch.equal(s1, p1), "stage 1"
    s2 = fused.ext.resnet_stage2(p1, fused.stage_params[1])
    assert torch.equal(s2, p2), "stage 2"
    s3, _ = fused.ext.resnet_stage3(p2, fused.stage_params[2])
    assert torch.equal(s3, p3), "stage 3"


def test_lds_state_position_independent(fused, runs):
    """An image gives the same bits alone and anywhere in a batch of 130
    whose other images are the large-magnitude one (stale halo, region
    reused unzeroed)."""
    large = _special_images()[1]
    singles = _inputs(130)[[0, 2, 5]]  # zero image, ties image, a random one
    for img in singles:
        alone_a, alone_l = fused.forward_nhwc(img[None].cuda().contiguous())
        for pos in (0, 57, 129):
            x = large[None].repeat(130, 1, 1, 1)
            x[pos] = img
            a, l = fused.forward_nhwc(x.cuda())
            assert torch.equal(a[pos], alone_a[0]), pos
            assert torch.equal(l[pos], alone_l[0]), pos


def test_logits_within_fp32_bound(fused, runs):
    """float64 pool + fc of the returned ATs is the reference; the bound is
    that of 130 fp32 roundings on sums of the terms' magnitudes (the tap is
    post-ReLU, so the pool's terms are non-negative)."""
    u = 2.0 ** -24
    gamma = 130 * u / (1 - 130 * u)
    r = runs[130]
    w = fused.fc_w.double()
    bias = fused.fc_b.double()
    pooled = r["ats"].reshape(130, 64, 64).double().mean(dim=1)
    ref = pooled @ w.t() + bias
    bound = gamma * (pooled @ w.abs().t() + bias.abs())
    worst = {}
    for name, got in (("stage", r["logits"]), ("chain", r["chain"][3])):
        dev = (got.double() - ref).abs()
        worst[name] = float((dev / bound.clamp_min(1e-300)).max())
        print(f"logits {name}: max |dev| {float(dev.max()):.3e}, "
              f"max dev/bound {worst[name]:.4f}")
    assert torch.isfinite(ref).all()
    assert worst["chain"] <= 1.0, "the bound itself is wrong"
    assert worst["stage"] <= 1.0


def test_dispatch(fused, runs, monkeypatch):
    r = runs[3]
    x = r["x"]
    want_ats = r["chain"][2]
    want_logits = r["chain"][3]

    def old_path(inp):
        calls = fused.stage_fused_calls
        ats, logits = fused.forward_nhwc(inp)
        assert fused.stage_fused_calls == calls, "took the stage path"
        return ats, logits

    # 4 channels (the 4th has zero stem weights, as every pad channel)
    x4 = torch.cat([x, torch.ones_like(x[..., :1])], dim=-1).contiguous()
    ats, logits = old_path(x4)
    c = _chain(fused, x4)
    assert torch.equal(ats, c[2]) and torch.equal(logits, c[3])
    # bf16 input
    xb = x.to(torch.bfloat16)
    ats, logits = old_path(xb)
    assert torch.equal(ats, want_ats) and torch.equal(logits, want_logits)
    # non-contiguous view of an NCHW tensor
    xs = x.permute(0, 3, 1, 2).contiguous().permute(0, 2, 3, 1)
    assert not xs.is_contiguous()
    ats, logits = old_path(xs)
    assert torch.equal(ats, want_ats) and torch.equal(logits, want_logits)
    # switched off
    monkeypatch.setenv("TIP_NO_STAGE_FUSED", "1")
    ats, logits = old_path(x)
    assert torch.equal(ats, want_ats) and torch.equal(logits, want_logits)
    monkeypatch.delenv("TIP_NO_STAGE_FUSED")
    # the fp32 3-channel contiguous input takes the new path
    calls = fused.stage_fused_calls
    ats, _ = fused.forward_nhwc(x)
    assert fused.stage_fused_calls == calls + 1
    assert torch.equal(ats, want_ats)


def test_graph_capture_and_replay(fused, runs):
    x_a = runs[130]["x"]
    x_b = torch.flip(x_a, dims=[0]).contiguous()
    static_x = torch.zeros_like(x_a)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fused.forward_nhwc(static_x)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ats, logits = fused.forward_nhwc(static_x)
    for x in (x_a, x_b):
        static_x.copy_(x)
        g.replay()
        want_ats, want_logits = fused.forward_nhwc(x)
        assert torch.equal(ats, want_ats)
        assert torch.equal(logits, want_logits)
