"""Small-plane path of the fused ResNet convs and the 8x8x64 LDS image (GPU).

The convs that write an 8x8x64 plane deal their 4 x 4 (pixel tile, cout
tile) grid to the waves in their own way (2 x 2 per wave), and the 8x8x64
LDS image has padded rows. These tests pin the tile, tap and layout mapping
whatever the dealing and the strides are, with weights whose
result torch can state exactly (zero, one-hot identity, channel permutation,
channel duplication), so every comparison but the last is bit for bit, and
none depends on the recorded golden forward. Every case runs on the
per-block ops and inside the stage kernels (the other blocks of the stage
get all-zero weights, which makes them relu(x)).
"""

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

BATCHES = (1, 3, 7)
TAPS = [(dy, dx) for dy in range(3) for dx in range(3)]
DEV = "cuda:0"


@pytest.fixture(scope="module")
def ext():
    from simple_tip_amd.ops import _load_compiled

    return _load_compiled()


def _pack(w):
    from simple_tip_amd.models.resnet_fused import _pack_conv

    taps = w.shape[2] * w.shape[3]
    return _pack_conv(w.float(), taps).reshape(-1, 8).to(DEV)


def _distinct(b, h, c):
    """[b, h, h, c] bf16: within an image every (pixel, channel) holds a
    distinct bf16 value (1 + m/128) * 2**e, about a third of them negative;
    image i is image 0 rolled by 37 * i elements."""
    n = h * h * c
    idx = torch.arange(n)
    m = idx % 128
    e = idx // 128 - n // 256
    mag = (1 + m.double() / 128) * torch.exp2(e.double())
    sign = torch.where((idx * 7 + idx // c) % 3 == 0, -1.0, 1.0)
    # scatter so that neighbouring pixels and channels are unrelated
    assert n & (n - 1) == 0  # a power of two: an odd multiplier permutes
    v = (mag * sign)[(idx * 1657 + 11) % n]
    assert torch.unique(v).numel() == n
    x = torch.stack([torch.roll(v, 37 * i) for i in range(b)])
    xb = x.to(torch.bfloat16)
    assert torch.equal(xb.double(), x), "values must be exact in bf16"
    return xb.reshape(b, h, h, c)


def _zeros_w(cout, cin, k=3):
    return torch.zeros(cout, cin, k, k)


def _tap_identity(cout, cin, dy, dx):
    """W[co, co % cin, dy, dx] = 1: output channel co copies input channel
    co % cin at tap (dy, dx)."""
    w = _zeros_w(cout, cin)
    co = torch.arange(cout)
    w[co, co % cin, dy, dx] = 1.0
    return w


def _shift(h, dy, dx, stride=1):
    """What a one-hot conv at tap (dy, dx), pad 1, reads: out[y, x] =
    h[stride * y + dy - 1, stride * x + dx - 1], zero outside. NHWC."""
    hp = F.pad(h, (0, 0, 1, 1, 1, 1))
    n = h.shape[1]
    return hp[:, dy:dy + n:stride, dx:dx + n:stride]


def _bf16_sum_relu(a, b):
    """bf16(relu(fp32(a + b))) of two bf16 tensors: the conv2 epilogue."""
    return (a.float() + b.float()).clamp_min(0).to(torch.bfloat16)


def _zero_bias(c):
    return torch.zeros(c, device=DEV)


def _res_block(ext, x, w1, b1, w2, b2):
    """res<8,8,64> on the per-block op."""
    b = x.shape[0]
    out = ext.resnet_block(2, x.reshape(b, -1).to(DEV), _pack(w1), b1.to(DEV),
                           _pack(w2), b2.to(DEV))
    return out.reshape(b, 8, 8, 64).cpu()


def _res_block_stage3(ext, x, w1, b1, w2, b2):
    """The same block as the first of stage 3; the second has zero weights,
    so it returns relu of the (already non-negative) first block's output."""
    b = x.shape[0]
    z, zb = _pack(_zeros_w(64, 64)), _zero_bias(64)
    params = [_pack(w1), b1.to(DEV), _pack(w2), b2.to(DEV), z, zb, z, zb,
              torch.zeros(10, 64, device=DEV), torch.zeros(10, device=DEV)]
    ats, logits = ext.resnet_stage3(x.reshape(b, -1).to(DEV), params)
    assert logits.shape == (b, 10)
    return ats.reshape(b, 8, 8, 64).cpu()


RES_PATHS = {"block": _res_block, "stage3": _res_block_stage3}


def _down_block(ext, x, w1, w2, wsc):
    b = x.shape[0]
    zb = _zero_bias(64)
    out = ext.resnet_down(1, x.reshape(b, -1).to(DEV), _pack(w1), zb,
                          _pack(w2), zb, _pack(wsc), zb)
    return out.reshape(b, 8, 8, 64).cpu()


def _down_block_stage2(ext, x, w1, w2, wsc):
    """The down block at the end of stage 2, behind two zero-weight res
    blocks: it sees relu(x), so the caller passes a non-negative x."""
    assert (x.float() >= 0).all()
    b = x.shape[0]
    z, zb32, zb = _pack(_zeros_w(32, 32)), _zero_bias(32), _zero_bias(64)
    params = [z, zb32, z, zb32] * 2 + [_pack(w1), zb, _pack(w2), zb,
                                       _pack(wsc), zb]
    out = ext.resnet_stage2(x.reshape(b, -1).to(DEV), params)
    return out.reshape(b, 8, 8, 64).cpu()


@pytest.mark.parametrize("path", sorted(RES_PATHS))
def test_layout_round_trip(ext, path):
    """Zero weights and biases: the block is relu(x). Pins load, store,
    residual and halo of the 8x8x64 image."""
    zw, zb = _zeros_w(64, 64), torch.zeros(64)
    for b in BATCHES:
        x = _distinct(b, 8, 64)
        got = RES_PATHS[path](ext, x, zw, zb, zw, zb)
        assert torch.equal(got, x.clamp_min(0)), b
        assert got.float().abs().sum() > 0


@pytest.mark.parametrize("path", sorted(RES_PATHS))
@pytest.mark.parametrize("tap", TAPS)
def test_tap_and_tile_mapping(ext, path, tap):
    """conv1 = centre identity, conv2 = identity at one tap: the output is
    bf16(relu(shift_t(relu(x)) + x)), border pixels included."""
    zb = torch.zeros(64)
    w1 = _tap_identity(64, 64, 1, 1)
    w2 = _tap_identity(64, 64, *tap)
    for b in BATCHES:
        x = _distinct(b, 8, 64)
        want = _bf16_sum_relu(_shift(x.clamp_min(0), *tap), x)
        got = RES_PATHS[path](ext, x, w1, zb, w2, zb)
        assert torch.equal(got, want), (b, tap)


@pytest.mark.parametrize("path", sorted(RES_PATHS))
def test_cout_tile_mapping(ext, path):
    """conv2 = centre-tap permutation that takes every output channel from
    another 16-channel tile."""
    zb = torch.zeros(64)
    co = torch.arange(64)
    r = co % 16
    src = ((co // 16 + 1 + r % 3) % 4) * 16 + (r * 5 + 3) % 16
    assert ((src // 16) != (co // 16)).all() and torch.unique(src).numel() == 64
    w1 = _tap_identity(64, 64, 1, 1)
    w2 = _zeros_w(64, 64)
    w2[co, src, 1, 1] = 1.0
    for b in BATCHES:
        x = _distinct(b, 8, 64)
        want = _bf16_sum_relu(x.clamp_min(0)[..., src], x)
        got = RES_PATHS[path](ext, x, w1, zb, w2, zb)
        assert torch.equal(got, want), b


DOWN_PATHS = {"block": _down_block, "stage2": _down_block_stage2}


def _down_input(b, path):
    x = _distinct(b, 16, 32)
    # stage 2 feeds the down block relu(x); keep the values distinct there
    return x.abs() if path == "stage2" else x


@pytest.mark.parametrize("path", sorted(DOWN_PATHS))
def test_down_block_shortcut_only(ext, path):
    """Zero 3x3 weights, 1x1 shortcut = channel duplication 32 -> 64: the
    output is relu(x[:, ::2, ::2]) twice along the channels."""
    dup = _zeros_w(64, 32, 1)
    co = torch.arange(64)
    dup[co, co % 32, 0, 0] = 1.0
    for b in BATCHES:
        x = _down_input(b, path)
        want = x[:, ::2, ::2].clamp_min(0).repeat(1, 1, 1, 2)
        got = DOWN_PATHS[path](ext, x, _zeros_w(64, 32), _zeros_w(64, 64), dup)
        assert torch.equal(got, want), b
        assert got.float().abs().sum() > 0


@pytest.mark.parametrize("path", sorted(DOWN_PATHS))
@pytest.mark.parametrize("tap", TAPS)
def test_down_block_stride2_gather(ext, path, tap):
    """conv1 = one-hot at one tap (stride 2, 32 -> 64 by duplication), conv2
    = centre identity, shortcut = duplication: the output is
    bf16(relu(relu(x[2y + dy - 1, 2x + dx - 1]) + x[2y, 2x]))."""
    dup = _zeros_w(64, 32, 1)
    co = torch.arange(64)
    dup[co, co % 32, 0, 0] = 1.0
    w1 = _tap_identity(64, 32, *tap)
    w2 = _tap_identity(64, 64, 1, 1)
    for b in BATCHES:
        x = _down_input(b, path)
        h = _shift(x, *tap, stride=2).clamp_min(0).repeat(1, 1, 1, 2)
        sc = x[:, ::2, ::2].repeat(1, 1, 1, 2)
        want = _bf16_sum_relu(h, sc)
        got = DOWN_PATHS[path](ext, x, w1, w2, dup)
        assert torch.equal(got, want), (b, tap)


def _conv64(x_nhwc, w):
    """float64 3x3 pad-1 convolution, NHWC in and out."""
    y = F.conv2d(x_nhwc.double().permute(0, 3, 1, 2), w.double(), padding=1)
    return y.permute(0, 2, 3, 1)


@pytest.mark.parametrize("path", sorted(RES_PATHS))
@pytest.mark.parametrize("random_convs", ["conv1", "conv2", "both"])
def test_random_weights_within_fp32_bound(ext, path, random_convs):
    """A random-weight block against float64 convolutions of the
    bf16-rounded operands.

    Bound, with u = 2**-24 and gamma = K u / (1 - K u) at K = 576 (the form
    tests/test_gpu_resnet_stage_fused.py uses): a conv's accumulator is a
    chain of K fp32 additions of exact bf16 x bf16 products from zero, the
    bias is one more, so |fp32 - exact| <= gamma * (|w| * |in| + |b|) (the
    first addition, to zero, is exact, which leaves K roundings). conv2's
    residual addition is one further rounding, u * |value|. Every output is
    then rounded to bf16 (8 significant bits): 2**-8 relative. conv1's error e1 reaches conv2 as
    |w2| * e1 (relu is 1-Lipschitz)."""
    u, ub = 2.0 ** -24, 2.0 ** -8
    k = 576
    gamma = k * u / (1 - k * u)
    g = torch.Generator().manual_seed(14)

    def rand_w():
        w = torch.randn(64, 64, 3, 3, generator=g) / 24.0
        return w.to(torch.bfloat16).float()

    ident = _tap_identity(64, 64, 1, 1)
    w1 = rand_w() if random_convs in ("conv1", "both") else ident
    w2 = rand_w() if random_convs in ("conv2", "both") else ident
    b1 = torch.randn(64, generator=g) * 0.1
    b2 = torch.randn(64, generator=g) * 0.1
    for b in BATCHES:
        x = torch.randn(b, 8, 8, 64, generator=g).to(torch.bfloat16)
        got = RES_PATHS[path](ext, x, w1, b1, w2, b2).double()
        # conv1 + bias + relu -> bf16
        c1 = _conv64(x, w1) + b1.double()
        e_acc1 = gamma * (_conv64(x.abs(), w1.abs()) + b1.double().abs())
        h = c1.clamp_min(0)
        e1 = e_acc1 + ub * (h + e_acc1)
        # conv2 + bias + residual + relu -> bf16
        c2 = _conv64(h, w2) + b2.double()
        e_in = _conv64(e1, w2.abs())
        mag2 = _conv64(h + e1, w2.abs()) + b2.double().abs()
        e_acc2 = e_in + gamma * mag2
        v = c2 + x.double()
        e_v = e_acc2 + u * (v.abs() + e_acc2)
        ref = v.clamp_min(0)
        bound = e_v + ub * (ref + e_v)
        ratio = ((got - ref).abs() / bound.clamp_min(1e-300)).reshape(b, -1)
        rows = ratio.max(dim=1).values
        print(f"{path} {random_convs} b={b}: max |dev| "
              f"{float((got - ref).abs().max()):.3e}, max dev/bound "
              f"{float(rows.max()):.4f}")
        assert rows.shape == (b,) and torch.isfinite(ratio).all(), "row skipped"
        assert (ref.reshape(b, -1).abs().sum(dim=1) > 0).all(), "empty row"
        assert (bound > 0).all()
        assert float(rows.max()) <= 1.0, (b, rows.tolist())
