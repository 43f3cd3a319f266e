"""Operand-swapped MFMA + packed epilogue of the fused ResNet convs (GPU).

The convs pass the weight fragment as the first MFMA operand and the pixel
fragment as the second, so a lane's 4 accumulator registers are 4
consecutive couts of one pixel and the epilogue stores 8 bytes at once.
Two things must hold for that to change no output bit:

- the gate: v_mfma_f32_16x16x32_bf16 gives the same fp32 bits for B^T A^T
  as for A B (checked through the unchanged ``mfma_probe``);
- parity: the forward reproduces the bits recorded from the build before the
  change (tests/golden/resnet_forward_parent.npz, written by
  scripts/make_resnet_golden.py), on the stage path and the per-block path.
"""

import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _recipe():
    spec = importlib.util.spec_from_file_location(
        "make_resnet_golden", os.path.join(REPO, "scripts", "make_resnet_golden.py")
    )
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _bf16_scaled(rng, shape):
    """randn * 2**k, k uniform in -20..20 per element, rounded to bf16."""
    v = rng.randn(*shape) * np.exp2(rng.randint(-20, 21, size=shape))
    return torch.from_numpy(v.astype(np.float32)).to(torch.bfloat16)


def _gate_pairs():
    rng = np.random.RandomState(3)
    pairs = [("scaled", _bf16_scaled(rng, (16, 32)), _bf16_scaled(rng, (32, 16)))]
    # heavy cancellation: k = 2i and 2i + 1 carry the same product with
    # opposite signs at magnitudes 2**-20 .. 2**20, plus one small term per
    # output that survives only if nothing was lost on the way
    a = _bf16_scaled(rng, (16, 32))
    b = _bf16_scaled(rng, (32, 16))
    a[:, 1::2] = a[:, 0::2]
    b[1::2, :] = -b[0::2, :]
    a[:, 31] = torch.from_numpy(rng.randn(16).astype(np.float32)).to(torch.bfloat16)
    b[31, :] = torch.from_numpy(
        (rng.randn(16) * 2.0 ** -12).astype(np.float32)).to(torch.bfloat16)
    pairs.append(("cancel", a, b))
    return {name: (a, b) for name, a, b in pairs}


@pytest.mark.parametrize("name", ["scaled", "cancel"])
def test_gate_swapped_operands_same_bits(name):
    from simple_tip_amd.ops import _load_compiled

    ext = _load_compiled()
    a, b = (t.cuda() for t in _gate_pairs()[name])
    d = ext.mfma_probe(a, b)
    dt = ext.mfma_probe(b.t().contiguous(), a.t().contiguous())
    assert d.shape == (16, 16) and torch.isfinite(d).all()
    assert d.abs().sum() > 0
    same = torch.equal(dt.t(), d)
    if not same:
        bad = (dt.t() != d).nonzero()[0].tolist()
        print(f"{name}: first differing element {bad}: "
              f"{float(d[bad[0], bad[1]])!r} vs {float(dt[bad[1], bad[0]])!r}")
    assert same


@pytest.fixture(scope="module")
def parity():
    """The recipe's model and inputs, the golden file, and both paths' results,
    computed once."""
    rec = _recipe()
    assert os.path.exists(rec.GOLDEN), f"{rec.GOLDEN} is missing: regenerate"
    gold = np.load(rec.GOLDEN)
    dev = torch.device("cuda:0")
    fused = rec.build_fused(dev)
    x = rec.build_inputs()
    assert rec.weights_sha(fused) == str(gold["weights_sha"]), (
        "the packed weights differ from the recorded ones: regenerate "
        "tests/golden/resnet_forward_parent.npz with scripts/make_resnet_golden.py"
    )
    assert rec.sha(x) == str(gold["inputs_sha"]), "inputs differ: regenerate"
    xd = x.to(dev)
    p1, p2, ats, logits = rec.stage_path(fused, xd)
    os.environ["TIP_NO_STAGE_FUSED"] = "1"
    try:
        calls = fused.stage_fused_calls
        block_ats, _ = fused.forward_nhwc(xd)
        assert fused.stage_fused_calls == calls, "took the stage path"
    finally:
        del os.environ["TIP_NO_STAGE_FUSED"]
    torch.cuda.synchronize()
    return dict(rec=rec, gold=gold, planes=(p1, p2, ats), ats=ats,
                logits=logits, block_ats=block_ats)


def _gold_ats(gold):
    return torch.from_numpy(gold["ats_bits"]).view(torch.bfloat16)


def test_stage_path_bits_equal_parent(parity):
    gold = parity["gold"]
    want = _gold_ats(gold)
    assert want.shape == (6, 4096) and want.float().abs().sum() > 0
    assert torch.equal(parity["ats"].cpu(), want)
    assert torch.equal(parity["logits"].cpu(), torch.from_numpy(gold["logits"]))


def test_stage_planes_hash_equal_parent(parity):
    rec = parity["rec"]
    for i, (plane, want) in enumerate(zip(parity["planes"], parity["gold"]["plane_sha"])):
        assert rec.sha(plane) == str(want), f"stage {i + 1} output plane"


def test_block_path_bits_equal_parent(parity):
    assert torch.equal(parity["block_ats"].cpu(), _gold_ats(parity["gold"]))
