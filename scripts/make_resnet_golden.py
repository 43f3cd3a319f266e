"""Record the fused ResNet-20 forward's bits as a golden file (GPU).

Run once on a build whose results are to be pinned:

    python scripts/make_resnet_golden.py [tests/golden/resnet_forward_parent.npz]

The weights follow tests/test_gpu_resnet_fused.py::folded_pair (seed 0,
randomised BN statistics); the batch is six fp32 NHWC images: all zero,
all +100, all -100, values on bf16 rounding ties, and two randn images.
The file holds the stage path's ATs (bf16 bits) and logits, the sha256 of
each stage's output plane, and the sha256 of the packed weights and of the
inputs, so a reader can tell a changed recipe from a changed kernel.
tests/test_gpu_resnet_conv_epilogue.py imports the recipe from here.
"""

import hashlib
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

GOLDEN = os.path.join(REPO, "tests", "golden", "resnet_forward_parent.npz")


def build_fused(device):
    """FusedResNet20 on the folded_pair weight recipe."""
    from simple_tip_amd.models import ResNet20
    from simple_tip_amd.models.fuse import fold_bn_inference
    from simple_tip_amd.models.resnet_fused import FusedResNet20

    torch.manual_seed(0)
    m = ResNet20()
    for mod in m.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.running_mean.normal_(0, 0.2)
            mod.running_var.uniform_(0.5, 2.0)
            mod.weight.data.uniform_(0.5, 1.5)
            mod.bias.data.normal_(0, 0.2)
    return FusedResNet20(fold_bn_inference(m), device)


def build_inputs():
    """[6, 32, 32, 3] fp32 NHWC, on the CPU."""
    g = torch.Generator().manual_seed(9)
    shape = (32, 32, 3)
    pick = torch.randint(0, 2, shape, generator=g).bool()
    sign = torch.randint(0, 2, shape, generator=g).float() * 2 - 1
    # 1 + 2**-8 and 1 + 3 * 2**-8 lie halfway between bf16 neighbours
    ties = torch.where(pick, torch.tensor(1 + 2.0 ** -8),
                       torch.tensor(1 + 3 * 2.0 ** -8)) * sign
    return torch.stack([
        torch.zeros(shape),
        torch.full(shape, 100.0),
        torch.full(shape, -100.0),
        ties,
        torch.randn(shape, generator=g),
        torch.randn(shape, generator=g),
    ]).contiguous()


def sha(t):
    """sha256 of a tensor's bytes (bf16 as its 16-bit patterns)."""
    t = t.detach().cpu().contiguous()
    if t.dtype == torch.bfloat16:
        t = t.view(torch.int16)
    return hashlib.sha256(t.numpy().tobytes()).hexdigest()


def weights_sha(fused):
    """One sha256 over every packed weight and bias, in forward order."""
    h = hashlib.sha256()
    for params in fused.stage_params:
        for t in params:
            h.update(sha(t).encode())
    return h.hexdigest()


def stage_path(fused, x):
    """The three stage launches; returns (plane1, plane2, ats, logits)."""
    p1 = fused.ext.resnet_stage1(x, fused.stage_params[0])
    p2 = fused.ext.resnet_stage2(p1, fused.stage_params[1])
    ats, logits = fused.ext.resnet_stage3(p2, fused.stage_params[2])
    return p1, p2, ats, logits


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    dev = torch.device("cuda:0")
    fused = build_fused(dev)
    x = build_inputs()
    p1, p2, ats, logits = stage_path(fused, x.to(dev))
    torch.cuda.synchronize()
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    np.savez_compressed(
        out,
        ats_bits=ats.cpu().view(torch.int16).numpy(),
        logits=logits.cpu().numpy(),
        plane_sha=np.array([sha(p1), sha(p2), sha(ats)]),
        weights_sha=np.array(weights_sha(fused)),
        inputs_sha=np.array(sha(x)),
    )
    print(f"wrote {out}: {os.path.getsize(out)} bytes, "
          f"ats nonzero {int((ats != 0).sum())} of {ats.numel()}, "
          f"weights {weights_sha(fused)[:16]}")


if __name__ == "__main__":
    main()
