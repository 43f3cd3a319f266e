"""Microbenchmark of the fused ResNet-20 forward (gfx950).

Times every per-block kernel and the torch glue alone, then each
stage-resident kernel against the chain of launches it replaces (same
process, alternating, device events), and prints the achieved TB/s and TF
of the stage kernels from the bytes and FLOPs their shapes need.

Usage: python scripts/perf_fused_resnet.py [batch] [rounds] [--stages-only]

--stages-only runs nothing but the three stage kernels (one untimed round,
then 10 calls per round after 2 warm-up calls): the short run to put under a profiler's counters,
and the per-stage timing of an A/B comparison.
"""

import statistics
import sys

import torch

sys.path.insert(0, ".")
from simple_tip_amd.models import ResNet20  # noqa: E402
from simple_tip_amd.models.fuse import fold_bn_inference  # noqa: E402
from simple_tip_amd.models.resnet_fused import FusedResNet20  # noqa: E402


def timeit(fn, iters=10, warmup=2):
    """Mean ms per call over `iters` calls, by device events."""
    for _ in range(warmup):
        fn()
    start = torch.cuda.Event(enable_timing=True)
    end = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def conv_flops(h, w, cin, cout, taps=9):
    return 2 * h * w * taps * cin * cout


def res_flops(h, c):
    return 2 * conv_flops(h, h, c, c)


def down_flops(h, c):
    o = h // 2
    return (conv_flops(o, o, c, 2 * c) + conv_flops(o, o, 2 * c, 2 * c)
            + conv_flops(o, o, c, 2 * c, taps=1))


# per image: (FLOPs, HBM bytes in + out) of each stage kernel, from the shapes
STAGE_WORK = {
    "stage1": (conv_flops(32, 32, 3, 16) + 3 * res_flops(32, 16) + down_flops(32, 16),
               32 * 32 * 3 * 4 + 16 * 16 * 32 * 2),
    "stage2": (2 * res_flops(16, 32) + down_flops(16, 32),
               16 * 16 * 32 * 2 + 8 * 8 * 64 * 2),
    "stage3": (2 * res_flops(8, 64) + 2 * 64 * 64 + 2 * 64 * 10,
               2 * 8 * 8 * 64 * 2 + 10 * 4),
}


def stages_alone(fused, x, b, rounds):
    """Time the three stage kernels alone, each on the plane before it."""
    ext = fused.ext
    p1, p2, p3 = fused.stage_params
    plane1 = ext.resnet_stage1(x, p1)
    plane2 = ext.resnet_stage2(plane1, p2)
    calls = [
        ("stage1", lambda: ext.resnet_stage1(x, p1)),
        ("stage2", lambda: ext.resnet_stage2(plane1, p2)),
        ("stage3", lambda: ext.resnet_stage3(plane2, p3)),
    ]
    times = {name: [] for name, _ in calls}
    for name, fn in calls:  # one untimed round: clocks and caches settle
        timeit(fn)
    for _ in range(rounds):
        for name, fn in calls:
            times[name].append(timeit(fn))
    for name, _ in calls:
        ts = times[name]
        ms = statistics.median(ts)
        flops, nbytes = STAGE_WORK[name]
        print(f"{name}: fused {ms:.3f} ms ({min(ts):.3f} - {max(ts):.3f}); "
              f"{flops * b / ms / 1e9:.0f} TF, {nbytes * b / ms / 1e9:.2f} TB/s")


def main():
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    argv = [a for a in sys.argv[1:] if a != "--stages-only"]
    stages_only = "--stages-only" in sys.argv[1:]
    b = int(argv[0]) if len(argv) > 0 else 20480
    rounds = int(argv[1]) if len(argv) > 1 else 5
    model = fold_bn_inference(ResNet20()).to(dev)
    fused = FusedResNet20(model, dev)
    ext = fused.ext
    x = torch.randn(b, 32, 32, 3, device=dev)
    print(f"batch {b}, {rounds} alternating rounds of 10 calls")
    if stages_only:
        stages_alone(fused, x, b, rounds)
        return

    # ---- the per-block chain, piece by piece ----
    def glue_in():
        nhwc = torch.zeros(b, 32, 32, 8, device=dev, dtype=torch.bfloat16)
        nhwc[..., :3] = x.to(torch.bfloat16)
        return nhwc.reshape(b, -1).contiguous()

    def stem(xin):
        return ext.resnet_stem(xin, fused.stem_w.reshape(-1, 8), fused.stem_b)

    def block(i, cur):
        blk = fused.blocks[i]
        args = [t.reshape(-1, 8) if t.dtype == torch.bfloat16 else t for t in blk[2:]]
        op = ext.resnet_block if blk[0] == "res" else ext.resnet_down
        return op(blk[1], cur, *args)

    def glue_out(cur):
        pooled = cur.reshape(b, 64, 64).float().mean(dim=1)
        return pooled @ fused.fc_w.t() + fused.fc_b

    xin = glue_in()
    planes = [stem(xin)]
    for i in range(9):
        planes.append(block(i, planes[-1]))
    print(f"  glue in (zeros + cast + slice-assign): {timeit(glue_in):.3f} ms")
    print(f"  stem: {timeit(lambda: stem(xin)):.3f} ms")
    for i in range(9):
        kind = fused.blocks[i][0]
        print(f"  block{i} ({kind}): {timeit(lambda: block(i, planes[i])):.3f} ms")
    print(f"  glue out (float + mean + fc): {timeit(lambda: glue_out(planes[9])):.3f} ms")

    # ---- each stage kernel against the chain it replaces ----
    def chain1():
        cur = stem(glue_in())
        for i in range(4):
            cur = block(i, cur)
        return cur

    def chain2():
        cur = planes[4]
        for i in range(4, 7):
            cur = block(i, cur)
        return cur

    def chain3():
        cur = planes[7]
        for i in range(7, 9):
            cur = block(i, cur)
        return cur, glue_out(cur)

    p1, p2, p3 = fused.stage_params
    pairs = [
        ("stage1", chain1, lambda: ext.resnet_stage1(x, p1)),
        ("stage2", chain2, lambda: ext.resnet_stage2(planes[4], p2)),
        ("stage3", chain3, lambda: ext.resnet_stage3(planes[7], p3)),
    ]

    def old_forward():
        cur = stem(glue_in())
        for i in range(9):
            cur = block(i, cur)
        return cur, glue_out(cur)

    pairs.append(("forward", old_forward, lambda: fused.forward_nhwc(x)))

    for name, chain, stage in pairs:
        tc, ts = [], []
        for _ in range(rounds):
            tc.append(timeit(chain))
            ts.append(timeit(stage))
        mc, ms = statistics.median(tc), statistics.median(ts)
        line = (f"{name}: chain {mc:.3f} ms ({min(tc):.3f} - {max(tc):.3f}), "
                f"fused {ms:.3f} ms ({min(ts):.3f} - {max(ts):.3f}), "
                f"ratio {mc / ms:.3f}")
        if name in STAGE_WORK:
            flops, nbytes = STAGE_WORK[name]
            line += (f"; fused kernel {flops * b / ms / 1e9:.0f} TF, "
                     f"{nbytes * b / ms / 1e9:.2f} TB/s")
        print(line)


if __name__ == "__main__":
    main()
