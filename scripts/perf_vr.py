"""MC-dropout variation ratio: replay vs the fused head, on the MNIST geometry.

Times, on one GPU and in one process:
  - ``BaseModel(vr_mode="replay")`` and ``vr_mode="fused"`` end to end
    (``_variation_ratio`` on N = 10000 inputs, MnistCNN, S = 200), the two
    modes alternating over ``--reps`` repetitions after one warm-up each;
  - the ``mc_dropout_votes`` kernel alone on [N, 1600] x [10, 1600], on the
    model's own trunk features and on two synthetic feature sets that bound
    the zero-skip (relu(randn): half zero; |randn|: no zeros);
  - the ``mc_dropout_stats`` kernel (votes + mean softmax + mean entropy) on
    the same three feature sets, each right after its votes timing.

Every window ends in a device synchronise. Prints one JSON line.

  python scripts/perf_vr.py [--n 10000] [--reps 5] [--kernel-iters 20]
"""

import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from simple_tip_amd import ops  # noqa: E402
from simple_tip_amd.config import DROPOUT_SAMPLE_SIZE  # noqa: E402
from simple_tip_amd.engine.model_handler import BaseModel  # noqa: E402
from simple_tip_amd.models import MnistCNN  # noqa: E402
from simple_tip_amd.studies.synthetic import synthetic_images  # noqa: E402


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1000.0, out


def kernel_ms(feats, weight, bias, iters, op=ops.mc_dropout_votes):
    """Median device-event time of one mc_dropout_votes / _stats call."""
    call = lambda: op(  # noqa: E731
        feats, weight, bias, 0.5, DROPOUT_SAMPLE_SIZE, 0
    )
    call()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        start = torch.cuda.Event(enable_timing=True)
        stop = torch.cuda.Event(enable_timing=True)
        start.record()
        call()
        stop.record()
        stop.synchronize()
        times.append(start.elapsed_time(stop))
    return statistics.median(times), min(times), max(times)


def spread(xs):
    return {
        "median_ms": round(statistics.median(xs), 3),
        "min_ms": round(min(xs), 3),
        "max_ms": round(max(xs), 3),
        "all_ms": [round(x, 3) for x in xs],
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kernel-iters", type=int, default=20)
    ap.add_argument("--predict-batch", type=int, default=512)
    args = ap.parse_args()

    assert torch.cuda.is_available(), "perf_vr.py needs a GPU"
    assert ops.hip_available(), "perf_vr.py requires the _tip_hip extension"
    from simple_tip_amd.ops import hip_ops
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = MnistCNN().to(dev)
    x_np, _ = synthetic_images("perf_vr_mnist", "test", args.n, (1, 28, 28), 10)
    x = torch.from_numpy(x_np)

    replay = BaseModel(model, None, device=dev, predict_batch=args.predict_batch,
                       vr_mode="replay")
    fused = BaseModel(model, None, device=dev, predict_batch=args.predict_batch,
                      vr_mode="fused", vr_seed=0)

    # warm-up: code objects, MIOpen algorithm choice, allocator
    _, vr_r = wall_ms(lambda: replay._variation_ratio(x)[0])
    _, vr_f = wall_ms(lambda: fused._variation_ratio(x)[0])
    t_replay, t_fused = [], []
    for _ in range(args.reps):
        t_replay.append(wall_ms(lambda: replay._variation_ratio(x))[0])
        t_fused.append(wall_ms(lambda: fused._variation_ratio(x))[0])

    # kernel alone
    k, _, lin = model.dropout_head()
    with torch.no_grad():
        h = x[: args.n].to(dev)
        parts = []
        for s0 in range(0, h.shape[0], 2048):
            t = h[s0 : s0 + 2048]
            for layer in model.layers[:k]:
                t = layer(t)
            parts.append(t.float())
        trunk_feats = torch.cat(parts).contiguous()
    weight = lin.weight.detach().float().contiguous()
    bias = lin.bias.detach().float().contiguous()
    g = torch.Generator(device="cpu").manual_seed(1)
    randn = torch.randn(args.n, lin.in_features, generator=g).to(dev)
    feature_sets = {
        "trunk": trunk_feats,
        "relu_randn": torch.relu(randn),
        "abs_randn": randn.abs(),
    }
    kernel = {}
    kernel_stats = {}
    for name, feats in feature_sets.items():
        med, lo, hi = kernel_ms(feats, weight, bias, args.kernel_iters)
        kernel[name] = {
            "nonzero_fraction": round(float((feats != 0).float().mean()), 4),
            "median_ms": round(med, 3),
            "min_ms": round(lo, 3),
            "max_ms": round(hi, 3),
        }
        med_s, lo_s, hi_s = kernel_ms(
            feats, weight, bias, args.kernel_iters, op=ops.mc_dropout_stats
        )
        kernel_stats[name] = {
            "median_ms": round(med_s, 3),
            "min_ms": round(lo_s, 3),
            "max_ms": round(hi_s, 3),
            "over_votes": round(med_s / med, 3),
        }

    med_r = statistics.median(t_replay)
    med_f = statistics.median(t_fused)
    result = {
        "script": "perf_vr",
        "device": torch.cuda.get_device_name(0),
        "n": args.n,
        "samples": DROPOUT_SAMPLE_SIZE,
        "predict_batch": args.predict_batch,
        "reps": args.reps,
        "replay": spread(t_replay),
        "fused": spread(t_fused),
        "speedup_median": round(med_r / med_f, 2),
        "speedup_worst_case": round(min(t_replay) / max(t_fused), 2),
        "kernel": kernel,
        "kernel_stats": kernel_stats,
        "mean_vr_replay": round(float(vr_r.mean()), 4),
        "mean_vr_fused": round(float(vr_f.mean()), 4),
        "launch": hip_ops.mc_dropout_launch_config(
            lin.in_features, lin.out_features
        ),
    }
    print(json.dumps(result))


if __name__ == "__main__":
    main()
