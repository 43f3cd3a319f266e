"""Grouped DSA + per-class LSA scoring in isolation: host-planned bf16 path
vs the sync-free path (device segment plan, gathered kernels).

Synthetic class-structured activation traces at the benchmark's shapes
(50000-row fit, 0.3 DSA subsample, 300 LSA features, batch 20480 x 4096).
Each path is timed with device events around whole calls; kernel launches
per call are counted with the torch profiler in a separate pass.

Usage: python scripts/perf_scoring.py [--train-n N] [--batch B] [--width D]
                                      [--classes C] [--iters K]
Prints one JSON line per path and a final ratio line. Needs a GPU.
"""

import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from simple_tip_amd.core.surprise import DSA, LSA, MultiModalSA  # noqa: E402
from simple_tip_amd.engine.serving import FusedPrioritizer  # noqa: E402


def synthetic(n, width, classes, seed, dev):
    """Class-structured traces: ReLU(class mean + noise), bf16 like the
    fused forward's tap."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    means = torch.randn(classes, width, generator=g) * 0.5
    pred = torch.randint(0, classes, (n,), generator=g)
    parts = []
    for s in range(0, n, 8192):
        p = pred[s : s + 8192]
        x = means[p] + torch.randn(p.shape[0], width, generator=g)
        parts.append(torch.relu(x).to(dev))
    return torch.cat(parts), pred.to(dev)


def time_calls(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return times


def count_launches(fn):
    """Device kernels and memcpys of one call, from the torch profiler."""
    try:
        from torch.profiler import ProfilerActivity, profile

        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        kernels = memcpy = 0
        for ev in prof.events():
            if str(ev.device_type).endswith("CUDA"):
                name = ev.name.lower()
                if name.startswith(("memcpy", "memset")):
                    memcpy += 1
                else:
                    kernels += 1
        return {"device_events": kernels + memcpy, "memcpy_events": memcpy}
    except Exception as e:  # profiler unavailable: say so, do not guess
        return {"device_events": None, "error": repr(e)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--train-n", type=int, default=50000)
    ap.add_argument("--batch", type=int, default=20480)
    ap.add_argument("--width", type=int, default=4096)
    ap.add_argument("--classes", type=int, default=10)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "perf_scoring needs a GPU"
    dev = torch.device("cuda:0")

    train, tpred = synthetic(args.train_n, args.width, args.classes, 0, dev)
    dsa = DSA(train, tpred, subsampling=0.3, device=dev)
    lsa = MultiModalSA.build_by_class(
        train, tpred, lambda a, p: LSA(a, max_features=300, device=dev)
    )
    del train
    test, pred = synthetic(args.batch, args.width, args.classes, 1, dev)
    test = test.to(torch.bfloat16)

    paths = {
        "old": FusedPrioritizer(dsa, lsa, dev, pairwise_dtype=torch.bfloat16,
                                fast=False),
        "fast": FusedPrioritizer(dsa, lsa, dev, pairwise_dtype=torch.bfloat16),
    }
    assert paths["fast"].fast and not paths["old"].fast
    med = {}
    for name, prio in paths.items():
        times = time_calls(lambda: prio(test, pred), args.iters)
        med[name] = float(np.median(times))
        print(json.dumps({
            "path": name, "batch": args.batch, "width": args.width,
            "train_n": args.train_n, "iters": args.iters,
            "ms_median": med[name], "ms_min": min(times), "ms_max": max(times),
            **count_launches(lambda: prio(test, pred)),
        }), flush=True)
    print(json.dumps({"old_over_fast": med["old"] / med["fast"]}), flush=True)


if __name__ == "__main__":
    main()
