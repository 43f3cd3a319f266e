"""Cost of scoring one batch of taps with the 12 configured neuron-coverage
metrics: the per-metric loop (what ``CoverageWorker`` does by default) against
one ``CoverageSuite`` call (``nc_mode="fused"``).

The taps are synthetic post-ReLU activations with the layer widths of the
two studied models; the tables are fitted from a second synthetic batch the
way ``CoverageWorker`` fits them (per-neuron min / max / std). Shapes:

  mnist512    N = 512,   layers 21632 + 5408 + 7744 + 1600   (MNIST CNN)
  resnet512   N = 512,   layers 16384 + 16384 + 8192 + 4096  (ResNet-20)
  mnist10000  N = 10000, the MNIST layers

Whole calls are timed with ``DeviceTimer`` (device drained before and after
each call). After warm-up the two paths alternate for ``--iters`` rounds, so
both see the same machine; median, min and max are reported, and whether
the slowest fused call beat the fastest per-metric call. Before timing, every
word and score of the two paths is compared at the timed size. Kernel
launches per call are counted with the torch profiler.

``--only per_metric`` times that path alone and needs nothing of the suite,
so the same script runs on a build that predates it.

Usage: python scripts/perf_coverage_suite.py [--shape NAME|all] [--iters K]
           [--warmup W] [--only per_metric|fused]
Prints one JSON line per shape. Needs a GPU.
"""

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from simple_tip_amd.core import neuron_coverage as nc  # noqa: E402
from simple_tip_amd.core.timer import DeviceTimer  # noqa: E402

MNIST = (21632, 5408, 7744, 1600)
RESNET = (16384, 16384, 8192, 4096)
SHAPES = {
    "mnist512": dict(n=512, widths=MNIST),
    "resnet512": dict(n=512, widths=RESNET),
    "mnist10000": dict(n=10000, widths=MNIST),
}


def taps(n, widths, seed, dev):
    g = torch.Generator(device=dev).manual_seed(seed)
    return [
        torch.relu(torch.randn(n, w, generator=g, device=dev)) for w in widths
    ]


def canon_metrics(widths, dev):
    """The 12 metrics of CoverageWorker, fitted on a synthetic train batch."""
    train = taps(2048, widths, 1, dev)
    mins = [t.min(dim=0).values for t in train]
    maxs = [t.max(dim=0).values for t in train]
    stds = [t.std(dim=0) for t in train]
    metrics = {}
    for s in (0, 0.5, 1):
        metrics[f"NBC_{s:g}"] = nc.NBC(mins=mins, maxs=maxs, stds=stds, scaler=s)
    for s in (0, 0.5, 1):
        metrics[f"SNAC_{s:g}"] = nc.SNAC(maxs=maxs, stds=stds, scaler=s)
    metrics["NAC_0"] = nc.NAC(cov_threshold=0.0)
    metrics["NAC_0.75"] = nc.NAC(cov_threshold=0.75)
    for k in (1, 2, 3):
        metrics[f"TKNC_{k}"] = nc.TKNC(top_neurons=k)
    metrics["KMNC_2"] = nc.KMNC(mins, maxs, sections=2)
    return metrics


def timed(fn):
    torch.cuda.synchronize()
    t = DeviceTimer()
    with t:
        fn()
    return t.get() * 1e3


def count_launches(fn):
    try:
        from torch.profiler import ProfilerActivity, profile

        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        kernels = memops = 0
        for ev in prof.events():
            if str(ev.device_type).endswith("CUDA"):
                if ev.name.lower().startswith(("memcpy", "memset")):
                    memops += 1
                else:
                    kernels += 1
        return {"kernels": kernels, "memcpy_memset": memops}
    except Exception as e:  # profiler unavailable: say so, do not guess
        return {"kernels": None, "error": repr(e)}


def summary(ts):
    return {
        "median_ms": round(statistics.median(ts), 3),
        "min_ms": round(min(ts), 3),
        "max_ms": round(max(ts), 3),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="all", choices=list(SHAPES) + ["all"])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=["per_metric", "fused"])
    args = ap.parse_args()
    assert torch.cuda.is_available(), "perf_coverage_suite needs a GPU"
    dev = torch.device("cuda:0")

    for shape in (list(SHAPES) if args.shape == "all" else [args.shape]):
        cfg = SHAPES[shape]
        metrics = canon_metrics(cfg["widths"], dev)
        layers = taps(cfg["n"], cfg["widths"], 2, dev)
        paths = {}
        if args.only != "fused":
            paths["per_metric"] = lambda: {m: f(layers) for m, f in metrics.items()}
        if args.only != "per_metric":
            suite = nc.CoverageSuite(metrics)
            paths["fused"] = lambda: suite(layers)
        row = {"shape": shape, "n": cfg["n"], "neurons": sum(cfg["widths"]),
               "iters": args.iters, "warmup": args.warmup}
        if len(paths) == 2:
            a, b = paths["per_metric"](), paths["fused"]()
            row["identical"] = all(
                torch.equal(a[m][0], b[m][0])
                and torch.equal(a[m][1].words, b[m][1].words)
                and a[m][1].nbits == b[m][1].nbits
                for m in metrics
            )
            del a, b
        for fn in paths.values():
            for _ in range(args.warmup):
                fn()
        times = {p: [] for p in paths}
        for _ in range(args.iters):  # alternate the paths
            for p, fn in paths.items():
                times[p].append(timed(fn))
        for p, fn in paths.items():
            row[p] = summary(times[p])
            row[p]["launches"] = count_launches(fn)
        if len(paths) == 2:
            row["speedup_median"] = round(
                row["per_metric"]["median_ms"] / row["fused"]["median_ms"], 2
            )
            row["slowest_fused_beats_fastest_per_metric"] = (
                row["fused"]["max_ms"] < row["per_metric"]["min_ms"]
            )
        print(json.dumps(row), flush=True)
        del layers, metrics, paths
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
