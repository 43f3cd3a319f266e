"""Cost of the CAM orders of one dataset: the loop of P ``ops.cam_order``
calls (what ``CoverageWorker`` and ``SurpriseHandler`` do by default) against
one ``ops.cam_order_many`` call (``cam_mode="batched"``).

Shapes:

  nc10000  the 12 neuron-coverage profiles of the MNIST-CNN tap widths at
           N = 10000, taps and tables made as scripts/perf_coverage_suite.py
           makes them, so the densities are the engine's
  nc512    the same at N = 512
  sc20000  ten 20000-row surprise-coverage profiles (1000 buckets, one bit
           per row; profiles/r02_cam_ladder.md), values from ten seeds
           through SurpriseCoverageMapper

Whole calls are timed with ``DeviceTimer`` (device drained before and after
each call). Before timing, the orders of the two paths are compared for
equality. After ``--warmup`` calls of each path the two alternate for
``--iters`` rounds, so both see the same machine; median, min and max are
reported per path, with the pick count (and how many of the picks were
followed by an incremental update) and the team size of every problem,
and whether the slowest batched call beat the fastest looped call.

``--only looped`` times that path alone and needs nothing of the batched op,
so the same script runs on a build that predates it. ``--no-incremental``
makes the batched kernel recount every row after every pick (the form the
incremental gain update is measured against).

Usage: python scripts/perf_cam_many.py [--shape NAME|all] [--iters K]
           [--warmup W] [--only looped|batched] [--no-incremental]
Prints one JSON line per shape. Needs a GPU.
"""

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from perf_coverage_suite import MNIST, canon_metrics, taps  # noqa: E402

from simple_tip_amd import ops  # noqa: E402
from simple_tip_amd.config import NUM_SC_BUCKETS  # noqa: E402
from simple_tip_amd.core.surprise import SurpriseCoverageMapper  # noqa: E402
from simple_tip_amd.core.timer import DeviceTimer  # noqa: E402

SHAPES = ("nc10000", "nc512", "sc20000")


def nc_problems(n, dev):
    """(names, scores, words, nbits) of the 12 configured metrics."""
    metrics = canon_metrics(MNIST, dev)
    layers = taps(n, MNIST, 2, dev)
    names, scores, words, nbits = [], [], [], []
    for name, metric in metrics.items():
        s, prof = metric(layers)
        names.append(name)
        scores.append(s.float())
        words.append(prof.words.contiguous())
        nbits.append(prof.nbits)
    del layers, metrics
    torch.cuda.empty_cache()
    return names, scores, words, nbits


def sc_problems(n, count, dev):
    names, scores, words, nbits = [], [], [], []
    for seed in range(count):
        g = torch.Generator(device=dev).manual_seed(100 + seed)
        # surprise values are positive with a long tail
        vals = -torch.log(torch.rand(n, generator=g, device=dev).clamp_min(1e-12))
        mapper = SurpriseCoverageMapper(NUM_SC_BUCKETS, float(vals.max()))
        prof = mapper.get_coverage_profile(vals)
        names.append(f"sc_{seed}")
        scores.append(vals.float())
        words.append(prof.words.contiguous())
        nbits.append(prof.nbits)
    return names, scores, words, nbits


def pick_forms(order, words, nbits):
    """[picks, picks updated incrementally]: the rows at the head of
    ``order`` that added coverage, and those among them whose ``newly`` mask
    was short enough for the batched kernel's incremental update (the sweep
    that follows such a pick touches only the listed words)."""
    import numpy as np

    from simple_tip_amd.ops import hip_ops

    w = words[order].cpu().numpy().view(np.uint64)
    width = w.shape[1]
    if hasattr(hip_ops, "CAM_MANY_INCR_DIV"):
        cap = min(width // hip_ops.CAM_MANY_INCR_DIV, hip_ops.CAM_MANY_LIST_CAP)
    else:  # a build without the batched kernel: nothing is incremental
        cap = 0
    unc = np.full(width, ~np.uint64(0), dtype=np.uint64)
    if nbits % 64:
        unc[-1] = np.uint64((1 << (nbits % 64)) - 1)
    picks = incremental = 0
    for row in w:
        newly = row & unc
        length = int(np.count_nonzero(newly))
        if length == 0:
            break
        unc &= ~newly
        picks += 1
        incremental += length <= cap
    return [picks, int(incremental)]


def log(msg):
    print(f"[perf_cam_many] {msg}", file=sys.stderr, flush=True)


def timed(fn):
    torch.cuda.synchronize()
    t = DeviceTimer()
    with t:
        fn()
    return t.get() * 1e3


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
    ap.add_argument("--only", choices=["looped", "batched"])
    ap.add_argument(
        "--no-incremental", action="store_true",
        help="batched path with a full re-sweep after every pick",
    )
    args = ap.parse_args()
    assert torch.cuda.is_available(), "perf_cam_many needs a GPU"
    dev = torch.device("cuda:0")
    if args.no_incremental:
        from simple_tip_amd.ops import hip_ops

        hip_ops.cam_many_force_full(True)

    for shape in (SHAPES if args.shape == "all" else [args.shape]):
        if shape == "sc20000":
            names, scores, words, nbits = sc_problems(20000, 10, dev)
        else:
            names, scores, words, nbits = nc_problems(int(shape[2:]), dev)
        paths = {}
        if args.only != "batched":
            paths["looped"] = lambda: [
                ops.cam_order(s, w, b) for s, w, b in zip(scores, words, nbits)
            ]
        if args.only != "looped":
            paths["batched"] = lambda: ops.cam_order_many(scores, words, nbits)
        row = {
            "shape": shape, "problems": len(names),
            "rows": words[0].shape[0], "iters": args.iters, "warmup": args.warmup,
            "incremental": not args.no_incremental,
            "words_per_row": {n: w.shape[1] for n, w in zip(names, words)},
        }
        log(f"{shape}: {len(names)} problems built")
        first = next(iter(paths.values()))()
        row["picks_and_incremental"] = {
            n: pick_forms(o, w, b) for n, o, w, b in zip(names, first, words, nbits)
        }
        if len(paths) == 2:
            a, b = paths["looped"](), paths["batched"]()
            row["identical"] = all(torch.equal(x, y) for x, y in zip(a, b))
            del a, b
        if "batched" in paths:
            from simple_tip_amd.ops import hip_ops

            cus = torch.cuda.get_device_properties(dev).multi_processor_count
            row["teams"] = dict(zip(names, hip_ops.cam_many_plan(
                [w.shape[0] for w in words], [w.shape[1] for w in words],
                min(256, cus),
            )))
        del first
        log(f"{shape}: picks {row['picks_and_incremental']}")
        for p, fn in paths.items():
            for _ in range(args.warmup):
                log(f"{shape}: warm-up {p} {timed(fn):.1f} ms")
        times = {p: [] for p in paths}
        for _ in range(args.iters):  # alternate the paths
            for p, fn in paths.items():
                times[p].append(timed(fn))
        for p in paths:
            row[p] = summary(times[p])
        if len(paths) == 2:
            row["speedup_median"] = round(
                row["looped"]["median_ms"] / row["batched"]["median_ms"], 2
            )
            row["slowest_batched_beats_fastest_looped"] = (
                row["batched"]["max_ms"] < row["looped"]["min_ms"]
            )
        print(json.dumps(row), flush=True)
        del scores, words, paths
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
