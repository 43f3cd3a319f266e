"""Cost of pc-MMDSA's k-means discovery: the ``_KmeansDiscriminator``
constructor with ``kmeans_mode="looped"`` (one ``kmeans_fit`` and one
``silhouette_score`` per k, the default) against ``"batched"`` (every restart
of every k in lockstep through ``kmeans_fit_many``, all silhouettes from one
``silhouette_scores_many`` call).

Shapes (k = 2..5, ``n_init = 10``, ``max_iter = 300``):

  mnist    N = 18000, D = 1600: 30 % of the MNIST training ATs
  serving  N = 18000, D = 64

Rows are synthetic and class-structured (ten classes, relu(mean + noise), as
scripts/perf_gaussian_sa.py makes them). Whole constructor calls are timed
with ``DeviceTimer`` (device drained before and after). After ``--warmup``
calls of each mode the two alternate for ``--iters`` rounds, so both see the
same machine; median, min and max are reported per mode, with the chosen k
and best silhouette of both, the Lloyd iterations run (batched: lockstep
iterations of all problems; looped: the sum over the 40 problems) and
whether the slowest batched call beat the fastest looped call. The batched
time is split into k-means++ init, Lloyd and silhouette by timing the three
pieces on their own.

Usage: python scripts/perf_kmeans_many.py [--shape NAME|all] [--iters K]
           [--warmup W]
Prints one JSON line per shape. Needs a GPU.
"""

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from simple_tip_amd import ops  # noqa: E402
from simple_tip_amd.core import kmeans  # noqa: E402
from simple_tip_amd.core.surprise import _KmeansDiscriminator  # noqa: E402
from simple_tip_amd.core.timer import DeviceTimer  # noqa: E402

SHAPES = {"mnist": (18000, 1600), "serving": (18000, 64)}
KS = (2, 3, 4, 5)
N_INIT = 10


def synthetic(n, width, classes, seed, dev):
    g = torch.Generator(device="cpu").manual_seed(seed)
    means = torch.randn(classes, width, generator=torch.Generator().manual_seed(7)) * 0.5
    pred = torch.randint(0, classes, (n,), generator=g)
    parts = []
    for s in range(0, n, 4096):
        p = pred[s : s + 4096]
        x = means[p] + torch.randn(p.shape[0], width, generator=g)
        parts.append(torch.relu(x).to(dev))
    return torch.cat(parts)


def log(msg):
    print(f"[perf_kmeans_many] {msg}", file=sys.stderr, flush=True)


def timed(fn):
    torch.cuda.synchronize()
    t = DeviceTimer()
    with t:
        out = fn()
    return t.get() * 1e3, out


def summary(ts):
    return {
        "median_ms": round(statistics.median(ts), 3),
        "min_ms": round(min(ts), 3),
        "max_ms": round(max(ts), 3),
    }


def looped_iterations(x):
    """Lloyd updates the looped path runs, summed over all restarts of all k:
    its rowmin_l2 calls minus the final assign of every restart."""
    calls = [0]
    real = ops.rowmin_l2

    def counting(*a, **kw):
        calls[0] += 1
        return real(*a, **kw)

    ops.rowmin_l2 = counting
    try:
        for k in KS:
            kmeans.kmeans_fit(x, k, n_init=N_INIT)
    finally:
        ops.rowmin_l2 = real
    return calls[0] - len(KS) * N_INIT


def draw_inits(x):
    for k in KS:
        gen = torch.Generator().manual_seed(0)
        for _ in range(N_INIT):
            kmeans._kmeanspp_init(x, k, gen)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="all", choices=list(SHAPES) + ["all"])
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "perf_kmeans_many needs a GPU"
    dev = torch.device("cuda:0")

    for shape in (SHAPES if args.shape == "all" else [args.shape]):
        n, d = SHAPES[shape]
        x = synthetic(n, d, 10, 0, dev)
        modes = {
            m: (lambda m=m: _KmeansDiscriminator(
                x, potential_k=KS, n_init=N_INIT, kmeans_mode=m))
            for m in ("looped", "batched")
        }
        row = {"shape": shape, "N": n, "D": d, "ks": list(KS), "n_init": N_INIT,
               "iters": args.iters, "warmup": args.warmup}
        for m, fn in modes.items():
            for _ in range(args.warmup):
                ms, disc = timed(fn)
                log(f"{shape}: warm-up {m} {ms:.1f} ms")
            row[f"{m}_best_k"] = disc.best_k
            row[f"{m}_best_silhouette"] = round(disc.best_score, 6)
        times = {m: [] for m in modes}
        for _ in range(args.iters):  # alternate the modes
            for m, fn in modes.items():
                times[m].append(timed(fn)[0])
        for m in modes:
            row[m] = summary(times[m])
        row["speedup_median"] = round(
            row["looped"]["median_ms"] / row["batched"]["median_ms"], 2
        )
        row["slowest_batched_beats_fastest_looped"] = (
            row["batched"]["max_ms"] < row["looped"]["min_ms"]
        )
        # the pieces of the batched path, each timed on its own
        stats = {}
        init_ms, _ = timed(lambda: draw_inits(x))
        fit_ms, fits = timed(lambda: kmeans.kmeans_fit_many(
            x, KS, n_init=N_INIT, stats=stats))
        sil_ms, _ = timed(lambda: kmeans.silhouette_scores_many(
            x, [fits[k][1] for k in KS]))
        row["batched_split_ms"] = {
            "kmeanspp_init": round(init_ms, 3),
            "lloyd": round(fit_ms - init_ms, 3),
            "silhouette": round(sil_ms, 3),
        }
        row["batched_lockstep_iterations"] = stats["lloyd_iterations"]
        row["looped_iterations_all_problems"] = looped_iterations(x)
        print(json.dumps(row), flush=True)
        del x, modes, fits
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
