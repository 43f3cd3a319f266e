"""MC-dropout sampling of the IMDB transformer: replay vs the fused tail.

Times, on one GPU and in one process:
  - ``BaseModel(vr_mode="replay")`` and ``vr_mode="fused"`` end to end
    (``_variation_ratio`` on N = 25000 token rows, the IMDB study's test-set
    size, ImdbTransformer, S = 200, the study's predict batch of 600), the two
    modes alternating over ``--reps`` repetitions after one warm-up each; and
    the same with the extras (``_mc_scores`` with PE, MI and MS);
  - the deterministic prefix (embedding + attention) alone;
  - the ``mc_transformer_votes`` and ``mc_transformer_stats`` kernels alone,
    one launch over all N rows of the model's own prefix output.

Every window ends in a device synchronise. Prints one JSON line.

  python scripts/perf_vr_transformer.py [--n 25000] [--reps 3] [--kernel-iters 10]
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
from simple_tip_amd.models import ImdbTransformer  # noqa: E402


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1000.0, out


def event_ms(call, iters):
    """Median / min / max device-event time of ``call``."""
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
    return {
        "median_ms": round(statistics.median(times), 3),
        "min_ms": round(min(times), 3),
        "max_ms": round(max(times), 3),
    }


def spread(xs):
    return {
        "median_ms": round(statistics.median(xs), 3),
        "min_ms": round(min(xs), 3),
        "max_ms": round(max(xs), 3),
        "all_ms": [round(x, 3) for x in xs],
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=25000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--kernel-iters", type=int, default=10)
    ap.add_argument("--predict-batch", type=int, default=600)
    args = ap.parse_args()

    assert torch.cuda.is_available(), "perf_vr_transformer.py needs a GPU"
    assert ops.hip_available(), "perf_vr_transformer.py requires _tip_hip"
    from simple_tip_amd.ops import hip_ops

    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = ImdbTransformer().to(dev)
    tokens = torch.randint(0, 2000, (args.n, 100))
    all_keys = ("VR", "PE", "MI", "MS")

    def handler(mode, keys=("VR",)):
        return BaseModel(model, None, device=dev, vr_mode=mode, vr_seed=0,
                         predict_batch=args.predict_batch, mc_quantifiers=keys)

    replay, fused = handler("replay"), handler("fused")
    replay_x, fused_x = handler("replay", all_keys), handler("fused", all_keys)

    # warm-up: code objects, library algorithm choice, allocator
    _, vr_r = wall_ms(lambda: replay._variation_ratio(tokens)[0])
    _, vr_f = wall_ms(lambda: fused._variation_ratio(tokens)[0])
    wall_ms(lambda: replay_x._mc_scores(tokens))
    wall_ms(lambda: fused_x._mc_scores(tokens))
    t = {"replay": [], "fused": [], "replay_extras": [], "fused_extras": []}
    for _ in range(args.reps):
        t["replay"].append(wall_ms(lambda: replay._variation_ratio(tokens))[0])
        t["fused"].append(wall_ms(lambda: fused._variation_ratio(tokens))[0])
        t["replay_extras"].append(wall_ms(lambda: replay_x._mc_scores(tokens))[0])
        t["fused_extras"].append(wall_ms(lambda: fused_x._mc_scores(tokens))[0])

    # the prefix and the kernels alone, on the model's own prefix output
    tail = model.dropout_tail()
    params = ops.McTransformerParams(*[
        v if isinstance(v, float) else v.detach().float().contiguous()
        for v in tail.params
    ])
    dev_tokens = tokens.to(dev)

    def prefix():
        xs, attns = [], []
        with torch.no_grad():
            for s0 in range(0, args.n, args.predict_batch):
                emb = tail.embed(dev_tokens[s0 : s0 + args.predict_batch])
                xs.append(emb)
                attns.append(tail.att(emb, emb, emb, need_weights=False)[0])
        return torch.cat(xs).contiguous(), torch.cat(attns).contiguous()

    x, attn = prefix()
    prefix_ms = event_ms(prefix, args.kernel_iters)
    call = lambda op: op(  # noqa: E731
        x, attn, params, tail.rates, DROPOUT_SAMPLE_SIZE, 0
    )
    votes_ms = event_ms(lambda: call(ops.mc_transformer_votes), args.kernel_iters)
    stats_ms = event_ms(lambda: call(ops.mc_transformer_stats), args.kernel_iters)
    t_e = x.shape[1] * x.shape[2]
    f, h, c = params.w1.shape[0], params.w3.shape[0], params.w4.shape[0]
    fma = args.n * DROPOUT_SAMPLE_SIZE * (
        x.shape[1] * 2 * f * x.shape[2] + h * x.shape[2] + c * h
    )

    med = {k: statistics.median(v) for k, v in t.items()}
    result = {
        "script": "perf_vr_transformer",
        "device": torch.cuda.get_device_name(0),
        "n": args.n,
        "tokens": x.shape[1],
        "samples": DROPOUT_SAMPLE_SIZE,
        "predict_batch": args.predict_batch,
        "reps": args.reps,
        "replay": spread(t["replay"]),
        "fused": spread(t["fused"]),
        "speedup": round(med["replay"] / med["fused"], 2),
        "replay_extras": spread(t["replay_extras"]),
        "fused_extras": spread(t["fused_extras"]),
        "speedup_extras": round(med["replay_extras"] / med["fused_extras"], 2),
        "prefix": prefix_ms,
        "kernel_votes": votes_ms,
        "kernel_stats": stats_ms,
        "kernel_votes_tflops": round(2 * fma / votes_ms["median_ms"] / 1e9, 2),
        "mask_elements_per_sample": 2 * t_e + x.shape[2] + h,
        "launch": hip_ops.mc_transformer_launch_config(x.shape[1], f, h),
        "mean_vr_replay": round(float(vr_r.mean()), 5),
        "mean_vr_fused": round(float(vr_f.mean()), 5),
    }
    print(json.dumps(result))


if __name__ == "__main__":
    main()
