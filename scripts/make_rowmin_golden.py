"""Record the bf16 grouped row-min of one seeded case as a golden file.

Run once on the build whose results are to be pinned (the commit before the
pipelined kernel): writes tests/golden/rowmin_bf16_parent.npz with `dist`,
`idx` and `dsa` of the gathered entry point, per source row.
tests/test_gpu_pairwise_bf16_pipeline.py regenerates the inputs from the
seed through golden_inputs() below and expects every build, on either
kernel, to reproduce the file bit for bit.

Usage: python scripts/make_rowmin_golden.py [out.npz]
"""

import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "rowmin_bf16_parent.npz")

SEED = 20
K = 3 * 64
TEST_ROWS = [200, 129, 1, 270]    # 600 rows, shuffled
TRAIN_ROWS = [257, 130, 513, 64]


def golden_inputs():
    """CPU tensors of the golden case: bf16 source rows, their predicted
    class (shuffled), bf16 class-sorted train rows, train offsets, b-table."""
    rng = np.random.RandomState(SEED)
    b, n = sum(TEST_ROWS), sum(TRAIN_ROWS)
    pred = rng.permutation(np.repeat(np.arange(len(TEST_ROWS)), TEST_ROWS))
    src = (rng.randn(b, K) * 0.3).astype(np.float32)
    train = (rng.randn(n, K) * 0.3).astype(np.float32)
    btable = rng.rand(n).astype(np.float32) + 0.5
    return dict(
        pred=torch.from_numpy(pred).long(),
        src=torch.from_numpy(src).to(torch.bfloat16),
        train=torch.from_numpy(train).to(torch.bfloat16),
        nseg=torch.tensor(np.concatenate([[0], np.cumsum(TRAIN_ROWS)]),
                          dtype=torch.int32),
        btable=torch.from_numpy(btable),
        jb_max=(max(TRAIN_ROWS) + 127) // 128,
    )


def run_plan(ext, case):
    """The gathered row-min of `case` on the GPU: (dist, idx, dsa) per source
    row, workspaces and outputs pre-filled with NaN / -7."""
    dev = torch.device("cuda")
    src, train, pred = case["src"].to(dev), case["train"].to(dev), case["pred"].to(dev)
    c = case["nseg"].numel() - 1
    b = src.shape[0]
    tseg, rowmap, _ = ext.segment_plan(pred, c)
    an = torch.empty(b, device=dev)
    ext.rownorm_bf16_out(src, an)
    bn = torch.empty(train.shape[0], device=dev)
    ext.rownorm_bf16_out(train, bn)
    bp = ext.segment_plan_rows(b, c)
    jb = case["jb_max"]
    pval = torch.full((jb, bp), float("nan"), device=dev)
    pidx = torch.full((jb, bp), -1, dtype=torch.int32, device=dev)
    dsa = torch.full((b,), float("nan"), device=dev)
    dist = torch.full((b,), float("nan"), device=dev)
    idx = torch.full((b,), -7, dtype=torch.int32, device=dev)
    ext.grouped_rowmin_plan(
        src, train, tseg, case["nseg"].to(dev), rowmap, an, bn,
        case["btable"].to(dev), jb, pval, pidx, dsa, dist, idx,
    )
    return dist.cpu().numpy(), idx.cpu().numpy(), dsa.cpu().numpy()


def main():
    sys.path.insert(0, REPO)
    from simple_tip_amd.ops import _load_compiled

    out = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    dist, idx, dsa = run_plan(_load_compiled(), golden_inputs())
    assert np.isfinite(dist).all() and (idx >= 0).all()
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    np.savez_compressed(out, dist=dist, idx=idx, dsa=dsa)
    print(f"wrote {out}: {dist.shape[0]} rows, K = {K}, "
          f"{os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
