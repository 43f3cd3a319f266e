"""The driver depends on bench.py's CLI + JSON contract; pin it.

Runs the real script (tiny sizes, CPU) in a subprocess and validates the
single JSON line the driver parses.
"""

import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


TINY = [
    "--steps", "2", "--warmup", "1", "--batch", "128",
    "--train-n", "512", "--setup-epochs", "1",
]
DUMP_NAMES = ("deep_gini", "dsa", "pc_lsa", "pred")
QUALITY_KEYS = (
    "apfd_gini_lastbatch", "apfd_gini_nominal_lastbatch",
    "apfd_dsa_lastbatch", "apfd_pclsa_lastbatch",
)


def _run_bench(*extra):
    return subprocess.run(
        [sys.executable, os.path.join(REPO, "bench.py"), *TINY, *extra],
        capture_output=True, text=True, timeout=540, cwd=REPO,
    )


@pytest.fixture(scope="module")
def plain_run(tmp_path_factory):
    """One plain (no --full) tiny run that also dumps its outputs."""
    dump = tmp_path_factory.mktemp("bench_plain") / "dump"
    return _run_bench("--dump-outputs", str(dump)), dump


@pytest.mark.timeout(600)
def test_bench_json_contract(plain_run):
    out, _ = plain_run
    assert out.returncode == 0, out.stderr[-2000:]
    line = out.stdout.strip().splitlines()[-1]
    d = json.loads(line)

    assert d["metric"] == "inputs_per_sec_prioritized"
    assert d["unit"] == "inputs/s"
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1
    assert d["value"] > 0 and d["ms_per_step"] > 0
    # value is the WHOLE-JOB aggregate: inputs/s * step time = global batch
    assert d["value"] * d["ms_per_step"] / 1000 == pytest.approx(
        d["config"]["global_batch"], rel=1e-6
    )
    assert d["higher_is_better"] is True
    assert d["scaling"] == "weak"
    assert d["dtype"] == "bf16" and d["data"] == "synthetic"
    assert d["config"]["model"] == "cifar10_resnet20"
    assert d["config"]["parallelism"] == "dp1"
    assert "vs_baseline" in d  # null (no published number), but present
    # a plain run skips the auxiliary quality signals: present, but null
    assert all(d["config"][k] is None for k in QUALITY_KEYS)


def _load_dump(dump):
    import numpy as np

    arrays = {n: np.load(dump / f"{n}.npy") for n in DUMP_NAMES}
    for a in arrays.values():
        assert a.dtype == np.float32 and a.shape == (128,)
    return arrays


def test_bench_dump_outputs(plain_run):
    """--dump-outputs writes what the last timed step returned: one float32
    score (or predicted class) per input of that step's batch."""
    import numpy as np

    out, dump = plain_run
    assert out.returncode == 0, out.stderr[-2000:]
    assert sorted(p.name for p in dump.iterdir()) == sorted(
        f"{n}.npy" for n in DUMP_NAMES
    )
    a = _load_dump(dump)
    assert np.isfinite(a["deep_gini"]).all() and np.isfinite(a["dsa"]).all()
    assert (a["deep_gini"] >= 0).all() and (a["deep_gini"] <= 1).all()
    assert (a["dsa"] >= 0).all()
    assert np.isin(a["pred"], np.arange(10)).all()


@pytest.mark.timeout(600)
def test_bench_full_adds_quality_and_repeats_outputs(plain_run, tmp_path):
    """--full reports the APFD quality signals, and a second run with the
    same sizes sees identical inputs, so its dumped outputs agree with the
    plain run's up to the summation order inside a kernel: the 4096-wide
    fp32 accumulations leave a relative 1e-5 at most, and deep-gini's
    1 - sum(p^2) an absolute few 1e-7; 1e-4 and 1e-6 are asserted."""
    import numpy as np

    out = _run_bench("--full", "--dump-outputs", str(tmp_path / "dump"))
    assert out.returncode == 0, out.stderr[-2000:]
    d = json.loads(out.stdout.strip().splitlines()[-1])
    vals = [d["config"][k] for k in QUALITY_KEYS]
    assert any(v is not None for v in vals)
    assert all(v is None or 0.0 <= v <= 1.0 for v in vals)

    a, b = _load_dump(plain_run[1]), _load_dump(tmp_path / "dump")
    assert np.array_equal(a["pred"], b["pred"])
    for n in ("deep_gini", "dsa", "pc_lsa"):
        np.testing.assert_allclose(a[n], b[n], rtol=1e-4, atol=1e-6, err_msg=n)


def test_bench_gpus_flag_validated():
    out = subprocess.run(
        [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "8",
         "--steps", "1", "--warmup", "0"],
        capture_output=True, text=True, timeout=120, cwd=REPO,
    )
    assert out.returncode != 0
    assert "WORLD_SIZE" in (out.stderr + out.stdout)


@pytest.mark.timeout(900)
def test_bench_shard_train_world2_contract():
    """The strong-scaling mode end-to-end (gloo world 2): sharded forward +
    train-AT-sharded scoring must produce the contract JSON with
    scaling=strong and the whole-job (not per-rank) aggregate.

    The backend is pinned to gloo so the two ranks also run on a machine
    with a single GPU, where they share the device (RCCL refuses duplicate
    devices); without a GPU gloo is the default anyway."""
    import numpy as np

    port = int(np.random.RandomState(os.getpid()).randint(20000, 40000))
    env = dict(os.environ, TIP_DIST_BACKEND="gloo")
    out = subprocess.run(
        [
            sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
            "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
            "--master-port", str(port),
            os.path.join(REPO, "bench.py"), "--gpus", "2",
            "--steps", "2", "--warmup", "1", "--batch", "128",
            "--train-n", "512", "--setup-epochs", "1", "--shard-train",
        ],
        capture_output=True, text=True, timeout=840, cwd=REPO, env=env,
    )
    assert out.returncode == 0, out.stderr[-2000:]
    line = [l for l in out.stdout.strip().splitlines() if l.startswith("{")][-1]
    d = json.loads(line)
    assert d["scaling"] == "strong"
    assert d["n_gpus"] == 2
    assert d["config"]["parallelism"] == "train-shard2"
    assert d["config"]["global_batch"] == 128  # total work fixed, not x2
