"""GPU: bench.py --dump-outputs writes what the timed path computed in its last step, and --steps sets the timed steps.

Two runs with the same arguments must see the same inputs (the synthetic envs' observations, rewards and terminals
depend only on the seed, the env index and the env's step count) and compute the same bits from them: three
iterations, so the rollouts that follow an optimiser step are covered."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["--gpus", "1", "--n-steps", "8", "--steps", "2", "--warmup", "1", "--no-cpu-baseline", "--no-scan",
        "--no-kernel-table", "--no-opt-in"]


def _bench(*argv):
    e = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT"):
        e.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *argv], env=e, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


@pytest.mark.gpu
def test_bench_dump_outputs_same_every_run(tmp_path):
    runs = []
    for i in range(2):
        d = tmp_path / f"run{i}"
        line = _bench(*ARGS, "--dump-outputs", str(d))
        assert line["steps"] == 2 and line["ms_per_step"] > 0
        assert line["dumped_outputs"]["dir"] == str(d)
        sampled = line["dumped_outputs"]["sampled"]
        files = sorted(os.listdir(d))
        assert len(files) == line["dumped_outputs"]["arrays"]
        arrays = {f[:-4]: np.load(d / f) for f in files}
        assert all(f.endswith(".npy") for f in files)
        assert all(v.dtype in (np.float32, np.float64) for v in arrays.values())
        assert sum(v.nbytes for v in arrays.values()) <= 64 << 20
        runs.append(arrays)
    a, b = runs
    assert a.keys() == b.keys()
    for k in ("observations", "rewards", "terminals", "policy_params", "advantage", "returns", "policy_stat_rows"):
        assert k in a, k
    # 9 x 256 x 4 x 84 x 84 uint8 observations: written as the fixed sample; everything else whole
    assert a["observations"].shape == (bench.DUMP_MAX_ELEMS,)
    assert sampled == ["observations"]
    assert a["rewards"].shape == (8, 256) and a["terminals"].shape == (8, 256)
    for k, v in a.items():
        assert v.shape == b[k].shape and np.isfinite(v).all(), k
        assert np.array_equal(v, b[k]), k
