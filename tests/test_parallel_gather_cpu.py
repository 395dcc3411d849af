"""CPU: `parallel.gather_columns` under a 2-process gloo group, and the guard that the intrinsic-return filter is a
function of the GLOBAL [N, world * A] array.

The gather writes a rank's [N, A] shard into its column block of a zeroed [N, world * A] buffer and sums the buffers
over ranks: x + 0 = x for every finite float and every integer, so the result must carry the shards' bits - checked here
for float32 (denormals, the largest finite value, negative values), int32 (non-negative hashes and negative values) and
bool.  With one rank the input object itself comes back and nothing is issued.

The filter (`rollout.intrinsic_return_scale`) feeds a running variance with the filter's output over ALL envs at every
step, so the scale of the whole array is not what either half gives on its own: a data-parallel run that filtered each
rank's columns separately would hold a different normaliser on every rank, and none of them the one-rank run's."""
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from ppo_amd import parallel  # noqa: E402
from ppo_amd.rollout import intrinsic_return_scale  # noqa: E402
from ppo_amd.running_stats import RunningMeanStd  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, A, GAMMA_INT = 5, 3, 0.99


def global_rewards():
    """A fixed [N, 2A] float32 array, clipped as generate_rollout clips; the halves differ in size and sign."""
    k = np.arange(N * 2 * A, dtype=np.float64).reshape(N, 2 * A)
    r = np.sin(0.7 * k) * (1.0 + (k % (2 * A) >= A) * 6.0) + 0.25 * (k % 4)
    return np.clip(r.astype(np.float32), -5, 5)


def expected_scale(rewards):
    """The filter and Chan's merge written out in the test, float64 throughout, --ir_propagation=True."""
    ems, mean, var, count = np.zeros(rewards.shape[1], np.float64), np.float64(0.0), np.float64(1.0), 1e-4
    for t in range(rewards.shape[0]):
        ems = GAMMA_INT * ems + rewards[t].astype(np.float64)
        b_mean, b_var, b_count = np.mean(ems), np.var(ems), ems.shape[0]
        total = count + b_count
        delta = b_mean - mean
        m2 = var * count + b_var * b_count + np.square(delta) * count * b_count / total
        mean, var, count = mean + delta * b_count / total, m2 / total, total
    return ems, np.float64(1e-5 + var ** 0.5)


def scale_of(rewards):
    ems, scale = intrinsic_return_scale(np.zeros([rewards.shape[1]]), RunningMeanStd(shape=()), rewards,
                                        np.zeros(rewards.shape, bool), GAMMA_INT, True)
    return ems, np.float64(scale)


def test_filter_over_the_global_array_is_not_what_its_halves_give():
    r = global_rewards()
    assert r.shape == (N, 2 * A) and r.dtype == np.float32
    want_ems, want = expected_scale(r)
    ems, got = scale_of(r)
    assert got.tobytes() == want.tobytes(), (got, want)
    assert ems.dtype == np.float64 and ems.tobytes() == want_ems.tobytes()
    halves = [scale_of(np.ascontiguousarray(r[:, lo:lo + A]))[1] for lo in (0, A)]
    assert halves[0] != want and halves[1] != want and halves[0] != halves[1], (halves, want)


def test_one_rank_returns_its_input():
    assert parallel.world_size() == 1
    for t in (torch.arange(6, dtype=torch.float32).view(2, 3), torch.ones((2, 3), dtype=torch.bool)):
        assert parallel.gather_columns(t) is t


GATHER_WORKER = r'''
import os, sys
sys.path.insert(0, sys.argv[1])
import numpy as np, torch, torch.distributed as dist
from ppo_amd import parallel
from ppo_amd.rollout import intrinsic_return_scale
from ppo_amd.running_stats import RunningMeanStd
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo", rank=rank, world_size=world)
assert parallel.world_size() == 2
N, A = 5, 3
tiny, big = float(np.float32(1e-45)), float(np.finfo(np.float32).max)


def shard(dtype, r):
    g = torch.Generator().manual_seed(40 + r)
    if dtype == torch.float32:
        t = torch.randn((N, A), generator=g) * 3.0
        t[0, 0], t[1, 1], t[2, 2], t[3, 0] = tiny, -big, 0.0, big
        return t
    if dtype == torch.int32:
        t = torch.randint(0, 2 ** 24, (N, A), generator=g, dtype=torch.int32)
        t[0, 0], t[1, 1], t[2, 2] = 2 ** 31 - 1, -7, 0
        return t
    if dtype == torch.uint8:
        return torch.randint(0, 256, (N, A), generator=g, dtype=torch.uint8)
    return torch.rand((N, A), generator=g) < 0.5


for dtype in (torch.float32, torch.int32, torch.uint8, torch.bool):
    mine = shard(dtype, rank)
    kept = mine.clone()
    got = parallel.gather_columns(mine)
    want = torch.cat([shard(dtype, r) for r in range(world)], dim=1)
    assert got.dtype == dtype and tuple(got.shape) == (N, world * A), (got.dtype, got.shape)
    assert got.numpy().tobytes() == want.numpy().tobytes(), f"{dtype}: gathered bits differ from the concatenation"
    assert mine.numpy().tobytes() == kept.numpy().tobytes(), "the gather changed its input"
    # a column slice of a wider buffer (what a rank holds of a strided array) gathers alike
    wide = torch.cat([mine, mine], dim=1)
    assert parallel.gather_columns(wide[:, A:]).numpy().tobytes() == want.numpy().tobytes()
try:
    parallel.gather_columns(torch.zeros((N, A), dtype=torch.float64))
except ValueError:
    pass
else:
    raise AssertionError("a float64 shard was accepted")

# the intrinsic-return filter over the gathered rewards: every rank gets the scale of the global array
rewards = torch.from_numpy(np.load(sys.argv[2]))
full = parallel.gather_columns(rewards[:, rank * A:(rank + 1) * A].contiguous()).numpy()
ems, scale = intrinsic_return_scale(np.zeros([world * A]), RunningMeanStd(shape=()), full, np.zeros(full.shape, bool),
                                    0.99, True)
dist.barrier(); dist.destroy_process_group()
print("rank", rank, "ok scale", np.float64(scale).tobytes().hex())
'''


def test_gather_is_the_concatenation_in_rank_order_two_ranks_gloo(tmp_path):
    script = tmp_path / "gather_worker.py"
    script.write_text(GATHER_WORKER)
    rewards = global_rewards()
    np.save(tmp_path / "rewards.npy", rewards)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29561", WORLD_SIZE="2")
    procs = [subprocess.Popen([sys.executable, str(script), ROOT, str(tmp_path / "rewards.npy")], env=dict(env, RANK=str(r)),
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(2)]
    try:
        outs = [p.communicate(timeout=180)[0] for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    want = expected_scale(rewards)[1].tobytes().hex()
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o[-3000:]
        assert "ok scale " + want in o, (o[-500:], want)
