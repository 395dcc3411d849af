"""GPU: --policy_opt_optimizer=sgd under data parallelism - two ranks sharing the one GPU (gloo carrying the device tensors,
as in tests/test_dp_rnd_gpu.py), started from different torch seeds.

One policy minibatch step (8 agents x 4 steps per rank, a global minibatch of 64: one step per phase).  What must hold:
  (a) the gradient is summed over the ranks before the step - one float32 addition of two buffers, one rounding,
      commutative, so the reduced buffer is g0 + g1 bit for bit on both ranks;
  (b) the step is the SGD step on that sum with grad_div = 2: flat and the norm within the bars of
      tests/test_sgd_float64_gpu.py (4 x plain float32 torch against float64, never below 2^-23 of the local scale) of
      tests/sgd_float64.py's sgd_ref, so the logged norm is |g0 + g1| / 2;
  (c) both ranks' parameters are bit-identical afterwards, and no rank has moments or a step count.
The early-bucket hook is parked for the step so that each rank's own gradient can be read whole before the reduction
(GradReducer.finish then reduces the whole buffer in one collective)."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import policy_optim_float64 as R  # noqa: E402
import sgd_float64 as S  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORLD, LR = 2, 0.01

WORKER = r'''
import os, sys
sys.path.insert(0, sys.argv[1])
import numpy as np, torch, torch.distributed as dist
from ppo_amd import envs, logger, models, parallel, rollout
from ppo_amd.config import args
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
torch.cuda.set_device(0)
dist.init_process_group("gloo", rank=rank, world_size=world)
args.setup(["--agents=8", "--n_steps=4", "--model_architecture=single", "--model_encoder=nature", "--env_type=synthetic",
            "--env_embed_time=False", "--seed=3", "--device=cuda", "--policy_opt_mini_batch_size=64", "--policy_opt_epochs=1",
            "--policy_opt_optimizer=sgd", "--policy_opt_lr=0.01", "--disable_logging=True"])
torch.manual_seed(1000 + rank)   # DIFFERENT initial weights per rank
np.random.seed(100 + rank)
shape, nA = envs.get_env_spec()
model = models.TVFModel("nature", input_dims=shape, actions=nA, device="cuda", architecture="single", hidden_units=256,
                        head_scale=0.1, head_bias=True)
r = rollout.Runner(model, logger.Logger(quiet=True))
assert r.world == 2 and r.rank == rank and r.policy_optimizer.kind == "sgd"
r.vec_env = envs.create_envs_classic(rank=rank, world=world)
r.reset()
net = r.policy_net
r.generate_rollout()
r.calculate_returns()
out = {"w0": net.flat.cpu().numpy()}
net.grad_ready_hook = None
red, seen = r._reducers[id(net)], []
finish = red.finish


def observed_finish(*a, **kw):
    torch.cuda.synchronize()
    own = net.grad.clone()
    finish(*a, **kw)
    seen.append((own, net.grad.clone()))


red.finish = observed_finish
r.train_policy()
red.finish = finish
torch.cuda.synchronize()
assert len(seen) == 1
out["grad"], out["reduced"] = seen[0][0].cpu().numpy(), seen[0][1].cpu().numpy()
out["w1"] = net.flat.cpu().numpy()
norms = r._phase_stats["policy"][1]
assert norms.numel() == 1
out["norm"] = np.float64(norms[0].item())
out["max_grad_norm"] = np.float32(args.max_grad_norm if args.grad_clip_mode == "global_norm" else 0.0)
out["no_state"] = np.array(net.exp_avg is None and net.exp_avg_sq is None and net._adam_step == 0)
parallel.assert_identical_across_ranks([net.flat], "replicas after one SGD step")
dist.barrier(); dist.destroy_process_group()
np.savez(os.path.join(sys.argv[2], f"r{rank}.npz"), **out)
print("rank", rank, "ok")
'''


@pytest.fixture(scope="module")
def ranks(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("dp_sgd")
    script = tmp / "dp_sgd_worker.py"
    script.write_text(WORKER)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29583", WORLD_SIZE="2")
    procs = [subprocess.Popen([sys.executable, str(script), ROOT, str(tmp)], env=dict(env, RANK=str(r)),
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(2)]
    try:
        outs = [p.communicate(timeout=180)[0] for p in procs]  # one rollout of 4 steps and one minibatch step
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o[-3000:]
        assert "ok" in o
    return [dict(np.load(tmp / f"r{r}.npz")) for r in range(2)]


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_gradient_is_summed_over_ranks_before_the_sgd_step(ranks):
    r0, r1 = ranks
    g0, g1 = r0["grad"], r1["grad"]
    assert g0.dtype == np.float32 and np.abs(g0).max() > 0 and not same(g0, g1), "the ranks trained on the same rows"
    want = g0 + g1  # float32, one rounding per element
    assert same(r0["reduced"], want) and same(r1["reduced"], want)


def test_the_step_is_sgd_on_the_summed_gradient_with_grad_div_2(ranks):
    r0, r1 = ranks
    assert same(r0["w0"], r1["w0"]), "Runner.__init__ did not broadcast rank 0's parameters"
    g, w0, mn = r0["grad"] + r1["grad"], r0["w0"], r0["max_grad_norm"]
    ref = S.sgd_ref(w0, [g], mn, float(WORLD), lr=LR)
    e32 = S.sgd_errs(S.sgd_f32(w0, [g], mn, float(WORLD), lr=LR), ref)
    for r in ranks:
        e = S.sgd_errs([{"w": r["w1"], "norm": float(r["norm"])}], ref)
        for k in ("w", "norm"):
            bar = R.report(f"sgd dp {k}", e[k], e32[k])
            assert e[k] <= bar, f"{k} {e[k]:.3e} over the bar {bar:.3e}"
    # the logged norm is that of the mean gradient
    norm = float(np.sqrt(np.sum(np.square(g.astype(np.float64))))) / WORLD
    assert norm > 0 and abs(ref[0]["norm"] - norm) <= 1e-12 * norm and float(r0["norm"]) == float(r1["norm"])
    assert not same(r0["w1"], w0)


def test_replicas_are_bit_identical_and_stateless_after_the_step(ranks):
    r0, r1 = ranks
    assert same(r0["w1"], r1["w1"])
    assert bool(r0["no_state"]) and bool(r1["no_state"])
