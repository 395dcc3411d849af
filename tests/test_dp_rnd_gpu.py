"""GPU: Random Network Distillation under data parallelism - two ranks sharing the one GPU (gloo carrying the device
tensors, as in tests/test_dp_gpu.py), started from different torch seeds.

What must hold:
  (a) Runner.__init__ leaves rank 0's target and predictor on every rank (the target never trains: replicas that drew
      their own would disagree for good);
  (b) the predictor's gradient is summed over ranks before its Adam step - one float32 addition of two ranks' buffers,
      one rounding, commutative, so the reduced buffer is g0 + g1 bit for bit - and Adam divides by the world size
      (the norm it reports is |g0 + g1| / 2; the bar of 1e-3 is three orders above a float32 sum of squares' error and
      far below the factor 2 it has to tell apart);
  (c) over whole iterations the replicas and the intrinsic-return normaliser (`intrinsic_reward_norm_scale`, `ems_norm`
      with one entry per env of the whole run, the `intrinsic_returns_rms` moments) stay identical across ranks, and the
      normaliser is what `intrinsic_return_scale` gives on the clipped rewards of both ranks together;
  (d) `--ir_center` subtracts the mean of the whole batch: every centred element is one float32 rounding of the exact
      difference (relative error <= 2^-24), and the float64 mean of the exact differences is zero up to the float64 sums,
      so |mean of the centred rewards over both ranks| <= 2^-24 * max|x| < 2^-23 * max|int_rewards| - derived, not measured.

One pair of child processes serves every test of the module: each rank records what it saw, the tests compare."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, A, WORLD = 4, 8, 2

WORKER = r'''
import os, sys, hashlib
sys.path.insert(0, sys.argv[1])
import numpy as np, torch, torch.distributed as dist
from ppo_amd import envs, logger, models, parallel, rollout
from ppo_amd.config import args
from ppo_amd.running_stats import RunningMeanStd
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
torch.cuda.set_device(0)
dist.init_process_group("gloo", rank=rank, world_size=world)
FLAGS = ["--agents=8", "--n_steps=4", "--model_architecture=single", "--model_encoder=nature", "--env_type=synthetic",
         "--env_embed_time=False", "--seed=3", "--device=cuda", "--policy_opt_mini_batch_size=32",
         "--rnd_opt_mini_batch_size=16", "--disable_logging=True", "--rnd_enabled=True", "--observation_normalization=True"]
out = {}


def digest(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return np.array(h.hexdigest())


def make_model():
    torch.manual_seed(1000 + rank)   # DIFFERENT initial weights per rank, target and predictor included
    np.random.seed(100 + rank)
    shape, nA = envs.get_env_spec()
    assert shape == (4, 84, 84)
    return models.TVFModel("nature", input_dims=shape, actions=nA, device="cuda", architecture="single", hidden_units=256,
                           head_scale=0.1, head_bias=True, use_rnd=True, observation_normalization=True,
                           value_head_names=("ext", "int"))


def make_runner(model):
    r = rollout.Runner(model, logger.Logger(quiet=True))
    assert r.world == 2 and r.rank == rank and r.value_heads == ["ext", "int"]
    r.vec_env = envs.create_envs_classic(rank=rank, world=world)
    r.reset()
    return r


# ---- (a) replicas
args.setup(FLAGS)
model = make_model()
rnd = model.rnd
out["a_target_before"], out["a_pred_before"] = digest(rnd.target_net.flat), digest(rnd.prediction_net.flat)
r = make_runner(model)
out["a_target_after"], out["a_pred_after"] = digest(rnd.target_net.flat), digest(rnd.prediction_net.flat)
assert id(rnd) in r._reducers and r._reducers[id(rnd)].split == 0 and rnd.grad_ready_hook is None

# ---- (b) one RND minibatch step with the reduction observed
r.generate_rollout()
pred_initial = rnd.prediction_net.flat.clone()
assert rnd.exp_avg is None and rnd.adam_steps == 0
obs_all = r.all_obs[:r.N].view(r.N * r.A, *r.state_shape)
idx = torch.arange(8, dtype=torch.int32, device="cuda")
rnd.train_minibatch(obs_all, idx, 1.0, stats=r._rnd_stats)
out["b_grad"] = rnd.prediction_net.grad.cpu().numpy()
red, seen = r._reducers[id(rnd)], []
finish = red.finish


def observed_finish(*a, **kw):
    finish(*a, **kw)
    seen.append(rnd.prediction_net.grad.clone())


red.finish = observed_finish
norm = r.optimizer_step(r.rnd_optimizer, "rnd")
red.finish = finish
torch.cuda.synchronize()
assert len(seen) == 1
out["b_reduced"] = seen[0].cpu().numpy()
out["b_norm"] = np.float64(norm.item())
out["b_max_grad_norm"] = np.float64(args.max_grad_norm if args.grad_clip_mode == "global_norm" else 0.0)
out["b_pred_changed"] = np.array(not torch.equal(rnd.prediction_net.flat, pred_initial))
out["b_moments_nonzero"] = np.array(bool(rnd.exp_avg.abs().max() > 0 and rnd.exp_avg_sq.abs().max() > 0))
out["b_pred"], out["b_moments"] = digest(rnd.prediction_net.flat), digest(rnd.exp_avg, rnd.exp_avg_sq)
out["b_exp_avg"] = rnd.exp_avg.cpu().numpy()
out["b_adam_steps"] = np.array(rnd.adam_steps)

# ---- (c), (d) two whole iterations with the normaliser and the centring on
args.setup([*FLAGS, "--ir_normalize=True", "--ir_center=True"])
assert args.ir.propagation
r = make_runner(make_model())
rnd = r.rnd
ems, rms = np.zeros([world * 8]), RunningMeanStd(shape=())
for it in range(2):
    r.generate_rollout()
    # the clipped rewards of both ranks together, before they are normalised: what the host filter must have seen
    raw = np.clip(parallel.gather_columns(r.int_rewards).cpu().numpy(), -5, 5)
    ems, scale = rollout.intrinsic_return_scale(ems, rms, raw, np.zeros(raw.shape, bool), args.gamma_int, True)
    r.calculate_returns()
    out[f"c_centred_{it}"] = r.int_rewards.cpu().numpy()
    out[f"c_raw_{it}"] = raw
    r.train()
torch.cuda.synchronize()
out["c_want_ems"], out["c_want_scale"] = ems, np.float64(scale)
out["c_want_rms"] = np.asarray([rms.mean, rms.var, rms.count], np.float64)
out["c_ems"], out["c_scale"] = np.asarray(r.ems_norm), np.float64(r.intrinsic_reward_norm_scale)
m = r.intrinsic_returns_rms
out["c_rms"] = np.asarray([m.mean, m.var, m.count], np.float64)
out["c_pred"] = digest(rnd.prediction_net.flat, rnd.exp_avg, rnd.exp_avg_sq)
out["c_policy"] = digest(r.net.flat, r.net.exp_avg, r.net.exp_avg_sq)
out["c_target"] = digest(rnd.target_net.flat)
out["c_adam_steps"] = np.array(rnd.adam_steps)
rows = round(4 * 8 * args.rnd.experience_proportion)
out["c_adam_steps_implied"] = np.array(2 * args.rnd_opt.epochs * (rows // (args.rnd_opt.mini_batch_size // world)))
out["c_finite"] = np.array(bool(torch.isfinite(rnd.prediction_net.flat).all() and torch.isfinite(r.net.flat).all()))
parallel.assert_identical_across_ranks([rnd.prediction_net.flat, rnd.target_net.flat, rnd.exp_avg, rnd.exp_avg_sq,
                                        r.net.flat, r.net.exp_avg, r.net.exp_avg_sq], "replicas after two iterations")
dist.barrier(); dist.destroy_process_group()
np.savez(os.path.join(sys.argv[2], f"r{rank}.npz"), **out)
print("rank", rank, "ok")
'''


@pytest.fixture(scope="module")
def ranks(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("dp_rnd")
    script = tmp / "dp_rnd_worker.py"
    script.write_text(WORKER)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29573", WORLD_SIZE="2")
    procs = [subprocess.Popen([sys.executable, str(script), ROOT, str(tmp)], env=dict(env, RANK=str(r)),
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(2)]
    try:
        outs = [p.communicate(timeout=300)[0] for p in procs]
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


def test_target_and_predictor_are_rank_0s_after_init(ranks):
    r0, r1 = ranks
    for net in ("target", "pred"):
        assert str(r0[f"a_{net}_before"]) != str(r1[f"a_{net}_before"]), "the test did not start the replicas apart"
        assert str(r0[f"a_{net}_after"]) == str(r1[f"a_{net}_after"]) == str(r0[f"a_{net}_before"]), \
            f"Runner.__init__ did not broadcast rank 0's {net} net"


def test_predictor_gradient_is_summed_over_ranks_before_adam(ranks):
    r0, r1 = ranks
    g0, g1 = r0["b_grad"], r1["b_grad"]
    assert g0.dtype == np.float32 and np.abs(g0).max() > 0 and not same(g0, g1), "the ranks trained on the same rows"
    want = g0 + g1  # float32, one rounding per element
    assert same(r0["b_reduced"], want) and same(r1["b_reduced"], want)
    # Adam divided the sum by the world size: the norm it reports is that of the mean gradient ...
    norm = float(np.sqrt(np.sum(np.square(want.astype(np.float64))))) / WORLD
    print(f"DP_RND reported norm {float(r0['b_norm']):.9g} want {norm:.9g}")
    assert float(r0["b_norm"]) == float(r1["b_norm"]) and abs(float(r0["b_norm"]) - norm) <= 1e-3 * norm
    # ... and the first step's first moment is (1 - beta1) times the clipped mean gradient
    max_norm = float(r0["b_max_grad_norm"])
    clip = min(1.0, max_norm / (norm + 1e-6)) if max_norm > 0 else 1.0
    m = 0.1 * clip * want.astype(np.float64) / WORLD
    assert np.abs(r0["b_exp_avg"] - m).max() <= 1e-3 * np.abs(m).max()
    for r in ranks:
        assert bool(r["b_pred_changed"]) and bool(r["b_moments_nonzero"]) and int(r["b_adam_steps"]) == 1
    assert str(r0["b_pred"]) == str(r1["b_pred"]) and str(r0["b_moments"]) == str(r1["b_moments"])


def test_replicas_and_normaliser_stay_identical_over_whole_iterations(ranks):
    r0, r1 = ranks
    for key in ("c_pred", "c_policy", "c_target"):
        assert str(r0[key]) == str(r1[key]), f"{key[2:]} replicas diverged"
    assert bool(r0["c_finite"]) and bool(r1["c_finite"])
    assert r0["c_ems"].shape == (WORLD * A,) and r0["c_ems"].dtype == np.float64
    for key in ("c_ems", "c_scale", "c_rms"):
        assert same(r0[key], r1[key]), f"{key[2:]} differs across ranks"
    # both ranks gathered the same global rewards, and the run's state is the filter's over them
    for it in range(2):
        assert same(r0[f"c_raw_{it}"], r1[f"c_raw_{it}"]) and r0[f"c_raw_{it}"].shape == (N, WORLD * A)
    for r in ranks:
        assert same(r["c_ems"], r["c_want_ems"]) and same(r["c_scale"], r["c_want_scale"]) and same(r["c_rms"], r["c_want_rms"])
    # the running variance took in the filter's output over all 16 envs at each of the 2 x 4 steps
    assert float(r0["c_scale"]) != 1.0 and abs(r0["c_rms"][2] - 2 * N * WORLD * A) < 1e-3
    assert int(r0["c_adam_steps"]) == int(r1["c_adam_steps"]) == int(r0["c_adam_steps_implied"]) == 2


@pytest.mark.parametrize("it", [0, 1])
def test_centred_rewards_have_zero_mean_over_both_ranks(ranks, it):
    x = np.concatenate([r[f"c_centred_{it}"] for r in ranks], axis=1).astype(np.float64)
    assert x.shape == (N, WORLD * A) and np.abs(x).max() > 0
    mean, bound = abs(float(x.mean())), 2.0 ** -23 * float(np.abs(x).max())
    print(f"DP_RND it {it} |mean| {mean:.3e} bound {bound:.3e}")
    assert mean <= bound
    # each rank's own mean is not zero: the centring used the global moments
    own = [abs(float(r[f"c_centred_{it}"].astype(np.float64).mean())) for r in ranks]
    assert max(own) > bound, own
