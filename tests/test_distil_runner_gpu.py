"""GPU: the distillation switches in the Runner (--distil_loss, --distil_value_loss, --distil_target, --distil_max_heads;
rl/rollout.py:1331-1449, 2050-2112): the batch get_distil_batch builds for return / advantage targets against the GAE
oracle on the rollout's own buffers, which recorded policy each loss is held to, a full train() under every new mode, a
split minibatch, the refusals that stay, and that the default flags still run the bits they ran.

Two small runners: an MLP dual runner on a float env with 6 discrete actions (8 agents x 8 steps, the fused MLP launches)
and the IMPALA dual runner of tests/test_sns_runner_gpu.py on the synthetic env (16 x 16, the op-by-op loss launch)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from oracle import returns as O  # noqa: E402 (checker)
from ppo_amd import logger, models, rollout, tvf  # noqa: E402
from ppo_amd.config import args  # noqa: E402
from ppo_amd.value_quality import even_sample_down  # noqa: E402
from ppo_amd.vec_env import SplitVecEnv, SyntheticVecEnv  # noqa: E402

N_ACTIONS, MLP_DIM, IMPALA_DIMS = 6, 4, (4, 84, 84)
COMMON = ["--seed=5", "--device=cuda", "--disable_logging=True", "--model_architecture=dual", "--env_type=synthetic",
          "--env_embed_time=False", "--policy_opt_epochs=1", "--value_opt_epochs=1", "--distil_opt_epochs=2",
          "--gamma=0.99", "--tvf_gamma=0.97", "--distil_adv_lambda=0.8", "--distil_beta=0.7"]
STAT_KEYS = ("loss_distil_value", "loss_distil_policy", "loss_distil", "distil_mse", "grad_distil")


@pytest.fixture(autouse=True)
def restore_micro_batch_size():
    """--max_micro_batch_size is a top-level flag: a later args.setup() without it would keep the value."""
    before = args.max_micro_batch_size
    yield
    args.max_micro_batch_size = before


class DiscreteFloatVecEnv:
    """Deterministic in-process vector env: flat float observations, discrete actions the reward depends on."""

    def __init__(self, A, dim, seed):
        self.num_envs, self.dim = A, dim
        self.rng = np.random.default_rng(seed)
        self.t = np.zeros(A, np.int64)

    def reset(self):
        self.t[:] = 0
        return self.rng.standard_normal((self.num_envs, self.dim)).astype(np.float32)

    def step(self, actions):
        actions = np.asarray(actions)
        assert actions.shape == (self.num_envs,)
        self.t += 1
        rew = (0.5 * (actions % 3) - 0.3 + 0.1 * self.rng.standard_normal(self.num_envs)).astype(np.float32)
        done = self.rng.random(self.num_envs) < 0.1
        infos = [{"time": int(t), "ep_length": int(t), "ep_score": float(t)} for t in self.t]
        self.t[done] = 0
        return self.rng.standard_normal((self.num_envs, self.dim)).astype(np.float32), rew, done, infos


def mlp_runner(extra=(), use_tvf=False, action_dist="discrete", env=True):
    flags = [*COMMON, "--model_encoder=mlp", "--model_hidden_units=64", "--agents=8", "--n_steps=8",
             "--policy_opt_mini_batch_size=32", "--value_opt_mini_batch_size=32", "--distil_opt_mini_batch_size=32"]
    if use_tvf:
        flags += ["--tvf_enabled=True", "--tvf_value_heads=8", "--tvf_max_horizon=100", "--tvf_return_samples=4"]
    args.setup([*flags, *extra])
    assert args._ignored == []
    torch.manual_seed(5)
    np.random.seed(5)
    horizons = weights = None
    if use_tvf:
        horizons, weights = tvf.get_value_head_horizons(args.tvf.value_heads, args.tvf.max_horizon, args.tvf.head_spacing,
                                                        include_weight=True)
    model = models.TVFModel("mlp", input_dims=(MLP_DIM,), actions=N_ACTIONS, device="cuda", architecture="dual",
                            hidden_units=64, encoder_activation_fn="tanh", tvf_fixed_head_horizons=horizons,
                            tvf_fixed_head_weights=weights, head_scale=0.1, head_bias=True, value_head_names=("ext",))
    assert model.policy_net.mlp_fused
    r = rollout.Runner(model, logger.Logger(quiet=True), action_dist=action_dist)
    if env:
        r.vec_env = DiscreteFloatVecEnv(8, MLP_DIM, seed=4)
        r.reset()
    return r


def impala_runner(extra=()):
    args.setup([*COMMON, "--model_encoder=impala", "--env_synthetic_shape=4,84,84", "--agents=16", "--n_steps=16",
                "--policy_opt_mini_batch_size=128", "--value_opt_mini_batch_size=128", "--distil_opt_mini_batch_size=128",
                *extra])
    assert args._ignored == []
    np.random.seed(11)
    torch.manual_seed(5)
    model = models.TVFModel(encoder="impala", input_dims=IMPALA_DIMS, actions=N_ACTIONS, device="cuda", architecture="dual",
                            hidden_units=64, head_scale=0.1, head_bias=True, value_head_names=("ext",))
    r = rollout.Runner(model, logger.Logger(quiet=True))
    r.vec_env = SplitVecEnv([SyntheticVecEnv(8, obs_shape=IMPALA_DIMS, n_actions=N_ACTIONS, seed=3, p_done=0.1,
                                             env_offset=i * 8, threads=2) for i in range(2)])
    r.reset()
    return r


def make(encoder, extra=(), **kw):
    return mlp_runner(extra, **kw) if encoder == "mlp" else impala_runner(extra)


def collect(r, seed=21):
    r.generate_rollout()
    np.random.seed(seed)
    r.calculate_returns()
    torch.cuda.synchronize()


@pytest.mark.parametrize("encoder,target,order,loss", [
    ("mlp", "return", "before_policy", "mse_logit"), ("mlp", "advantage", "after_policy", "mse_logit"),
    ("mlp", "advantage", "before_policy", "mse_policy"), ("mlp", "return", "after_policy", "kl_policy"),
    ("impala", "advantage", "after_policy", "mse_logit"), ("impala", "return", "before_policy", "kl_policy")])
def test_return_and_advantage_batches(encoder, target, order, loss):
    r = make(encoder, [f"--distil_target={target}", f"--distil_order={order}", f"--distil_loss={loss}"])
    collect(r)
    r._phase_stats = {}
    r.train_policy()  # the policy moves: `after_policy` must re-evaluate it, `before_policy` must not
    torch.cuda.synchronize()
    N, A = r.N, r.A
    B = N * A
    batch = r.get_distil_batch()
    torch.cuda.synchronize()
    # targets: GAE(tvf_gamma, distil_adv_lambda) on the rollout's own buffers, to the bar of the GAE tests
    assert (args.tvf.gamma, args.distil.adv_lambda) == (0.97, 0.8)
    rew, done = r.ext_rewards.cpu().numpy(), r.terminals.cpu().numpy()
    val = r.ext_value.cpu().numpy()
    adv, ret = O.gae_and_returns(rew, val[:N], val[N], done, 0.97, 0.8, 0.8)
    want = adv if target == "advantage" else adv + val[:N]
    if target == "return":
        assert np.abs(ret - want).max() <= 1e-6 * np.abs(want).max()
    got = batch["distil_targets"].cpu().numpy()
    assert got.shape == (B,) and batch["use_tvf"] is False
    err = np.abs(got - want.reshape(B)).max()
    print(f"{target}: max err {err / np.abs(want).max():.3e} of the largest target (bar 1e-05)")
    assert err <= 1e-5 * np.abs(want).max()
    other = np.abs(got - (adv + val[:N] if target == "advantage" else adv).reshape(B)).max()
    # and not the other target: the two differ by the value estimates, which are at least 100 bars large
    assert np.abs(val[:N]).max() > 1e-3 * np.abs(want).max() and other > 0.9 * np.abs(val[:N]).max()
    # the rollout's actions
    assert batch["distil_actions"].dtype == torch.int32 and batch["distil_actions"].is_contiguous()
    assert torch.equal(batch["distil_actions"], r.actions.reshape(B))
    # the policy to stay close to: raw logits for mse_logit, the log-policy otherwise; recorded or re-evaluated
    key = "raw_policy" if loss == "mse_logit" else "log_policy"
    recorded = getattr(r, key).reshape(B, N_ACTIONS)
    obs = r.all_obs[:N].reshape(B, *r.state_shape)
    chunk = max(args.max_micro_batch_size, 1)
    now = torch.cat([r.policy_net.forward(obs[i:i + chunk], exclude_value=True)[key].clone() for i in range(0, B, chunk)])
    assert not torch.equal(recorded, now)
    assert torch.equal(batch["old_policy"], recorded if order == "before_policy" else now)
    lse = torch.logsumexp(batch["old_policy"], dim=1)
    if key == "log_policy":
        assert float(lse.abs().max()) < 1e-5
    else:
        assert float(lse.abs().max()) > 1e-3  # raw logits are not normalised


MODES = {
    "logit_l1": ["--distil_loss=mse_logit", "--distil_value_loss=l1"],
    "policy_clipped": ["--distil_loss=mse_policy", "--distil_value_loss=clipped_mse"],
    "kl_huber": ["--distil_value_loss=huber", "--distil_delta=0.1"],
    "huber0": ["--distil_value_loss=huber", "--distil_delta=0"],
    "advantage": ["--distil_target=advantage"],
    "return_before": ["--distil_target=return", "--distil_order=before_policy", "--distil_loss=mse_logit"],
    "tvf_heads3": ["--distil_max_heads=3", "--distil_value_loss=huber"],
}


@pytest.mark.parametrize("encoder,mode", [("mlp", m) for m in MODES] + [("impala", "logit_l1"), ("impala", "advantage")])
def test_full_train_under_every_mode(encoder, mode):
    r = make(encoder, MODES[mode], use_tvf=mode == "tvf_heads3") if encoder == "mlp" else make(encoder, MODES[mode])
    collect(r)
    pol, val = r.policy_net, r.value_net
    seen = {}
    phase = r.train_distil

    def watched():
        torch.cuda.synchronize()
        seen["before"] = (pol.flat.clone(), val.flat.clone())
        phase()
        torch.cuda.synchronize()
        seen["after"] = (pol.flat.clone(), val.flat.clone())
    r.train_distil = watched
    r.train()
    torch.cuda.synchronize()
    assert not torch.equal(seen["before"][0], seen["after"][0]), "the distil phase did not move policy_net"
    assert torch.equal(seen["before"][1], seen["after"][1]), "the distil phase moved value_net"
    assert bool(torch.isfinite(pol.flat).all())
    stats = r.fetch_stats()
    for k in STAT_KEYS:
        assert np.isfinite(stats[k]), (k, stats[k])
    assert stats["loss_distil_value"] > 0 and stats["distil_mse"] > 0
    if mode == "tvf_heads3":
        # heads outside even_sample_down(range(K), 3) are not trained by the distil phase
        K, H = r.K, 64
        subset = [int(k) for k in even_sample_down(range(K), 3)]
        assert K > 3 and len(subset) == 3 and subset[-1] == K - 1
        w0 = seen["before"][0][pol._offsets["tvf_head.weight"][0]:][:K * H].view(K, H)
        w1 = seen["after"][0][pol._offsets["tvf_head.weight"][0]:][:K * H].view(K, H)
        moved = [bool((w0[k] != w1[k]).any()) for k in range(K)]
        assert moved == [k in subset for k in range(K)], moved


def rel(a, b):
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-30)


def test_split_minibatch_gives_the_unsplit_update():
    """--max_micro_batch_size = half a distil minibatch: the accumulated passes give the one-pass update, to the bar of
    tests/test_train_batch_gpu.py (the optimiser's first moment within 1e-4 of its largest entry)."""
    flags = ["--distil_target=advantage", "--distil_loss=mse_policy", "--distil_value_loss=huber",
             "--distil_order=before_policy"]
    runs = []
    for micro in (None, 16):
        r = mlp_runner(flags + ([f"--max_micro_batch_size={micro}"] if micro else []))
        collect(r)
        np.random.seed(77)
        r._phase_stats = {}
        r.train_distil()
        torch.cuda.synchronize()
        runs.append(r)
    one, two = runs
    assert one.distil_optimizer.state.step == two.distil_optimizer.state.step == 2 * 2
    assert torch.equal(one.actions, two.actions) and not torch.equal(one.policy_net.flat, mlp_runner(flags).policy_net.flat)
    err = rel(two.distil_optimizer.state.exp_avg, one.distil_optimizer.state.exp_avg)
    print(f"split vs unsplit first moment: {err:.3e} of the largest entry (bar 1e-04)")
    assert err < 1e-4
    a, b = one.fetch_stats(), two.fetch_stats()
    for k in STAT_KEYS[:4]:
        assert abs(a[k] - b[k]) <= 1e-5 * max(1.0, abs(a[k])), k


def test_refusals_that_stay():
    r = mlp_runner(["--distil_target=return"], use_tvf=True)
    collect(r)
    with pytest.raises(AssertionError, match="Only value targets supported for TVF distil"):
        r.get_distil_batch()
    # ... but with --distil_force_ext the ext head is distilled and any target goes
    r = mlp_runner(["--distil_target=return", "--distil_force_ext=True"], use_tvf=True)
    collect(r)
    assert "distil_actions" in r.get_distil_batch()
    r = mlp_runner(["--distil_target=return", "--replay_mode=uniform", "--replay_size=64"])
    assert r.replay_buffer is not None
    with pytest.raises(AssertionError, match="value targets"):
        r.get_distil_batch()
    r = mlp_runner(["--distil_target=advantage"], action_dist="gaussian", env=False)
    with pytest.raises(ValueError, match="needs discrete actions"):
        r.get_distil_batch()


DEFAULTS = ["--distil_loss=kl_policy", "--distil_value_loss=mse", "--distil_target=value", "--distil_max_heads=-1",
            "--distil_delta=0.1", "--distil_l1_scale=0.0333", "--distil_adv_lambda=0.6"]


@pytest.mark.parametrize("encoder", ["mlp", "impala"])
def test_default_flags_run_what_they_ran(encoder):
    """One iteration with the default switches spelled out, against a runner whose distil step is the call from before
    the switches existed - no mode keyword passed, and on the op-by-op path the old C entry ppo_distil_loss_f32 with
    its 17 arguments: byte-identical policy_net."""
    new = make(encoder, DEFAULTS)
    old = make(encoder)
    net = old.policy_net

    def old_step(prev_state, targets, old_policy, use_tvf, pred_actions=None, **kw):
        assert pred_actions is None
        return net.distil_minibatch(prev_state, targets, old_policy, beta=args.distil.beta, use_tvf=use_tvf, weights=None,
                                    gaussian=False, **kw)
    old._distil_step = old_step
    calls = []
    call = net._call

    def old_entry(fn, *a):
        calls.append(fn)
        if fn == "ppo_distil_loss_modes_f32":
            assert a[17:] == (0, 0, 0.0, 0.0, None, 0)
            return call("ppo_distil_loss_f32", *a[:17])
        return call(fn, *a)
    net._call = old_entry
    for r in (new, old):
        collect(r)
        np.random.seed(31)
        r.train()
        torch.cuda.synchronize()
    assert ("ppo_distil_loss_modes_f32" in calls) == (encoder == "impala")
    assert torch.equal(new.all_obs, old.all_obs) and new.distil_optimizer.state.step == old.distil_optimizer.state.step > 0
    assert new.policy_net.flat.cpu().numpy().tobytes() == old.policy_net.flat.cpu().numpy().tobytes()
    assert new.value_net.flat.cpu().numpy().tobytes() == old.value_net.flat.cpu().numpy().tobytes()
