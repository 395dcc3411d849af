"""GPU: --*_opt_optimizer=sgd in the Runner (ppo_amd/rollout.py, models.py, rnd.py): which launch a phase takes, that an SGD
optimiser keeps no moments and no step count, one optimizer_step against float64 (tests/sgd_float64.py) with the packed
convolution operands following the new weights, every combination of kinds in the dual architecture, the RND predictor,
checkpoints in torch.optim.SGD's layout that refuse the other kind, and --*_opt_adam_beta1=-1 end to end.

Two small runners: an MLP dual TVF runner of 16 agents x 16 steps (tests/test_sns_runner_gpu.py's; the fused MLP backward
leaves the partial sums of g^2, so its optimiser steps take the presummed entry point) and a nature-CNN runner of 8 agents
x 4 steps on 36 x 36 synthetic frames with a minibatch of 32 (the plain entry point; convolution weights with packed
operands), with and without RND."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import policy_optim_float64 as R  # noqa: E402
import sgd_float64 as S  # noqa: E402
from ppo_amd import checkpoint, logger, models, rollout, tvf  # noqa: E402
from ppo_amd.config import args  # noqa: E402
from ppo_amd.vec_env import SplitVecEnv, SyntheticVecEnv  # noqa: E402

DIMS, N_ACTIONS = (4, 36, 36), 6
NATURE = ["--model_encoder=nature", "--env_type=synthetic", "--env_embed_time=False", "--env_synthetic_shape=4,36,36",
          "--seed=5", "--disable_logging=True", "--device=cuda", "--agents=8", "--n_steps=4",
          "--policy_opt_mini_batch_size=32", "--policy_opt_epochs=1", "--value_opt_mini_batch_size=32", "--value_opt_epochs=1",
          "--distil_opt_mini_batch_size=32", "--rnd_opt_mini_batch_size=8"]
MLP = ["--seed=5", "--device=cuda", "--agents=16", "--n_steps=16", "--disable_logging=True",
       "--policy_opt_mini_batch_size=64", "--value_opt_mini_batch_size=64", "--distil_opt_mini_batch_size=64",
       "--model_architecture=dual", "--model_encoder=mlp", "--model_hidden_units=64", "--env_type=mujoco", "--env_name=Fake",
       "--tvf_enabled=True", "--tvf_value_heads=5", "--tvf_max_horizon=100", "--tvf_return_samples=4",
       "--env_reward_normalization=off"]


def nature_runner(extra=(), rnd=False, seed=5):
    args.setup([*NATURE, "--model_architecture=single", *(["--rnd_enabled=True", "--observation_normalization=True"] if rnd else []),
                *extra])
    np.random.seed(11)
    torch.manual_seed(seed)
    model = models.TVFModel(encoder="nature", input_dims=DIMS, actions=N_ACTIONS, device="cuda", architecture="single",
                            hidden_units=64, use_rnd=rnd, observation_normalization=rnd, head_scale=0.1, head_bias=True,
                            value_head_names=("ext", "int") if rnd else ("ext",))
    r = rollout.Runner(model, logger.Logger(quiet=True))
    r.vec_env = SplitVecEnv([SyntheticVecEnv(4, obs_shape=DIMS, n_actions=N_ACTIONS, seed=3, p_done=0.1, env_offset=i * 4,
                                             threads=2) for i in range(2)])
    r.reset()
    return r


class FloatVecEnv:
    """Deterministic in-process vector env with flat float observations and continuous actions."""

    def __init__(self, A, dim, seed):
        self.num_envs, self.dim = A, dim
        self.rng = np.random.default_rng(seed)
        self.t = np.zeros(A, np.int64)

    def reset(self):
        self.t[:] = 0
        return self.rng.standard_normal((self.num_envs, self.dim)).astype(np.float32)

    def step(self, actions):
        self.t += 1
        rew = (1.0 - 0.1 * np.square(actions).sum(1)).astype(np.float32)
        done = self.rng.random(self.num_envs) < 0.05
        infos = [{"time": int(t), "ep_length": int(t), "ep_score": float(t)} for t in self.t]
        self.t[done] = 0
        return self.rng.standard_normal((self.num_envs, self.dim)).astype(np.float32), rew, done, infos


def mlp_runner(extra=(), seed=9):
    args.setup([*MLP, *extra])
    torch.manual_seed(seed)
    np.random.seed(seed)
    horizons, weights = tvf.get_value_head_horizons(args.tvf.value_heads, args.tvf.max_horizon, args.tvf.head_spacing,
                                                    include_weight=True)
    model = models.TVFModel("mlp", input_dims=(11,), actions=3, device="cuda", architecture="dual", hidden_units=64,
                            encoder_activation_fn="tanh", tvf_fixed_head_horizons=horizons, tvf_fixed_head_weights=weights,
                            head_scale=0.1, head_bias=True)
    r = rollout.Runner(model, logger.Logger(quiet=True), action_dist="gaussian")
    r.vec_env = FloatVecEnv(16, 11, seed=4)
    r.reset()
    assert r.policy_net.mlp_fused and r.value_net.mlp_fused
    return r


def collect(r, seed=1):
    r.generate_rollout()
    np.random.seed(seed)
    r.calculate_returns()
    torch.cuda.synchronize()


def record_calls(net):
    """The names of the library entry points the net calls from now on."""
    seen, original = [], net._call

    def call(name, *a):
        seen.append(name)
        return original(name, *a)
    net._call = call
    return seen


def optimiser_calls(seen):
    return [n for n in seen if n.startswith(("ppo_adam_step", "ppo_sgd_step"))]


def moments(net):
    return None if net.exp_avg is None else (net.exp_avg.clone(), net.exp_avg_sq.clone())


def torch_sgd_dict(n, lr):
    return torch.optim.SGD([torch.nn.Parameter(torch.zeros(1)) for _ in range(n)], lr=lr).state_dict()


# ---------------------------------------------------------------- policy phase
@pytest.mark.parametrize("kind", ["mlp", "nature"])
def test_policy_phase_with_sgd_takes_the_sgd_launch_and_keeps_no_moments(kind):
    r = (mlp_runner if kind == "mlp" else nature_runner)(["--policy_opt_optimizer=sgd"])
    assert r.policy_optimizer.kind == "sgd"
    collect(r)
    net = r.policy_net
    before, seen = net.flat.clone(), record_calls(net)
    r.train_policy()
    torch.cuda.synchronize()
    n_steps = args.policy_opt.epochs * (r.N * r.A // args.policy_opt.mini_batch_size)
    entry = "ppo_sgd_step_presummed_f32" if kind == "mlp" else "ppo_sgd_step_f32"
    assert optimiser_calls(seen) == [entry] * n_steps and n_steps >= 1
    assert not torch.equal(net.flat, before) and bool(torch.isfinite(net.flat).all())
    assert net.exp_avg is None and net.exp_avg_sq is None and net._adam_step == 0
    norms = r._phase_stats["policy"][1]
    assert norms.numel() == n_steps and bool((norms > 0).all()) and bool(torch.isfinite(norms).all())


# ---------------------------------------------------------------- optimizer_step
@pytest.mark.parametrize("clip_mode", ["global_norm", "off"])
def test_optimizer_step_against_float64_and_the_packed_operands_follow(clip_mode):
    lr = 0.01
    r = nature_runner(["--policy_opt_optimizer=sgd", f"--policy_opt_lr={lr}", f"--grad_clip_mode={clip_mode}", "--max_grad_norm=5"])
    net = r.policy_net
    x = torch.from_numpy(np.random.default_rng(3).integers(0, 256, (8, *DIMS), dtype=np.uint8)).cuda()
    out0 = {k: v.clone() for k, v in net.forward(x).items() if k in ("raw_policy", "value")}  # packs the operands
    g = torch.Generator().manual_seed(7)
    grad = (torch.randn(net.grad.numel(), generator=g) * 0.1).numpy()
    net.grad.copy_(torch.from_numpy(grad))
    w = net.flat.cpu().numpy().copy()
    seen = record_calls(net)
    norm = r.optimizer_step(r.policy_optimizer, "policy")
    torch.cuda.synchronize()
    assert optimiser_calls(seen) == ["ppo_sgd_step_f32"]
    mn = np.float32(5.0 if clip_mode == "global_norm" else 0.0)
    ref = S.sgd_ref(w, [grad], mn, 1.0, lr=lr)
    assert clip_mode == "off" or ref[0]["norm"] > 5.0, "the clip does not act in this case"
    got = [{"w": net.flat.cpu().numpy(), "norm": float(norm.item())}]
    e, e32 = S.sgd_errs(got, ref), S.sgd_errs(S.sgd_f32(w, [grad], mn, 1.0, lr=lr), ref)
    for k in ("w", "norm"):
        bar = R.report(f"sgd optimizer_step clip={clip_mode} {k}", e[k], e32[k])
        assert e[k] <= bar, f"{k} {e[k]:.3e} over the bar {bar:.3e}"
    assert net.exp_avg is None and net._adam_step == 0
    # a forward of the stepped net is a forward of a fresh net holding the same parameters
    out1 = net.forward(x)
    torch.manual_seed(99)
    fresh = models.TVFModel(encoder="nature", input_dims=DIMS, actions=N_ACTIONS, device="cuda", architecture="single",
                            hidden_units=64, head_scale=0.1, head_bias=True, value_head_names=("ext",))
    fresh.load_state_dict(r.model.state_dict())
    out2 = fresh.policy_net.forward(x)
    for k in ("raw_policy", "value"):
        assert R.same_bits(out1[k], out2[k]), f"{k}: the packed operands did not follow the step"
        assert not torch.equal(out1[k], out0[k]), f"{k}: the step did not change the forward"


def test_lr_anneal_reaches_the_sgd_launch():
    r = nature_runner(["--policy_opt_optimizer=sgd", "--policy_opt_lr=0.01", "--policy_opt_lr_anneal=True"])
    seen = []
    step = r.policy_net.sgd_step
    r.policy_net.sgd_step = lambda **kw: (seen.append(kw["lr"]), step(**kw))[1]
    r.policy_net.grad.fill_(0.01)
    r.optimizer_step(r.policy_optimizer, "policy")
    torch.cuda.synchronize()
    assert seen == [r._lr(args.policy_opt)]


# ---------------------------------------------------------------- kind combinations
@pytest.mark.parametrize("value_kind,distil_kind", [("sgd", "adam"), ("adam", "sgd")])
def test_each_phase_touches_only_its_own_kind_of_state(value_kind, distil_kind):
    r = mlp_runner([f"--value_opt_optimizer={value_kind}", f"--distil_opt_optimizer={distil_kind}"])
    pol, val, dis = r.policy_net, r.value_net, r.distil_optimizer
    assert (r.policy_optimizer.kind, r.value_optimizer.kind, dis.kind) == ("adam", value_kind, distil_kind)
    assert (dis.state is None) == (distil_kind == "sgd")
    collect(r)
    r.train_policy()
    assert pol._adam_step > 0 and pol.exp_avg is not None and val._adam_step == 0 and val.exp_avg is None
    pol_step, pol_m, val_flat, pol_flat = pol._adam_step, moments(pol), val.flat.clone(), pol.flat.clone()
    seen_v = record_calls(val)
    r.train_value()
    torch.cuda.synchronize()
    assert not torch.equal(val.flat, val_flat) and torch.equal(pol.flat, pol_flat)
    calls = set(optimiser_calls(seen_v))
    if value_kind == "sgd":
        assert calls == {"ppo_sgd_step_presummed_f32"} and val._adam_step == 0 and val.exp_avg is None
    else:
        assert calls == {"ppo_adam_step_presummed_f32"} and val._adam_step > 0 and val.exp_avg is not None
    val_flat, val_step = val.flat.clone(), val._adam_step
    seen_p = record_calls(pol)
    r.train_distil()
    torch.cuda.synchronize()
    assert not torch.equal(pol.flat, pol_flat) and torch.equal(val.flat, val_flat) and val._adam_step == val_step
    # the policy optimiser's own moments are not the distil phase's, whatever its kind
    assert pol._adam_step == pol_step and all(torch.equal(a, b) for a, b in zip(moments(pol), pol_m))
    calls = set(optimiser_calls(seen_p))
    if distil_kind == "sgd":
        assert calls == {"ppo_sgd_step_presummed_f32"} and dis.state is None
    else:
        assert calls == {"ppo_adam_step_presummed_f32"} and dis.state.step > 0 and dis.state.exp_avg.abs().max() > 0
    # and the checkpoint entries carry each optimiser's own layout
    kinds = {"policy": "adam", "value": value_kind, "distil": distil_kind}
    for name, opt in (("policy", r.policy_optimizer), ("value", r.value_optimizer), ("distil", dis)):
        assert models.optimizer_layout_kind(opt.state_dict()) == kinds[name], name


def test_distil_on_the_policy_optimiser_takes_its_kind():
    r = mlp_runner(["--policy_opt_optimizer=sgd", "--distil_use_policy_opt=True"])
    assert r.distil_optimizer is None
    collect(r)
    pol = r.policy_net
    seen = record_calls(pol)
    r.train_distil()
    torch.cuda.synchronize()
    assert set(optimiser_calls(seen)) == {"ppo_sgd_step_presummed_f32"} and pol.exp_avg is None and pol._adam_step == 0


# ---------------------------------------------------------------- RND
def test_rnd_predictor_trains_with_sgd_and_has_no_moments():
    r = nature_runner(["--rnd_opt_optimizer=sgd"], rnd=True)
    assert r.rnd_optimizer.kind == "sgd" and r.policy_optimizer.kind == "adam"
    collect(r)
    rnd = r.rnd
    before, target = rnd.prediction_net.flat.clone(), rnd.target_net.flat.clone()
    seen, original = [], rnd._call

    def call(name, *a):
        seen.append(name)
        return original(name, *a)
    rnd._call = call
    r.train_rnd()
    torch.cuda.synchronize()
    assert set(optimiser_calls(seen)) == {"ppo_sgd_step_f32"}
    assert not torch.equal(rnd.prediction_net.flat, before) and torch.equal(rnd.target_net.flat, target)
    assert bool(torch.isfinite(rnd.prediction_net.flat).all())
    assert rnd.exp_avg is None and rnd.exp_avg_sq is None and rnd.adam_steps == 0
    sd = r.rnd_optimizer.state_dict()
    assert sd == torch_sgd_dict(len(rnd.prediction_net.offsets), args.rnd_opt.lr)


# ---------------------------------------------------------------- checkpoints
def iteration(r):
    r.generate_rollout()
    r.calculate_returns()
    r.train()


def test_checkpoint_round_trip_in_torchs_sgd_layout_and_the_other_kind_is_refused(tmp_path):
    sgd = ["--policy_opt_optimizer=sgd", "--rnd_opt_optimizer=sgd", "--policy_opt_lr=0.003"]
    a = nature_runner(sgd, rnd=True)
    iteration(a)
    torch.cuda.synchronize()
    path = a.save_checkpoint(str(tmp_path / "sgd.pt"), a.step)
    cp = checkpoint.load(path)
    n = len(a.policy_net.parameter_order())
    want = torch_sgd_dict(n, 0.003)
    assert cp["policy_optimizer_state_dict"] == want and cp["value_optimizer_state_dict"] == want
    assert cp["policy_optimizer_state_dict"]["state"] == {}
    assert cp["policy_optimizer_state_dict"]["param_groups"][0]["params"] == list(range(n))
    assert cp["rnd_optimizer_state_dict"] == torch_sgd_dict(len(a.rnd.prediction_net.offsets), args.rnd_opt.lr)
    # torch's own SGD takes the entry
    params = [torch.nn.Parameter(torch.zeros(1)) for _ in range(n)]
    torch.optim.SGD(params, lr=1.0).load_state_dict(cp["policy_optimizer_state_dict"])
    b = nature_runner(sgd, rnd=True, seed=6)
    assert not torch.equal(b.policy_net.flat, a.policy_net.flat)
    b.load_checkpoint(path)
    assert torch.equal(b.policy_net.flat, a.policy_net.flat)
    assert torch.equal(b.rnd.prediction_net.flat, a.rnd.prediction_net.flat)
    assert b.policy_optimizer.state_dict() == want and b.policy_net.exp_avg is None and b.policy_net._adam_step == 0
    # an Adam run refuses the SGD checkpoint, and an SGD run an Adam checkpoint - before and after Adam has stepped
    c = nature_runner(rnd=True, seed=7)
    with pytest.raises(ValueError, match="sgd.*adam"):
        c.load_checkpoint(path)
    fresh_adam = c.save_checkpoint(str(tmp_path / "adam0.pt"), 0)
    iteration(c)
    torch.cuda.synchronize()
    stepped_adam = c.save_checkpoint(str(tmp_path / "adam1.pt"), c.step)
    for p in (fresh_adam, stepped_adam):
        d = nature_runner(sgd, rnd=True, seed=8)
        with pytest.raises(ValueError, match="adam.*sgd"):
            d.load_checkpoint(p)
    # only the kind that differs is refused: an SGD predictor next to an Adam policy checkpoint
    e = nature_runner(["--rnd_opt_optimizer=sgd"], rnd=True, seed=8)
    with pytest.raises(ValueError, match="adam.*sgd"):
        e.rnd_optimizer.load_state_dict(checkpoint.load(stepped_adam)["rnd_optimizer_state_dict"])
    e.policy_optimizer.load_state_dict(checkpoint.load(stepped_adam)["policy_optimizer_state_dict"])
    assert e.policy_net._adam_step == c.policy_net._adam_step > 0


# ---------------------------------------------------------------- beta1 = -1
def test_adam_beta1_auto_reaches_the_launch():
    r = nature_runner(["--policy_opt_adam_beta1=-1", "--policy_opt_mini_batch_size=16", "--policy_opt_epochs=2"])
    want = 1 - 1 / ((8 * 4 / 16) * 2)
    assert args.policy_opt.adam_beta1 == want == 0.75
    assert r.policy_optimizer.state_dict()["param_groups"][0]["betas"] == (want, args.policy_opt.adam_beta2)
    collect(r)
    seen, step = [], r.policy_net.adam_step
    r.policy_net.adam_step = lambda **kw: (seen.append(kw["beta1"]), step(**kw))[1]
    r.train_policy()
    torch.cuda.synchronize()
    assert seen == [want] * 4
    assert r.policy_optimizer.state_dict()["param_groups"][0]["betas"][0] == want
