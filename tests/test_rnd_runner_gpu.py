"""GPU: Random Network Distillation in the Runner - intrinsic rewards in the rollout, intrinsic returns, the two-head policy
minibatch, the predictor's training phase and the checkpoint entries - against tests/golden/rnd_runner_golden.npz (the
reference on CPU; tests/golden/make_rnd_golden.py --runner) and against itself.

Bars.  (f): the loss and the other results 2e-6, gradients of the dense layers and heads 2e-5 of the tensor's largest entry
(tests/test_variants_gpu.py), gradients of the convolutions 1e-4 (the per-kernel bar of DESIGN.md §2, as in
tests/test_nature_gpu.py).  (g): the host half bit-exact; normalised rewards, int_advantage and int_returns within 1e-6 of
the tensor's largest entry (a float32 scan of 6 steps against the reference's float64 one)."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from ppo_amd import checkpoint, logger, models, rollout  # noqa: E402
from ppo_amd.config import args  # noqa: E402
from ppo_amd.vec_env import SplitVecEnv, SyntheticVecEnv  # noqa: E402

DIMS, N_ACTIONS = (4, 36, 36), 6
FLAGS = ["--model_encoder=nature", "--env_type=synthetic", "--env_embed_time=False", "--env_synthetic_shape=4,36,36",
         "--seed=5", "--rnd_enabled=True", "--observation_normalization=True", "--disable_logging=True", "--device=cuda",
         "--policy_opt_mini_batch_size=16", "--policy_opt_epochs=1", "--value_opt_mini_batch_size=16", "--value_opt_epochs=1",
         "--distil_opt_mini_batch_size=16", "--rnd_opt_mini_batch_size=8"]


@pytest.fixture(scope="module")
def gold(golden_dir):
    return (np.load(os.path.join(golden_dir, "rnd_runner_golden.npz")),
            json.load(open(os.path.join(golden_dir, "rnd_runner_golden.json"))))


def make_model(g, architecture="single", seed=5, frozen=False, use_rnd=True):
    torch.manual_seed(seed)
    model = models.TVFModel(encoder="nature", input_dims=DIMS, actions=N_ACTIONS, device="cuda", architecture=architecture,
                            hidden_units=64, use_rnd=use_rnd, observation_normalization=True, head_scale=0.1, head_bias=True,
                            freeze_observation_normalization=frozen, value_head_names=("ext", "int") if use_rnd else ("ext",))
    model.obs_norm.load_state_dict({"mean": g["f_obs_mean"], "var": g["f_obs_var"], "count": float(g["f_obs_count"])})
    return model


def make_runner(g, agents, n_steps, architecture="single", extra=(), parts=2, model=None, env_seed=3, **kw):
    args.setup([*FLAGS, f"--agents={agents}", f"--n_steps={n_steps}", f"--model_architecture={architecture}", *extra])
    model = model or make_model(g, architecture, **kw)
    r = rollout.Runner(model, logger.Logger(quiet=True))
    per = agents // parts
    envs_ = [SyntheticVecEnv(per, obs_shape=DIMS, n_actions=N_ACTIONS, seed=env_seed, p_done=0.1, env_offset=i * per,
                             threads=2) for i in range(parts)]
    r.vec_env = envs_[0] if parts == 1 else SplitVecEnv(envs_)
    r.reset()
    return r


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def close(got, want, bar, what):
    got, want = (x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x for x in (got, want))
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    err, scale = float(np.abs(got - want).max()), max(float(np.abs(want).max()), 1e-30)
    print(f"RND_RUNNER {what} err/max={err / scale:.3e} bar={bar:.0e}")
    assert err <= bar * scale, f"{what}: max err {err:.3e} vs {bar:.0e} x {scale:.3e}"


# ---------------------------------------------------------------- (f)
def test_policy_minibatch_with_two_value_heads_matches_the_reference(gold):
    g, meta = gold
    r = make_runner(g, 8, 4)
    net = r.policy_net
    assert r.VH == 2 and r.value_heads == ["ext", "int"] and net.vh == 2
    names = [k[len("f_param_"):] for k in g.files if k.startswith("f_param_")]
    net.load_state_dict({n: torch.from_numpy(g["f_param_" + n]) for n in names}, strict=True)
    data = {k: cuda(g["f_" + k]) for k in ("prev_state", "actions", "log_policy", "log_pac", "advantages", "returns")}
    assert tuple(data["returns"].shape) == (8, 2)
    net.grad.zero_()
    res = r.train_policy_minibatch(data, loss_scale=1.0)
    want = g["f_result"]
    for got, w, what in zip((res["loss"], res["kl_approx"], res["kl_true"], res["clip_frac"]), want,
                            ("loss", "kl_approx", "kl_true", "clip_frac")):
        print(f"RND_RUNNER f {what} got={got:.9g} want={w:.9g}")
        assert abs(got - w) <= 2e-6, what
    for n in names:
        if n in meta["f_grad_none"]:
            assert not net.grads[n].any(), n
        else:
            close(net.grads[n], g["f_grad_" + n], 1e-4 if ".conv" in n else 2e-5, "f grad " + n)
    # the value head's two rows both learn: neither head's gradient is zero
    assert net.grads["value_head.weight"].abs().amax(1).min() > 0


# ---------------------------------------------------------------- (g)
@pytest.mark.parametrize("prop,center", [(1, 0), (1, 1), (0, 0), (0, 1)])
def test_intrinsic_returns_match_the_reference(gold, prop, center):
    g, meta = gold
    r = make_runner(g, 5, 6, parts=1, extra=[f"--ir_propagation={bool(prop)}", f"--ir_center={bool(center)}"])
    assert args.gamma_int == meta["gamma_int"] and args.lambda_policy == meta["lambda_policy"]
    assert tuple(r.int_rewards.shape) == (6, 5) and r.ems_norm.dtype == np.float64 and not r.ems_norm.any()
    for k in range(2):
        key = f"g_prop{prop}_center{center}_r{k}_"
        r.int_rewards.copy_(cuda(g["g_int_rewards"][k]))  # unclipped: 7.0 at [0][2, 3]
        r.terminals.copy_(cuda(g["g_terminals"][k]))
        r.value.zero_()
        r.int_value.copy_(cuda(g["g_int_value"][k]))
        adv = r.calculate_intrinsic_returns()
        torch.cuda.synchronize()
        assert r.ems_norm.tobytes() == g[key + "ems_norm"].tobytes()
        rms = r.intrinsic_returns_rms
        assert np.asarray([rms.mean, rms.var, rms.count], np.float64).tobytes() == g[key + "rms"].tobytes()
        assert np.float64(r.intrinsic_reward_norm_scale).tobytes() == g[key + "scale"].tobytes()
        close(r.int_rewards, g[key + "rewards"], 1e-6, key + "rewards")
        close(adv, g[key + "advantage"], 1e-6, key + "advantage")
        close(r.int_returns, g[key + "returns"], 1e-6, key + "returns")
        assert torch.equal(r.int_returns, adv + r.int_value[:6])  # rl/rollout.py:1179
        assert not r.ext_returns.any()
        if k == 0 and not center:  # the planted 7.0 left as 5 / scale
            assert abs(float(r.int_rewards[2, 3]) - 5.0 / float(g[key + "scale"])) <= 1e-6 * float(r.int_rewards.max())
            assert float(r.int_rewards[2, 3]) == float(r.int_rewards.max())


def test_calculate_returns_clips_scales_and_adds_the_intrinsic_advantage(gold):
    g, meta = gold
    r = make_runner(g, 5, 6, parts=1)
    key = "g_prop1_center0_r0_"
    r.int_rewards.copy_(cuda(g["g_int_rewards"][0]))
    r.terminals.copy_(cuda(g["g_terminals"][0]))
    r.value.zero_()
    r.int_value.copy_(cuda(g["g_int_value"][0]))
    r.ext_rewards.copy_(cuda(np.arange(30, dtype=np.float32).reshape(6, 5) / 10))
    r.calculate_returns()
    torch.cuda.synchronize()
    close(r.int_rewards, g[key + "rewards"], 1e-6, "calculate_returns rewards")
    assert abs(float(r.int_rewards[2, 3]) * float(g[key + "scale"]) - 5.0) <= 1e-5  # 7.0 was clipped to 5
    close(r.int_returns, g[key + "returns"], 1e-6, "calculate_returns int_returns")
    # the ext head is what a one-head run computes from column 0 (all-zero values here), the advantage is the sum
    from ppo_amd import returns as R
    ext_adv, ext_ret = R.gae_and_returns(r.ext_rewards, r.ext_value[:6].contiguous(), r.ext_value[6].contiguous(), r.terminals,
                                         args.gamma, args.lambda_policy, args.lambda_value)
    assert torch.equal(r.ext_returns, ext_ret)
    want = ext_adv + (torch.tensor(args.ir.scale, dtype=torch.float32, device="cuda") * r.int_advantage)
    assert torch.equal(r.advantage, want)
    assert tuple(r.returns.shape) == (6, 5, 2) and tuple(r.value.shape) == (7, 5, 2)


# ---------------------------------------------------------------- Runner
def iteration(r):
    r.generate_rollout()
    r.calculate_returns()
    r.train()


def run_single(g, generic, frozen=True):
    np.random.seed(11)
    r = make_runner(g, 8, 4, extra=["--freeze_observation_normalization=True"] if frozen else [], frozen=frozen)
    r.force_generic_rollout = generic
    pred0, target0 = r.rnd.prediction_net.flat.clone(), r.rnd.target_net.flat.clone()
    r.generate_rollout()
    torch.cuda.synchronize()
    raw = r.int_rewards.clone()
    recomputed = torch.stack([r.model.rnd_prediction_error(r.all_obs[t]).clone() for t in range(r.N)])
    r.calculate_returns()
    r.train()
    torch.cuda.synchronize()
    return r, raw, recomputed, pred0, target0


def test_runner_single_architecture_end_to_end(gold):
    g, _meta = gold
    a, raw_a, recomputed, pred0, target0 = run_single(g, generic=False)
    assert raw_a.min() > 0 and len(torch.unique(raw_a)) > 16
    # row t is the prediction error of the observations of step t (normaliser frozen, predictor not yet trained)
    close(raw_a, recomputed, 1e-6, "int_rewards vs recomputed error")
    assert tuple(a.value.shape) == (5, 8, 2) and tuple(a.returns.shape) == (4, 8, 2)
    assert a.int_value.abs().max() > 0 and a.int_returns.abs().max() > 0 and torch.isfinite(a.advantage).all()
    assert not torch.equal(a.rnd.prediction_net.flat, pred0) and torch.equal(a.rnd.target_net.flat, target0)
    assert a.rnd.adam_steps == 1  # round(32 * 0.25) = 8 rows, one minibatch of 8, one epoch
    stats = a.fetch_stats()
    assert np.isfinite([stats[k] for k in ("loss_rnd", "*feat_mean", "*feat_var", "*feat_max", "grad_rnd", "loss_policy")]).all()
    assert stats["loss_rnd"] > 0 and stats["*feat_var"] > 0
    # the generic (one group, gym-API) rollout gives the same bytes, and its rows are the recomputed error exactly
    b, raw_b, recomputed_b, _p, _t = run_single(g, generic=True)
    assert torch.equal(raw_a, raw_b) and torch.equal(a.all_obs, b.all_obs) and torch.equal(a.actions, b.actions)
    assert torch.equal(raw_b, recomputed_b)
    # a second run from the same seed: identical buffers and parameters
    c, raw_c, _r, _p, _t = run_single(g, generic=False)
    for x, y in ((raw_a, raw_c), (a.int_rewards, c.int_rewards), (a.returns, c.returns), (a.value, c.value),
                 (a.advantage, c.advantage), (a.rnd.prediction_net.flat, c.rnd.prediction_net.flat),
                 (a.policy_net.flat, c.policy_net.flat)):
        assert torch.equal(x, y)


def test_runner_dual_architecture_runs(gold):
    g, _meta = gold
    np.random.seed(11)
    r = make_runner(g, 8, 4, architecture="dual")
    before = [n.flat.clone() for n in (r.policy_net, r.value_net, r.rnd.prediction_net)]
    iteration(r)
    torch.cuda.synchronize()
    stats = r.fetch_stats()
    assert np.isfinite([float(v) for v in stats.values()]).all(), stats
    for n, b0 in zip((r.policy_net, r.value_net, r.rnd.prediction_net), before):
        assert torch.isfinite(n.flat).all() and not torch.equal(n.flat, b0)
    assert r.int_rewards.abs().max() > 0 and r.int_value.abs().max() > 0


def test_rnd_refuses_what_is_not_built(gold):
    g, _meta = gold
    args.setup([*FLAGS, "--agents=8", "--n_steps=4", "--model_architecture=single", "--rnd_enabled=False"])
    with pytest.raises(ValueError, match="must agree"):
        rollout.Runner(make_model(g), logger.Logger(quiet=True))


def test_already_normed_input_gives_the_same_error(gold):
    """rl/models.py:716-723: with already_normed the caller's normalised tensor is used as it is, last channel."""
    g, _meta = gold
    model = make_model(g)
    x = cuda(g["f_prev_state"])
    want = model.rnd_prediction_error(x).clone()
    normed = model.perform_normalization(x)
    assert torch.equal(model.rnd_prediction_error(normed, already_normed=True), want)
    assert torch.equal(model.forward(x, include_rnd=True)["rnd_error"], want)


# ---------------------------------------------------------------- checkpoint
def _tree(v):
    """The describe() of tests/golden/make_checkpoint_golden.py, applied to what checkpoint.load returns."""
    if isinstance(v, torch.Tensor):
        return {"__tensor__": str(v.dtype).replace("torch.", ""), "shape": list(v.shape)}
    if isinstance(v, np.ndarray):
        return {"__ndarray__": str(v.dtype), "shape": list(v.shape)}
    if isinstance(v, dict):
        return {"__dict__": {str(k): _tree(x) for k, x in v.items()}, "key_type": sorted({type(k).__name__ for k in v})}
    if isinstance(v, (list, tuple)):
        kinds = [_tree(x) for x in v]
        same = all(k == kinds[0] for k in kinds) if kinds else True
        return {"__seq__": type(v).__name__, "len": len(v), "items": kinds[:1] if same else kinds}
    return {"__scalar__": type(v).__name__}


CORE_GROUP_KEYS = ("lr", "betas", "eps", "weight_decay", "amsgrad", "maximize", "foreach", "capturable", "params")


def test_checkpoint_entries_and_bit_identical_resume(gold, tmp_path):
    g, meta = gold
    np.random.seed(9)
    a = make_runner(g, 8, 4)
    iteration(a)
    path = a.save_checkpoint(str(tmp_path / "checkpoint-000M-params.pt"), a.step)
    cp = checkpoint.load(path)
    ref, got = meta["checkpoint_tree"]["__dict__"], _tree(cp)["__dict__"]
    # the reference's top-level keys (`stats`, `vars`, `discounted_episode_score`: logging accumulators, see test_train_gpu)
    assert set(ref) - set(got) == {"stats", "vars", "discounted_episode_score"}
    assert got["ems_norm"] == ref["ems_norm"] == {"__ndarray__": "float64", "shape": [8]}
    # the reference pickles its RunningMeanStd object; a checkpoint here holds data only: its three float64 moments
    assert ref["intrinsic_returns_rms"] == {"__object__": "rl.utils.RunningMeanStd"}
    assert set(cp["intrinsic_returns_rms"]) == {"mean", "var", "count"}
    gr, wr = got["rnd_optimizer_state_dict"]["__dict__"], ref["rnd_optimizer_state_dict"]["__dict__"]
    assert gr["state"] == wr["state"]  # the same parameter indices with the same tensors
    assert sorted(cp["rnd_optimizer_state_dict"]["state"]) == meta["checkpoint_rnd_state_indices"]
    for key in CORE_GROUP_KEYS:
        assert gr["param_groups"]["items"][0]["__dict__"][key] == wr["param_groups"]["items"][0]["__dict__"][key], key
    rnd_names = [k for k in cp["model_state_dict"] if k.startswith(("prediction_net.", "target_net."))]  # in parameter order
    assert len(rnd_names) == 20
    for k in rnd_names:
        assert got["model_state_dict"]["__dict__"][k] == ref["model_state_dict"]["__dict__"][k], k
    assert sorted(got["model_state_dict"]["__dict__"]) == sorted(ref["model_state_dict"]["__dict__"])
    assert list(cp["model_state_dict"])[-20:] == [f"{net}.{n}" for net, names in (
        ("prediction_net", list(a.rnd.prediction_net.params)), ("target_net", list(a.rnd.target_net.params))) for n in names]
    params = [torch.nn.Parameter(torch.zeros(tuple(cp["model_state_dict"][k].shape))) for k in rnd_names[:12]]
    torch.optim.Adam(params, lr=1.0).load_state_dict(cp["rnd_optimizer_state_dict"])  # torch's own Adam takes it
    # resume: the next rollout's intrinsic rewards and the predictor after train_rnd are those of the uninterrupted run
    iteration(a)
    torch.cuda.synchronize()
    np.random.seed(12345)
    b = make_runner(g, 8, 4, seed=6, env_seed=3)
    assert not torch.equal(b.rnd.prediction_net.flat, a.rnd.prediction_net.flat)
    assert b.load_checkpoint(path) == 32
    iteration(b)
    torch.cuda.synchronize()
    assert torch.equal(a.all_obs, b.all_obs) and torch.equal(a.int_rewards, b.int_rewards) and a.int_rewards.abs().max() > 0
    assert a.ems_norm.tobytes() == b.ems_norm.tobytes()
    assert np.float64(a.intrinsic_returns_rms.var).tobytes() == np.float64(b.intrinsic_returns_rms.var).tobytes()
    assert a.intrinsic_returns_rms.count == b.intrinsic_returns_rms.count
    for x, y in ((a.rnd.prediction_net.flat, b.rnd.prediction_net.flat), (a.rnd.exp_avg, b.rnd.exp_avg),
                 (a.rnd.exp_avg_sq, b.rnd.exp_avg_sq), (a.rnd.target_net.flat, b.rnd.target_net.flat),
                 (a.policy_net.flat, b.policy_net.flat), (a.returns, b.returns)):
        assert torch.equal(x, y)
    assert a.rnd.adam_steps == b.rnd.adam_steps == 2


def test_with_rnd_off_the_checkpoint_has_no_rnd_entries(gold, tmp_path):
    g, _meta = gold
    args.setup([*FLAGS, "--agents=8", "--n_steps=4", "--model_architecture=single", "--rnd_enabled=False"])
    model = make_model(g, use_rnd=False)
    r = rollout.Runner(model, logger.Logger(quiet=True))
    assert r.rnd is None and r.rnd_optimizer is None and not hasattr(r, "int_rewards") and r.value_heads == ["ext"]
    cp = checkpoint.load(r.save_checkpoint(str(tmp_path / "c.pt"), 0))
    assert sorted(cp) == sorted(["step", "ep_count", "batch_counter", "episode_length_buffer", "model_state_dict",
                                 "reward_scale", "episode_score", "world", "sample_calls", "device_seed", "rank_state",
                                 "policy_optimizer_state_dict", "value_optimizer_state_dict",
                                 "distil_optimizer_state_dict", "obs_rms"])
    assert not [k for k in cp["model_state_dict"] if k.startswith(("prediction_net.", "target_net."))]
