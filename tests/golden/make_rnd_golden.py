#!/usr/bin/env python3
"""Generate tests/golden/rnd_golden.npz / .json: the REFERENCE's Random Network Distillation path on CPU.

Build container only (needs the reference checkout; see ref_shim.py):  python tests/golden/make_rnd_golden.py

TVFModel(encoder="nature", single, input_dims=(4, 36, 36), hidden_units=64, use_rnd=True, observation_normalization=True,
value_head_names=("ext", "int")) under torch.manual_seed(<seed>): the RND networks see (1, 36, 36) -> 8x8 -> 3x3 -> 1x1, a
flat width of 64, the smallest geometry where all three layers exist.  MKL is pinned as in make_nature_golden.py (the
policy net, built first, draws an orthogonal initialisation).  Contents:
  (a) "params": shape and sha256 of every initial parameter of prediction_net and target_net
  (b) obs_mean / obs_var / obs_count: the observation normaliser after 3 updates of 8 uint8 observations each
  (c) fwd_x, fwd_rnd_error: rnd_prediction_error of 8 uint8 observations
  (d) mb_x, mb_loss, mb_feat, grad_<name>: one Runner.train_rnd_minibatch of 8 with its loss, the three feature statistics
      and every predictor gradient ("grad_none" lists the tensors without one: the whole target net)
  (e) step_<name>: the predictor after one Runner.optimizer_step(rnd_optimizer); "opt" holds the optimiser's settings
The seed is the first one (from SEED upwards) for which no leaky-ReLU / ReLU pre-activation of the minibatch's forward
pass (conv1-3 of both nets, fc1 and fc2 of the predictor) lies within 1e-5 of zero; the margin found is recorded, so a
comparison of gradients has no element to exclude.

Parts (f)-(h) go to a second pair of files, rnd_runner_golden.npz / .json (`--runner`; one file of everything would pass
the size limit below), from a Runner of the same model class under --seed=RUNNER_SEED:
  (f) f_<input>, f_param_<name>, f_result, f_grad_<name>: the policy net's parameters, one single-architecture
      Runner.train_policy_minibatch of 8 with returns [8, 2], its result and every gradient
  (g) g_int_rewards [2, 6, 5] (one planted 7.0; clipped to +-5 here as generate_rollout does, rl/rollout.py:929, before the
      reference's calculate_intrinsic_returns sees them), g_terminals, g_int_value [2, 7, 5] and, per case
      <c> in prop{0,1}_center{0,1} and rollout r: g_<c>_r<r>_ems_norm, _rms (mean, var, count), _scale, _rewards (normalised),
      _advantage, _returns; "g_dtypes" records the dtype NumPy gave the normalised rewards (float64 under NumPy >= 2)
  (h) "checkpoint_tree": the key tree of a checkpoint saved with RND on, by the method of make_checkpoint_golden.py

Size: a committed file stays under 1 MiB, and the predictor's two 512 x 512 layers alone are 2 MB per copy.  Tensors of
more than FULL_MAX elements are therefore stored as every `stride`-th row (stride in "row_stride"), together with the
float64 sum and sum of squares of the whole tensor ("whole_<key>"), which pin the rows left out.
"""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
PINNED = {"MKL_CBWR": "COMPATIBLE", "MKL_NUM_THREADS": "1", "OMP_NUM_THREADS": "1"}
SEED, MB, N_ACTIONS, MARGIN = 23, 8, 6, 1e-5
DIMS, HIDDEN = (4, 36, 36), 64
GRAD_FULL_MAX, STEP_FULL_MAX = 40000, 4096


def param_meta(net):
    return {n: {"shape": list(p.shape), "sha256": hashlib.sha256(p.detach().numpy().tobytes()).hexdigest()}
            for n, p in net.named_parameters()}


def store(out, meta, key, a, full_max):
    """The array, or every stride-th row of it plus the float64 sums of the whole."""
    a = np.ascontiguousarray(a)
    stride = 1
    while a[::stride].size > full_max:
        stride *= 2
    out[key] = a[::stride].copy()
    meta["row_stride"][key] = stride
    if stride > 1:
        out["whole_" + key] = np.asarray([a.astype(np.float64).sum(), (a.astype(np.float64) ** 2).sum()])


def main():
    from ref_shim import load_reference
    load_reference([
        "--model_architecture=single", "--model_encoder=nature", "--env_embed_time=False", "--device=cpu",
        "--env_reward_normalization=off", "--disable_ev=True", "--output_folder=/tmp/ref_golden_out",
        "--rnd_enabled=True", "--observation_normalization=True",
        f"--agents={MB}", "--n_steps=4", f"--seed={SEED}", f"--policy_opt_mini_batch_size={MB}"])
    import torch
    from rl import config, logger, models, rollout
    args = config.args
    out, meta = {}, {"n_actions": N_ACTIONS, "input_dims": list(DIMS), "hidden_units": HIDDEN, "mkl_env": PINNED,
                     "head_scale": args.model.head_scale, "head_bias": args.model.head_bias, "row_stride": {}}

    for seed in range(SEED, SEED + 64):
        torch.manual_seed(seed)
        model = models.TVFModel(
            encoder="nature", encoder_args=None, input_dims=DIMS, actions=N_ACTIONS, device="cpu", architecture="single",
            dtype=torch.float32, hidden_units=HIDDEN, encoder_activation_fn="relu", use_rnd=True,
            observation_normalization=True, head_scale=args.model.head_scale, head_bias=args.model.head_bias,
            value_head_names=("ext", "int"))
        initial = {"prediction_net": param_meta(model.prediction_net), "target_net": param_meta(model.target_net)}
        rng = np.random.default_rng(seed)
        for _ in range(3):  # (b)
            x = rng.integers(0, 256, size=(MB, *DIMS), dtype=np.uint8)
            model.perform_normalization(model.prep_for_model(x), update_normalization=True)
        xs = rng.integers(0, 256, size=(MB, *DIMS), dtype=np.uint8)
        pre = []
        p, t = model.prediction_net, model.target_net
        watched = (p.conv1, p.conv2, p.conv3, p.fc1, p.fc2, t.conv1, t.conv2, t.conv3)
        hooks = [m.register_forward_hook(lambda _m, _i, o: pre.append(o.detach().abs().min().item())) for m in watched]
        with torch.no_grad():
            model.rnd_prediction_error(xs)
        for h in hooks:
            h.remove()
        margin = min(pre)
        if len(pre) == len(watched) and margin >= MARGIN:
            break
    else:
        raise SystemExit("no seed with the required activation margin")
    meta.update(seed=seed, margin=margin, params=initial,
                param_names={k: list(v) for k, v in initial.items()})
    out["obs_mean"], out["obs_var"] = model.obs_rms.mean.copy(), model.obs_rms.var.copy()
    out["obs_count"] = np.asarray(float(model.obs_rms.count))

    xf = rng.integers(0, 256, size=(MB, *DIMS), dtype=np.uint8)  # (c)
    with torch.no_grad():
        out["fwd_rnd_error"] = model.rnd_prediction_error(xf).numpy()
    out["fwd_x"] = xf

    runner = rollout.Runner(model, logger.Logger(), action_dist="discrete")  # (d)
    runner.rnd_optimizer.zero_grad(set_to_none=True)
    with torch.no_grad():
        out["mb_loss"] = np.asarray(float(model.rnd_prediction_error(xs).mean()), np.float64)
    runner.train_rnd_minibatch({"prev_state": torch.from_numpy(xs)}, loss_scale=1.0)
    out["mb_x"] = xs
    out["mb_feat"] = np.asarray([model.rnd_features_mean, model.rnd_features_var, model.rnd_features_max], np.float64)
    meta["grad_none"] = [f"{net}.{n}" for net in ("prediction_net", "target_net")
                         for n, q in getattr(model, net).named_parameters() if q.grad is None]
    for n, q in p.named_parameters():
        store(out, meta, "grad_" + n, q.grad.detach().numpy(), GRAD_FULL_MAX)

    group = runner.rnd_optimizer.param_groups[0]  # (e)
    meta["opt"] = {"lr": group["lr"], "betas": list(group["betas"]), "eps": group["eps"],
                   "max_grad_norm": args.max_grad_norm, "grad_clip_mode": args.grad_clip_mode}
    out["step_grad_norm"] = np.asarray(runner.optimizer_step(runner.rnd_optimizer, "rnd"), np.float64)
    for n, q in p.named_parameters():
        store(out, meta, "step_" + n, q.detach().numpy(), STEP_FULL_MAX)

    np.savez_compressed(os.path.join(HERE, "rnd_golden.npz"), **out)
    json.dump(meta, open(os.path.join(HERE, "rnd_golden.json"), "w"), indent=1)
    print("rnd_golden:", len(out), "arrays,", sum(v.nbytes for v in out.values()) / 1e6, "MB raw; seed", seed, "margin", margin,
          "loss", float(out["mb_loss"]), "grad norm", float(out["step_grad_norm"]), "feat", out["mb_feat"].tolist())


RUNNER_SEED, G_N, G_A = 5, 6, 5
G_CASES = [(prop, center) for prop in (1, 0) for center in (0, 1)]


def runner_flags(extra=()):
    return ["--model_architecture=single", "--model_encoder=nature", "--env_embed_time=False", "--device=cpu",
            "--env_reward_normalization=off", "--disable_ev=True", "--output_folder=/tmp/ref_golden_out",
            "--rnd_enabled=True", "--observation_normalization=True", "--checkpoint_compression=False",
            f"--seed={RUNNER_SEED}", *extra]


def make_runner(agents, n_steps, extra=()):
    from ref_shim import load_reference
    load_reference(runner_flags([f"--agents={agents}", f"--n_steps={n_steps}", f"--policy_opt_mini_batch_size={MB}",
                                 f"--rnd_opt_mini_batch_size={MB}", *extra]))
    import torch
    from rl import config, logger, models, rollout
    args = config.args
    torch.manual_seed(RUNNER_SEED)
    model = models.TVFModel(
        encoder="nature", encoder_args=None, input_dims=DIMS, actions=N_ACTIONS, device="cpu", architecture="single",
        dtype=torch.float32, hidden_units=HIDDEN, encoder_activation_fn="relu", use_rnd=True,
        observation_normalization=True, head_scale=args.model.head_scale, head_bias=args.model.head_bias,
        value_head_names=("ext", "int"))
    return model, rollout.Runner(model, logger.Logger(), action_dist="discrete"), args


def policy_case(out, meta):
    """(f) and (h)."""
    import torch
    from make_checkpoint_golden import describe
    model, runner, args = make_runner(MB, 4)
    rng = np.random.default_rng(RUNNER_SEED)
    for _ in range(3):
        model.perform_normalization(model.prep_for_model(rng.integers(0, 256, size=(MB, *DIMS), dtype=np.uint8)),
                                    update_normalization=True)
    out["f_obs_mean"], out["f_obs_var"] = model.obs_rms.mean.copy(), model.obs_rms.var.copy()
    out["f_obs_count"] = np.asarray(float(model.obs_rms.count))
    x = torch.from_numpy(rng.integers(0, 256, size=(MB, *DIMS), dtype=np.uint8))
    with torch.no_grad():
        cur = model.forward(x, output="policy")
    lp = torch.log_softmax(cur["raw_policy"], dim=1)
    actions = torch.from_numpy(rng.integers(0, N_ACTIONS, size=(MB,)).astype(np.int64))
    data = {"prev_state": x, "actions": actions, "log_policy": lp, "log_pac": lp[range(MB), actions] + torch.from_numpy(
                rng.normal(scale=0.1, size=(MB,)).astype(np.float32)),
            "advantages": torch.from_numpy(rng.normal(size=(MB,)).astype(np.float32)),
            "returns": torch.from_numpy(rng.normal(size=(MB, 2)).astype(np.float32))}
    for n, q in model.policy_net.named_parameters():
        out["f_param_" + n] = q.detach().numpy().copy()
    runner.policy_optimizer.zero_grad(set_to_none=True)
    res = runner.train_policy_minibatch(data, loss_scale=1.0)
    for k, v in data.items():
        out["f_" + k] = v.detach().numpy()
    out["f_result"] = np.asarray([res["loss"], res["kl_approx"], res["kl_true"], res["clip_frac"]], np.float64)
    meta["f_grad_none"] = [n for n, q in model.policy_net.named_parameters() if q.grad is None]
    for n, q in model.policy_net.named_parameters():
        if q.grad is not None:
            out["f_grad_" + n] = q.grad.detach().numpy().copy()
    meta.update(ppo_epsilon=args.ppo_epsilon, entropy_bonus=args.entropy_bonus, ppo_vf_coef=args.ppo_vf_coef)
    # (h): every optimiser holds state, the intrinsic-return statistics have seen one rollout
    runner.optimizer_step(runner.policy_optimizer, "policy")
    runner.rnd_optimizer.zero_grad(set_to_none=True)
    runner.train_rnd_minibatch({"prev_state": x}, loss_scale=1.0)
    runner.optimizer_step(runner.rnd_optimizer, "rnd")
    runner.int_rewards = rng.random(runner.int_rewards.shape).astype(np.float32)
    runner.calculate_intrinsic_returns()
    captured = {}
    real_save = torch.save
    torch.save = lambda obj, f, **kw: captured.update(obj)
    try:
        runner.save_checkpoint("/tmp/ref_golden_out_ckpt_rnd.pt", 12345, disable_log=True, disable_env_state=True)
    finally:
        torch.save = real_save
    meta["checkpoint_tree"] = describe(captured)
    meta["checkpoint_rnd_state_indices"] = sorted(int(i) for i in captured["rnd_optimizer_state_dict"]["state"])


def returns_case(out, meta, prop, center):
    """(g) for one setting, two consecutive rollouts."""
    tag = f"prop{prop}_center{center}"
    _model, runner, args = make_runner(G_A, G_N, [f"--ir_propagation={bool(prop)}", f"--ir_center={bool(center)}"])
    rng = np.random.default_rng(RUNNER_SEED + 1)  # the same script for every case
    rewards = (rng.random((2, G_N, G_A)) * 3).astype(np.float32)
    rewards[0, 2, 3] = 7.0
    terminals = rng.random((2, G_N, G_A)) < 0.25
    int_value = rng.normal(size=(2, G_N + 1, G_A)).astype(np.float32)
    out["g_int_rewards"], out["g_terminals"], out["g_int_value"] = rewards, terminals, int_value
    meta.update(gamma_int=args.gamma_int, lambda_policy=args.lambda_policy)
    for r in range(2):
        runner.int_rewards = np.clip(rewards[r], -5, 5)
        runner.terminals[:] = terminals[r]
        runner.value[:, :, runner.value_heads.index("int")] = int_value[r]
        adv = runner.calculate_intrinsic_returns()
        key = f"g_{tag}_r{r}_"
        out[key + "ems_norm"] = np.asarray(runner.ems_norm, np.float64).copy()
        rms = runner.intrinsic_returns_rms
        out[key + "rms"] = np.asarray([rms.mean, rms.var, rms.count], np.float64)
        out[key + "scale"] = np.asarray(runner.intrinsic_reward_norm_scale, np.float64)
        meta.setdefault("g_dtypes", {})[key + "rewards"] = str(np.asarray(runner.int_rewards).dtype)
        out[key + "rewards"] = np.asarray(runner.int_rewards, np.float64)
        out[key + "advantage"] = np.asarray(adv, np.float64)
        out[key + "returns"] = np.asarray(runner.int_returns, np.float64).copy()


def main_runner(case):
    """One reference process per case (rl.config.args is a process-wide singleton); results travel through /tmp."""
    if case is None:
        out, meta = {}, {"seed": RUNNER_SEED, "n_actions": N_ACTIONS, "input_dims": list(DIMS), "hidden_units": HIDDEN,
                         "numpy": np.__version__}
        for c in ["policy"] + [f"{p}{c}" for p, c in G_CASES]:
            subprocess.run([sys.executable, os.path.abspath(__file__), "--runner", c], check=True)
            part = np.load(f"/tmp/rnd_runner_{c}.npz")
            out.update({k: part[k] for k in part.files})
            m = json.load(open(f"/tmp/rnd_runner_{c}.json"))
            meta.setdefault("g_dtypes", {}).update(m.pop("g_dtypes", {}))
            meta.update(m)
        np.savez_compressed(os.path.join(HERE, "rnd_runner_golden.npz"), **out)
        json.dump(meta, open(os.path.join(HERE, "rnd_runner_golden.json"), "w"), indent=1, sort_keys=True)
        print("rnd_runner_golden:", len(out), "arrays,", sum(v.nbytes for v in out.values()) / 1e6, "MB raw")
        return
    out, meta = {}, {}
    if case == "policy":
        policy_case(out, meta)
    else:
        returns_case(out, meta, int(case[0]), int(case[1]))
    np.savez(f"/tmp/rnd_runner_{case}.npz", **out)
    json.dump(meta, open(f"/tmp/rnd_runner_{case}.json", "w"))


if __name__ == "__main__":
    if os.environ.get("MKL_CBWR") != PINNED["MKL_CBWR"]:
        sys.exit(subprocess.call([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=dict(os.environ, **PINNED)))
    if len(sys.argv) > 1 and sys.argv[1] == "--runner":
        main_runner(sys.argv[2] if len(sys.argv) > 2 else None)
    else:
        main()
