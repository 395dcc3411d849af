#!/usr/bin/env python3
"""Generate tests/golden/distil_golden.npz / .json: the REFERENCE's Runner.train_distil_minibatch on CPU under the
distillation switches beyond the default (--distil_loss, --distil_value_loss, --distil_target, --distil_max_heads;
rl/config.py:329-347, rl/rollout.py:1331-1449) - inputs, loss, loss_std and every policy_net gradient of one minibatch.

Build side only (needs the reference checkout ref_shim.py points at):  python tests/golden/make_distil_golden.py

Every combination: MLP encoder / relu / dual architecture / 6 discrete actions / obs (4,) / hidden 64 / minibatch 32.
  logit_l1       --distil_loss=mse_logit  --distil_value_loss=l1
  policy_clipped --distil_loss=mse_policy --distil_value_loss=clipped_mse
  kl_huber       --distil_loss=kl_policy  --distil_value_loss=huber --distil_delta=0.1
  huber0         --distil_value_loss=huber --distil_delta=0
  advantage      --distil_target=advantage   (the advantage head's entry for the action taken)
  return         --distil_target=return      (the same prediction; the batch builder's targets differ)
  tvf_heads3     8 TVF heads, --distil_max_heads=3

The targets are spread so that every zone of every value loss is met (|d| below 0.1, between, above 1).  The initial
policy_net parameters are recorded too (once per network shape): the orthogonal initialiser's last bits depend on the
host, and the gradients belong to exactly these parameters.
"""
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from ref_shim import load_reference  # noqa: E402

MB, DIMS, N_ACTIONS, HIDDEN = 32, (4,), 6, 64
TMP = tempfile.gettempdir()
TVF = ["--tvf_enabled=True", "--tvf_value_heads=8", "--tvf_max_horizon=1000"]
COMBOS = {
    "logit_l1": ["--distil_loss=mse_logit", "--distil_value_loss=l1"],
    "policy_clipped": ["--distil_loss=mse_policy", "--distil_value_loss=clipped_mse"],
    "kl_huber": ["--distil_loss=kl_policy", "--distil_value_loss=huber", "--distil_delta=0.1"],
    "huber0": ["--distil_value_loss=huber", "--distil_delta=0"],
    "advantage": ["--distil_target=advantage"],
    "return": ["--distil_target=return"],
    "tvf_heads3": TVF + ["--distil_max_heads=3"],
}


def run(tag):
    flags = ["--device=cpu", "--env_reward_normalization=off", "--disable_ev=True", f"--output_folder={os.path.join(TMP, 'ref_golden_out')}",
             f"--agents={MB}", "--n_steps=4", "--seed=7", "--model_architecture=dual", "--model_encoder=mlp",
             f"--model_hidden_units={HIDDEN}", f"--policy_opt_mini_batch_size={MB}", f"--value_opt_mini_batch_size={MB}",
             f"--distil_opt_mini_batch_size={MB}", "--env_type=atari", "--distil_beta=0.7"]
    flags += COMBOS[tag]
    if "--tvf_enabled=True" not in flags:
        flags.append("--tvf_enabled=False")
    load_reference(flags)
    import torch
    from rl import config, logger, models, rollout
    import rl.tvf
    args = config.args
    out, m = {}, {"flags": COMBOS[tag]}
    torch.manual_seed(7)
    horizons = weights = None
    if args.tvf.enabled:
        horizons, weights = rl.tvf.get_value_head_horizons(args.tvf.value_heads, args.tvf.max_horizon, args.tvf.head_spacing,
                                                           include_weight=True)
        args.tvf.value_heads = len(horizons)
        out["tvf_horizons"] = np.asarray(horizons)
        out["tvf_weights"] = np.asarray(weights, np.float32)
    model = models.TVFModel(
        encoder="mlp", encoder_args=None, input_dims=DIMS, actions=N_ACTIONS, device="cpu", architecture="dual",
        dtype=torch.float32, hidden_units=HIDDEN, encoder_activation_fn="relu", tvf_fixed_head_horizons=horizons,
        tvf_fixed_head_weights=weights, head_scale=args.model.head_scale, head_bias=args.model.head_bias,
        value_head_names=("ext",))
    m.update(head_scale=args.model.head_scale, head_bias=args.model.head_bias, distil_beta=args.distil.beta,
             distil_loss=args.distil.loss, distil_value_loss=args.distil.value_loss, distil_target=args.distil.target,
             distil_delta=args.distil.delta, distil_l1_scale=args.distil.l1_scale, distil_max_heads=args.distil.max_heads)
    for n, p in model.policy_net.named_parameters():
        out[f"init_{n}"] = p.detach().numpy().copy()
    runner = rollout.Runner(model, logger.Logger(), action_dist="discrete")

    rng = np.random.default_rng(23 + list(COMBOS).index(tag))  # (so that `return` is not `advantage` again)
    x = rng.standard_normal((MB, *DIMS)).astype(np.float32)
    with torch.no_grad():
        cur = model.forward(x, output="policy", exclude_tvf=not args.tvf.enabled)
    actions = rng.integers(0, N_ACTIONS, size=(MB,)).astype(np.int64)
    if args.tvf.enabled:
        pred = cur["tvf_value"][:, :, 0].numpy()
    elif args.distil.target == "value":
        pred = cur["value"][:, 0].numpy()
    else:
        pred = cur["advantage"].numpy()[np.arange(MB), actions]
    # d = prediction - target over the zones of every value loss: a third within +-0.08, a third within +-0.8, the rest
    # out to +-3; none within 1e-3 of a kink (0, 0.1, 1)
    d = rng.uniform(-1, 1, size=pred.shape) * rng.choice([0.08, 0.8, 3.0], size=pred.shape)
    for kink in (0.0, 0.1, 1.0):
        near = np.abs(np.abs(d) - kink) < 1e-3
        d[near] = np.sign(d[near] + 1e-12) * (kink + 2e-3)
    targets = (pred - d).astype(np.float32)
    noise = 0.4 * rng.normal(size=(MB, N_ACTIONS)).astype(np.float32)
    raw = cur["raw_policy"] + torch.from_numpy(noise)
    data = {"prev_state": torch.from_numpy(x), "distil_targets": torch.from_numpy(targets), "old_raw_policy": raw,
            "old_log_policy": torch.log_softmax(raw, dim=1), "distil_actions": torch.from_numpy(actions)}
    for k, v in data.items():
        out[k] = v.numpy()
    runner.distil_optimizer.zero_grad(set_to_none=True)
    for p in model.policy_net.parameters():
        p.grad = None
    res = runner.train_distil_minibatch(data, loss_scale=1.0)
    out["result"] = np.asarray([res["loss"], res["loss_std"]], np.float64)
    m["grad_none"] = []
    for n, p in model.policy_net.named_parameters():
        if p.grad is None:
            m["grad_none"].append(n)
        else:
            out[f"grad_{n}"] = p.grad.detach().numpy().copy()
    part = os.path.join(TMP, f"distil_golden_{tag}.npz")
    np.savez(part, **out)
    json.dump(m, open(part + ".json", "w"))
    print(tag, out["result"].tolist(), "no gradient:", m["grad_none"])


def main():
    if len(sys.argv) > 1:  # the reference's config is a module singleton that is set up once: one process per combination
        return run(sys.argv[1])
    import subprocess
    merged, meta, inits = {}, {"minibatch": MB, "input_dims": list(DIMS), "n_actions": N_ACTIONS, "hidden": HIDDEN}, {}
    for tag in COMBOS:
        subprocess.run([sys.executable, os.path.abspath(__file__), tag], check=True)
        part = os.path.join(TMP, f"distil_golden_{tag}.npz")
        arrays = dict(np.load(part))
        meta[tag] = json.load(open(part + ".json"))
        # the initial parameters: stored once per network shape, the combinations name the set they started from
        init = {k[len("init_"):]: arrays.pop(k) for k in list(arrays) if k.startswith("init_")}
        shape = "tvf" if "tvf_horizons" in arrays else "plain"
        if shape not in inits:
            inits[shape] = init
            merged.update({f"init_{shape}_{k}": v for k, v in init.items()})
        assert all(np.array_equal(init[k], inits[shape][k]) for k in init), f"{tag}: another initial net than {shape}"
        meta[tag]["init"] = shape
        merged.update({f"{tag}_{k}": v for k, v in arrays.items()})
    path = os.path.join(HERE, "distil_golden.npz")
    np.savez_compressed(path, **merged)
    json.dump(meta, open(os.path.join(HERE, "distil_golden.json"), "w"), indent=1)
    print("wrote", len(merged), "arrays;", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
