#!/usr/bin/env python3
"""Generate tests/golden/policy_reg_golden.npz / .json: the REFERENCE's Runner.train_policy_minibatch on CPU with the
global KL penalty (--gkl_*, rl/config.py:378-394, rl/rollout.py:1723-1738) and with SIDE, state-independent exploration
(--side_*, rl/config.py:479-492, rl/rollout.py:1662-1679) - inputs, loss, global_kl and every gradient of one minibatch.

Build side only (needs the reference checkout ref_shim.py points at):  python tests/golden/make_policy_reg_golden.py

Every combination: MLP encoder / relu / single architecture (the value head trains in the same pass) / 6 discrete actions /
obs (4,) / hidden 64 / minibatch 32 / 16 global states / --entropy_bonus=0.1.
  gkl   --gkl_enabled=True --gkl_penalty=0.3
  side  --side_enabled=True
  both  the two together

The old policies - of the minibatch and of the global states - are the net's own with logits tilted by -2 .. 2 over the
actions plus noise: with old = new the KL and its gradient are zero and the fixture would pin nothing.  The SIDE target
is log_softmax of a standard normal draw (a target far from uniform, so that its term is not the entropy bonus again).
The initial parameters are recorded too: the orthogonal initialiser's last bits depend on the host, and the gradients
belong to exactly these parameters.
"""
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from ref_shim import load_reference  # noqa: E402

MB, S, DIMS, N_ACTIONS, HIDDEN = 32, 16, (4,), 6, 64
TMP = tempfile.gettempdir()
GKL = ["--gkl_enabled=True", "--gkl_penalty=0.3", f"--gkl_samples={S}"]
SIDE = ["--side_enabled=True"]
COMBOS = {"gkl": GKL, "side": SIDE, "both": GKL + SIDE}
COMMON = ["--entropy_bonus=0.1"]


def run(tag):
    flags = ["--device=cpu", "--env_reward_normalization=off", "--disable_ev=True", f"--output_folder={os.path.join(TMP, 'ref_golden_out')}",
             f"--agents={MB}", "--n_steps=4", "--seed=7", "--model_architecture=single", "--model_encoder=mlp",
             f"--model_hidden_units={HIDDEN}", f"--policy_opt_mini_batch_size={MB}", "--env_type=atari", "--tvf_enabled=False"]
    flags += COMMON + COMBOS[tag]
    load_reference(flags)
    import torch
    from rl import config, logger, models, rollout
    args = config.args
    out, m = {}, {"flags": COMMON + COMBOS[tag]}
    torch.manual_seed(7)
    model = models.TVFModel(
        encoder="mlp", encoder_args=None, input_dims=DIMS, actions=N_ACTIONS, device="cpu", architecture="single",
        dtype=torch.float32, hidden_units=HIDDEN, encoder_activation_fn="relu", tvf_fixed_head_horizons=None,
        tvf_fixed_head_weights=None, head_scale=args.model.head_scale, head_bias=args.model.head_bias,
        value_head_names=("ext",))
    m.update(head_scale=args.model.head_scale, head_bias=args.model.head_bias, entropy_bonus=args.entropy_bonus,
             ppo_epsilon=args.ppo_epsilon, ppo_vf_coef=args.ppo_vf_coef, gkl_enabled=bool(args.gkl.enabled),
             gkl_penalty=args.gkl.penalty, side_enabled=bool(args.side.enabled))
    for n, p in model.policy_net.named_parameters():
        out[f"init_{n}"] = p.detach().numpy().copy()
    runner = rollout.Runner(model, logger.Logger(), action_dist="discrete")

    rng = np.random.default_rng(41)  # the same inputs for every combination
    x = rng.standard_normal((MB, *DIMS)).astype(np.float32)
    gx = rng.standard_normal((S, *DIMS)).astype(np.float32)
    with torch.no_grad():
        cur = model.forward(x, output="policy")
        gcur = model.forward(gx, output="policy")
    actions = rng.integers(0, N_ACTIONS, size=(MB,)).astype(np.int64)
    # (make_inputs of tests/test_distil_modes_gpu.py: the new logits tilted by -2 .. 2 over the actions, plus noise)
    tilt = np.linspace(-2.0, 2.0, N_ACTIONS)

    def tilted(raw, n):
        return torch.log_softmax(raw + torch.from_numpy((tilt + 0.3 * rng.normal(size=(n, N_ACTIONS))).astype(np.float32)), dim=1)
    old_lp, gold_lp = tilted(cur["raw_policy"], MB), tilted(gcur["raw_policy"], S)
    adv = rng.standard_normal(MB).astype(np.float32)
    returns = (cur["value"].numpy() + rng.uniform(-1, 1, size=(MB, 1))).astype(np.float32)
    target = torch.log_softmax(torch.from_numpy(rng.standard_normal(N_ACTIONS).astype(np.float32)), dim=0)
    data = {"prev_state": torch.from_numpy(x), "actions": torch.from_numpy(actions), "log_policy": old_lp,
            "log_pac": old_lp[torch.arange(MB), torch.from_numpy(actions)].clone(), "advantages": torch.from_numpy(adv),
            "returns": torch.from_numpy(returns), "*global_states": torch.from_numpy(gx), "*global_log_policy": gold_lp}
    for k, v in data.items():
        out[k.lstrip("*")] = v.numpy()
    out["side_target_logp"] = target.numpy()
    runner.side_target_policy_logp = target
    for p in model.policy_net.parameters():
        p.grad = None
    res = runner.train_policy_minibatch(data, loss_scale=1.0)
    out["result"] = np.asarray([res["loss"], float(res["global_kl"]) if "global_kl" in res else np.nan], np.float64)
    m["grad_none"] = []
    for n, p in model.policy_net.named_parameters():
        if p.grad is None:
            m["grad_none"].append(n)
        else:
            out[f"grad_{n}"] = p.grad.detach().numpy().copy()
    part = os.path.join(TMP, f"policy_reg_golden_{tag}.npz")
    np.savez(part, **out)
    json.dump(m, open(part + ".json", "w"))
    print(tag, out["result"].tolist(), "no gradient:", m["grad_none"])


def main():
    if len(sys.argv) > 1:  # the reference's config is a module singleton that is set up once: one process per combination
        return run(sys.argv[1])
    import subprocess
    merged, meta, first = {}, {"minibatch": MB, "global_states": S, "input_dims": list(DIMS), "n_actions": N_ACTIONS,
                               "hidden": HIDDEN}, None
    shared = ("prev_state", "actions", "log_policy", "log_pac", "advantages", "returns", "global_states", "global_log_policy",
              "side_target_logp")
    for tag in COMBOS:
        subprocess.run([sys.executable, os.path.abspath(__file__), tag], check=True)
        part = os.path.join(TMP, f"policy_reg_golden_{tag}.npz")
        arrays = dict(np.load(part))
        meta[tag] = json.load(open(part + ".json"))
        # the initial parameters and the inputs are the same for every combination: stored once
        common = {k: arrays.pop(k) for k in list(arrays) if k.startswith("init_") or k in shared}
        if first is None:
            first = common
            merged.update(common)
        assert all(np.array_equal(common[k], first[k]) for k in common), f"{tag}: other inputs than the first combination"
        merged.update({f"{tag}_{k}": v for k, v in arrays.items()})
    path = os.path.join(HERE, "policy_reg_golden.npz")
    np.savez_compressed(path, **merged)
    json.dump(meta, open(os.path.join(HERE, "policy_reg_golden.json"), "w"), indent=1)
    print("wrote", len(merged), "arrays;", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
