#!/usr/bin/env python3
"""Generate tests/golden/nature_golden.npz / .json: the REFERENCE's TVFModel(encoder="nature", single) on CPU.

Build container only (needs the reference checkout; see ref_shim.py):  python tests/golden/make_nature_golden.py

Two sets, both from torch.manual_seed(<seed>) with MKL's LAPACK pinned as in make_init_pinned_golden.py (the orthogonal
initialiser is a QR factorisation), so "params" holds host-independent sha256 hashes of every initial parameter:
  small   input (4, 36, 36) -> 8x8 -> 3x3 -> 1x1, hidden 64, 6 actions: forward head outputs of 8 uint8 observations,
          and one policy minibatch of 8 through Runner.train_policy_minibatch with its loss and EVERY parameter gradient
  full    input (4, 84, 84), hidden 512, 6 actions: initial-parameter hashes and the forward head outputs of 8 uint8
          observations
The seed of the small set is the first one (from SEED upwards) for which no ReLU pre-activation of the minibatch's
forward pass (conv1, conv2, conv3 outputs, the encoder output) lies within 1e-5 of zero; the margin found is recorded,
so a comparison of gradients has no element to exclude.
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
SEED, MB, N_ACTIONS, MARGIN = 11, 8, 6, 1e-5


def build(models, torch, args, seed, input_dims, hidden):
    torch.manual_seed(seed)
    return models.TVFModel(
        encoder="nature", encoder_args=None, input_dims=input_dims, actions=N_ACTIONS, device="cpu",
        architecture="single", dtype=torch.float32, hidden_units=hidden, encoder_activation_fn="relu",
        head_scale=args.model.head_scale, head_bias=args.model.head_bias, value_head_names=("ext",))


def param_meta(net):
    return {n: {"shape": list(p.shape), "sha256": hashlib.sha256(p.detach().numpy().tobytes()).hexdigest()}
            for n, p in net.named_parameters()}


def forward_set(torch, model, x, out, prefix):
    with torch.no_grad():
        r = model.forward(x, output="policy", policy_temperature=1.0)
    for k in ("raw_policy", "log_policy", "value", "advantage"):
        out[f"{prefix}_fwd_{k}"] = r[k].numpy()
    out[f"{prefix}_fwd_x"] = x


def main():
    from ref_shim import load_reference
    load_reference([
        "--model_architecture=single", "--model_encoder=nature", "--env_embed_time=False", "--device=cpu",
        "--env_reward_normalization=off", "--disable_ev=True", "--output_folder=/tmp/ref_golden_out",
        f"--agents={MB}", "--n_steps=4", f"--seed={SEED}", f"--policy_opt_mini_batch_size={MB}"])
    import torch
    from rl import config, logger, models, rollout
    args = config.args
    out, meta = {}, {"n_actions": N_ACTIONS, "head_scale": args.model.head_scale, "head_bias": args.model.head_bias,
                     "ppo_epsilon": args.ppo_epsilon, "entropy_bonus": args.entropy_bonus, "ppo_vf_coef": args.ppo_vf_coef,
                     "mkl_env": PINNED}

    # ---- small: forward + one policy minibatch, seed chosen for its ReLU margins
    dims, hidden = (4, 36, 36), 64
    for seed in range(SEED, SEED + 64):
        model = build(models, torch, args, seed, dims, hidden)
        net = model.policy_net
        rng = np.random.default_rng(seed)
        xs = rng.integers(0, 256, size=(MB, *dims), dtype=np.uint8)
        pre = []
        hooks = [m.register_forward_hook(lambda _m, _i, o: pre.append(o.detach().abs().min().item()))
                 for m in (net.encoder.conv1, net.encoder.conv2, net.encoder.conv3, net.encoder)]
        with torch.no_grad():
            cur = model.forward(xs, output="policy")
        for h in hooks:
            h.remove()
        margin = min(pre)
        if len(pre) == 4 and margin >= MARGIN:
            break
    else:
        raise SystemExit("no seed with the required ReLU margin")
    assert margin >= MARGIN
    meta["small"] = {"seed": seed, "input_dims": list(dims), "hidden_units": hidden, "relu_margin": margin,
                     "params": param_meta(net), "param_names": [n for n, _ in net.named_parameters()]}
    xf = rng.integers(0, 256, size=(MB, *dims), dtype=np.uint8)
    forward_set(torch, model, xf, out, "small")
    old_logits = cur["raw_policy"] + 0.5 * torch.from_numpy(rng.normal(size=(MB, N_ACTIONS)).astype(np.float32))
    old_lp = torch.log_softmax(old_logits, dim=1)
    actions = torch.from_numpy(rng.integers(0, N_ACTIONS, size=(MB,)).astype(np.int64))
    data = {"prev_state": torch.from_numpy(xs), "actions": actions, "log_policy": old_lp,
            "log_pac": old_lp[range(MB), actions], "advantages": torch.from_numpy(rng.normal(size=(MB,)).astype(np.float32)),
            "returns": torch.from_numpy(rng.normal(size=(MB, 1)).astype(np.float32))}
    for k, v in data.items():
        out[f"small_mb_{k}"] = v.numpy()
    runner = rollout.Runner(model, logger.Logger(), action_dist="discrete")
    runner.policy_optimizer.zero_grad(set_to_none=True)
    res = runner.train_policy_minibatch(data, loss_scale=1.0)
    out["small_mb_result"] = np.asarray([res["loss"], res["kl_approx"], res["kl_true"], res["clip_frac"]], np.float64)
    meta["small"]["grad_none"] = [n for n, p in net.named_parameters() if p.grad is None]
    for n, p in net.named_parameters():
        if p.grad is not None:
            out["small_grad_" + n] = p.grad.detach().numpy().copy()

    # ---- full size: initial parameters and forward
    dims, hidden = (4, 84, 84), 512
    model = build(models, torch, args, SEED, dims, hidden)
    meta["full"] = {"seed": SEED, "input_dims": list(dims), "hidden_units": hidden, "params": param_meta(model.policy_net),
                    "param_names": [n for n, _ in model.policy_net.named_parameters()]}
    forward_set(torch, model, np.random.default_rng(SEED).integers(0, 256, size=(MB, *dims), dtype=np.uint8), out, "full")

    np.savez_compressed(os.path.join(HERE, "nature_golden.npz"), **out)
    json.dump(meta, open(os.path.join(HERE, "nature_golden.json"), "w"), indent=1)
    print("nature_golden:", len(out), "arrays,", sum(v.nbytes for v in out.values()) / 1e6, "MB raw; small seed", seed,
          "margin", margin, "result", out["small_mb_result"].tolist())


if __name__ == "__main__":
    if os.environ.get("MKL_CBWR") != PINNED["MKL_CBWR"]:
        sys.exit(subprocess.call([sys.executable, os.path.abspath(__file__)], env=dict(os.environ, **PINNED)))
    main()
