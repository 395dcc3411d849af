#!/usr/bin/env python3
"""Generate tests/golden/rtg_golden.npz / .json: the REFERENCE's TVFModel(encoder="rtg", single) on CPU.

Build container only (needs the reference checkout; see ref_shim.py):  python tests/golden/make_rtg_golden.py

The RTG encoder (rl/models.py:172-213) keeps torch's default initialisation, so no LAPACK is involved; MKL is pinned all
the same, as in make_nature_golden.py, and "params" holds sha256 hashes of every initial parameter.  Sets, each from
torch.manual_seed(<seed>), then the model, then np.random.default_rng(<seed>) with the minibatch's observations as its
first draw:
  small    input (4, 36, 46) -> h 17, 8, 8, 4, 4, 2; w 22, 11, 11, 5, 5, 2 (an odd height at pool 1, odd widths at pools
           2 and 3), hidden 64, 6 actions: forward head outputs of 8 uint8 observations, and one policy minibatch of 8
           through Runner.train_policy_minibatch with its loss, KL figures and EVERY parameter gradient
  full     input (4, 84, 84), hidden 512, 6 actions: initial-parameter hashes and the forward head outputs of 8 uint8
           observations
  full_b2  input (4, 84, 84), hidden 512, minibatch 2: the seed and margin only (tests/test_rtg_gpu.py builds a float64
           network from that seed)
This network has two kinds of kink, ReLU zeros and pool ties.  The seed of `small` and of `full_b2` is the first one
(from SEED upwards) whose minibatch has a margin of at least 1e-5, the margin being the smallest of: the distance of every
pooled value from zero; the gap between the maximum and the runner-up of every window whose pooled value is positive (a
closed window passes no gradient); the distance of every encoder output from zero.  The margin found is recorded, so a
comparison of gradients has no element to exclude.  (At (4, 84, 84) no seed of 64 comes near that with a minibatch of 8
- typical minima are 2e-7 - hence the minibatch of 2.)
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
        encoder="rtg", encoder_args=None, input_dims=input_dims, actions=N_ACTIONS, device="cpu",
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


def pool_margin(y):
    """Of one pre-pool map [B, C, H, W]: min(|pooled value|, maximum - runner-up over the windows pooled > 0)."""
    b, c, h, w = y.shape
    ho, wo = h // 2, w // 2
    win = y[:, :, :2 * ho, :2 * wo].reshape(b, c, ho, 2, wo, 2).permute(0, 1, 2, 4, 3, 5).reshape(b, c, ho, wo, 4)
    top = win.sort(dim=-1, descending=True).values
    pooled, gap = top[..., 0], top[..., 0] - top[..., 1]
    m = pooled.abs().min().item()
    if (pooled > 0).any():
        m = min(m, gap[pooled > 0].min().item())
    return m


def kink_margin(torch, model, xs):
    """(margin, the forward's result) of the minibatch xs on the reference model."""
    net = model.policy_net
    seen = []
    hooks = [m.register_forward_hook(lambda _m, _i, o: seen.append(pool_margin(o.detach())))
             for m in (net.encoder.conv1, net.encoder.conv2, net.encoder.conv3)]
    hooks.append(net.encoder.register_forward_hook(lambda _m, _i, o: seen.append(o.detach().abs().min().item())))
    with torch.no_grad():
        cur = model.forward(xs, output="policy")
    for h in hooks:
        h.remove()
    assert len(seen) == 4
    return min(seen), cur


def search(models, torch, args, dims, hidden, mb):
    for seed in range(SEED, SEED + 64):
        model = build(models, torch, args, seed, dims, hidden)
        rng = np.random.default_rng(seed)
        xs = rng.integers(0, 256, size=(mb, *dims), dtype=np.uint8)
        margin, cur = kink_margin(torch, model, xs)
        if margin >= MARGIN:
            return seed, margin, model, rng, xs, cur
    raise SystemExit(f"no seed with the required margin at {dims}, minibatch {mb}")


def main():
    from ref_shim import load_reference
    load_reference([
        "--model_architecture=single", "--model_encoder=rtg", "--env_embed_time=False", "--device=cpu",
        "--env_reward_normalization=off", "--disable_ev=True", "--output_folder=/tmp/ref_golden_out",
        f"--agents={MB}", "--n_steps=4", f"--seed={SEED}", f"--policy_opt_mini_batch_size={MB}"])
    import torch
    from rl import config, logger, models, rollout
    args = config.args
    out, meta = {}, {"n_actions": N_ACTIONS, "head_scale": args.model.head_scale, "head_bias": args.model.head_bias,
                     "ppo_epsilon": args.ppo_epsilon, "entropy_bonus": args.entropy_bonus, "ppo_vf_coef": args.ppo_vf_coef,
                     "mkl_env": PINNED}

    # ---- small: forward + one policy minibatch, seed chosen for its margins
    dims, hidden = (4, 36, 46), 64
    seed, margin, model, rng, xs, cur = search(models, torch, args, dims, hidden, MB)
    net = model.policy_net
    meta["small"] = {"seed": seed, "input_dims": list(dims), "hidden_units": hidden, "kink_margin": margin,
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

    # ---- full size, minibatch 2: the seed whose gradients a float64 network can be compared with
    seed2, margin2, *_r = search(models, torch, args, dims, hidden, 2)
    meta["full_b2"] = {"seed": seed2, "input_dims": list(dims), "hidden_units": hidden, "minibatch": 2, "kink_margin": margin2}

    np.savez_compressed(os.path.join(HERE, "rtg_golden.npz"), **out)
    json.dump(meta, open(os.path.join(HERE, "rtg_golden.json"), "w"), indent=1)
    print("rtg_golden:", len(out), "arrays,", sum(v.nbytes for v in out.values()) / 1e6, "MB raw; small seed", seed,
          "margin", margin, "full_b2 seed", seed2, "margin", margin2, "result", out["small_mb_result"].tolist())


if __name__ == "__main__":
    if os.environ.get("MKL_CBWR") != PINNED["MKL_CBWR"]:
        sys.exit(subprocess.call([sys.executable, os.path.abspath(__file__)], env=dict(os.environ, **PINNED)))
    main()
