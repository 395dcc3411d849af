#!/usr/bin/env python3
"""Generate tests/golden/impala_downsample_golden.npz / .json: the REFERENCE's TVFModel(encoder="impala",
encoder_args={'down_sample': m}, single) on CPU for the two modes without a max-pool.

Build container only (needs the reference checkout; see ref_shim.py):  python tests/golden/make_impala_downsample_golden.py

Two sets, each from torch.manual_seed(<seed>) with MKL's LAPACK pinned as in make_init_pinned_golden.py (the heads'
orthogonal initialiser is a QR factorisation), so "params" holds host-independent sha256 hashes of every initial parameter:
  stride  down_sample='stride', default channels (16, 32, 32) and n_block, input (4, 36, 36) (maps 18 -> 9 -> 5),
          hidden 64, 6 actions
  none    down_sample='none', channels (8, 16), n_block 1, input (3, 12, 10), hidden 64, 6 actions (the channel list
          goes to the reference's ImpalaCNN directly, see build)
and per set the forward head outputs of 8 uint8 observations and one policy minibatch of 8 through
Runner.train_policy_minibatch with its result vector and EVERY parameter gradient.
The seed of a set is the first one (from SEED upwards) for which no ReLU pre-activation of the minibatch's forward pass
(every block convolution's input and mid map, the flattened map, the encoder output) lies within 1e-5 of zero; the
margin found is recorded.  These modes have no max-pool, so ReLU is the only kink and a comparison of gradients has no
element to exclude.
"""
import contextlib
import hashlib
import io
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
PINNED = {"MKL_CBWR": "COMPATIBLE", "MKL_NUM_THREADS": "1", "OMP_NUM_THREADS": "1"}
SEED, MB, N_ACTIONS, MARGIN, HIDDEN = 11, 8, 6, 1e-5, 64
MAX_SEEDS = 100000  # (a few hundred thousand pre-activations per pass: most seeds have one inside the margin)
SETS = {
    "stride": {"encoder_args": {"down_sample": "stride"}, "input_dims": (4, 36, 36)},
    "none": {"encoder_args": {"down_sample": "none", "channels": (8, 16), "n_block": 1}, "input_dims": (3, 12, 10)},
}


def build(models, torch, args, seed, input_dims, encoder_args):
    torch.manual_seed(seed)
    real = models.construct_network
    if "channels" in encoder_args:
        # construct_network (rl/models.py:868) puts channels=(16, 32, 32) in front of the encoder arguments, so a channel
        # list cannot reach ImpalaCNN through it; the class itself (rl/models.py:62-69) takes one
        models.construct_network = lambda head_name, dims, **kwargs: models.ImpalaCNN(dims, **kwargs)
    try:
        with contextlib.redirect_stdout(io.StringIO()):  # (the constructor reports its encoder arguments, per seed tried)
            return models.TVFModel(
                encoder="impala", encoder_args=dict(encoder_args), input_dims=input_dims, actions=N_ACTIONS, device="cpu",
                architecture="single", dtype=torch.float32, hidden_units=HIDDEN, encoder_activation_fn="relu",
                head_scale=args.model.head_scale, head_bias=args.model.head_bias, value_head_names=("ext",))
    finally:
        models.construct_network = real


def param_meta(net):
    return {n: {"shape": list(p.shape), "sha256": hashlib.sha256(p.detach().numpy().tobytes()).hexdigest()}
            for n, p in net.named_parameters()}


def relu_margin(torch, model, xs):
    """The forward pass of the minibatch and the smallest |pre-activation| any ReLU of it sees, with their count."""
    enc = model.policy_net.encoder
    pre = []

    def seen(t):
        pre.append(t.detach().abs().min().item())

    hooks = []
    for stack in enc.stacks:
        for block in stack.blocks:
            hooks.append(block.register_forward_pre_hook(lambda _m, i: seen(i[0])))       # conv0 reads relu(block input)
            hooks.append(block.conv0.register_forward_hook(lambda _m, _i, o: seen(o)))     # conv1 reads relu(mid map)
    hooks.append(enc.stacks[-1].register_forward_hook(lambda _m, _i, o: seen(o)))          # the flattened map
    hooks.append(enc.register_forward_hook(lambda _m, _i, o: seen(o)))                     # the encoder output
    with torch.no_grad():
        cur = model.forward(xs, output="policy")
    for h in hooks:
        h.remove()
    return cur, min(pre), len(pre), len(hooks)


def main():
    from ref_shim import load_reference
    load_reference([
        "--model_architecture=single", "--model_encoder=impala", "--env_embed_time=False", "--device=cpu",
        "--env_reward_normalization=off", "--disable_ev=True", "--output_folder=/tmp/ref_golden_out",
        f"--agents={MB}", "--n_steps=4", f"--seed={SEED}", f"--policy_opt_mini_batch_size={MB}"])
    import torch
    from rl import config, logger, models, rollout
    args = config.args
    out, meta = {}, {"n_actions": N_ACTIONS, "head_scale": args.model.head_scale, "head_bias": args.model.head_bias,
                     "ppo_epsilon": args.ppo_epsilon, "entropy_bonus": args.entropy_bonus, "ppo_vf_coef": args.ppo_vf_coef,
                     "hidden_units": HIDDEN, "mkl_env": PINNED}
    for tag, cfg in SETS.items():
        dims = cfg["input_dims"]
        for seed in range(SEED, SEED + MAX_SEEDS):
            model = build(models, torch, args, seed, dims, cfg["encoder_args"])
            rng = np.random.default_rng(seed)
            xs = rng.integers(0, 256, size=(MB, *dims), dtype=np.uint8)
            cur, margin, seen, expected = relu_margin(torch, model, xs)
            if seen == expected and margin >= MARGIN:
                break
        else:
            raise SystemExit(f"{tag}: no seed with the required ReLU margin")
        net = model.policy_net
        meta[tag] = {"seed": seed, "input_dims": list(dims), "hidden_units": HIDDEN, "relu_margin": margin,
                     "relu_maps_checked": seen,
                     "encoder_args": {k: (list(v) if isinstance(v, tuple) else v) for k, v in cfg["encoder_args"].items()},
                     "out_shape": list(net.encoder.out_shape), "params": param_meta(net),
                     "param_names": [n for n, _ in net.named_parameters()]}
        xf = rng.integers(0, 256, size=(MB, *dims), dtype=np.uint8)
        with torch.no_grad():
            r = model.forward(xf, output="policy", policy_temperature=1.0)
        for k in ("raw_policy", "log_policy", "value", "advantage"):
            out[f"{tag}_fwd_{k}"] = r[k].numpy()
        out[f"{tag}_fwd_x"] = xf
        old_logits = cur["raw_policy"] + 0.5 * torch.from_numpy(rng.normal(size=(MB, N_ACTIONS)).astype(np.float32))
        old_lp = torch.log_softmax(old_logits, dim=1)
        actions = torch.from_numpy(rng.integers(0, N_ACTIONS, size=(MB,)).astype(np.int64))
        data = {"prev_state": torch.from_numpy(xs), "actions": actions, "log_policy": old_lp,
                "log_pac": old_lp[range(MB), actions],
                "advantages": torch.from_numpy(rng.normal(size=(MB,)).astype(np.float32)),
                "returns": torch.from_numpy(rng.normal(size=(MB, 1)).astype(np.float32))}
        for k, v in data.items():
            out[f"{tag}_mb_{k}"] = v.numpy()
        runner = rollout.Runner(model, logger.Logger(), action_dist="discrete")
        runner.policy_optimizer.zero_grad(set_to_none=True)
        res = runner.train_policy_minibatch(data, loss_scale=1.0)
        out[f"{tag}_mb_result"] = np.asarray([res["loss"], res["kl_approx"], res["kl_true"], res["clip_frac"]], np.float64)
        meta[tag]["grad_none"] = [n for n, p in net.named_parameters() if p.grad is None]
        for n, p in net.named_parameters():
            if p.grad is not None:
                out[f"{tag}_grad_{n}"] = p.grad.detach().numpy().copy()
        print(f"{tag}: seed {seed} margin {margin:.3e} over {seen} maps, out_shape {meta[tag]['out_shape']}, result",
              out[f"{tag}_mb_result"].tolist())

    path = os.path.join(HERE, "impala_downsample_golden.npz")
    np.savez_compressed(path, **out)
    json.dump(meta, open(os.path.join(HERE, "impala_downsample_golden.json"), "w"), indent=1)
    print("impala_downsample_golden:", len(out), "arrays,", sum(v.nbytes for v in out.values()) / 1e6, "MB raw,",
          os.path.getsize(path), "bytes on disk")


if __name__ == "__main__":
    if os.environ.get("MKL_CBWR") != PINNED["MKL_CBWR"]:
        sys.exit(subprocess.call([sys.executable, os.path.abspath(__file__)], env=dict(os.environ, **PINNED)))
    main()
