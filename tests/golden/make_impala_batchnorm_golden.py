#!/usr/bin/env python3
"""Generate tests/golden/impala_batchnorm_golden.npz / .json: the REFERENCE's TVFModel(encoder="impala",
encoder_args={'batch_norm': True, ...}, single) on CPU - bn0 / bn1 = nn.BatchNorm2d in every residual block
(rl/impala.py:63-76).

Build container only (needs the reference checkout; see ref_shim.py):  python tests/golden/make_impala_batchnorm_golden.py

Two sets, each from torch.manual_seed(<seed>) with MKL's LAPACK pinned as in make_init_pinned_golden.py, so "params" holds
host-independent sha256 hashes of every INITIAL parameter (gamma ones, beta zeros):
  pool    default channels (16, 32, 32) and n_block, down_sample 'pool', input (4, 20, 20), hidden 64, 6 actions
  stride  down_sample 'stride', channels (8, 16), n_block 1, input (3, 12, 10), hidden 64, 6 actions (the channel list goes
          to the reference's ImpalaCNN directly, see build)
Then, before anything else is recorded, gamma ~ U(0.5, 1.5) and beta ~ N(0, 0.3) are written into every layer (recorded as
<set>_bn_<name>): with gamma = 1 and beta = 0 a swapped or missing tensor would go unseen.  Per set:
  - the key lists of state_dict() and of named_parameters();
  - three consecutive model.train() forwards of different 8-row uint8 batches (<set>_train<k>_x) with their head outputs and
    every batch-norm buffer after each (<set>_train<k>_buf_<name>);
  - then, after model.eval(), one forward (<set>_fwd_*) and one policy minibatch of 8 through Runner.train_policy_minibatch
    with its result vector and EVERY parameter gradient.
The seed of a set is the first one (from SEED upwards) for which, in the eval-mode forward of the minibatch, no ReLU
pre-activation (every bn0 / bn1 output, the flattened map, the encoder output) lies within 1e-5 of zero and - 'pool' - no
max-pool window's runner-up lies within 1e-5 of its maximum; the margins found are recorded.
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
SEED, MB, N_ACTIONS, MARGIN, HIDDEN, N_TRAIN = 11, 8, 6, 1e-5, 64, 3
MAX_SEEDS = 100000
SETS = {
    "pool": {"encoder_args": {"batch_norm": True}, "input_dims": (4, 20, 20)},
    "stride": {"encoder_args": {"batch_norm": True, "down_sample": "stride", "channels": (8, 16), "n_block": 1},
               "input_dims": (3, 12, 10)},
}
HEADS = ("raw_policy", "log_policy", "value", "advantage")


def build(models, torch, args, seed, input_dims, encoder_args):
    torch.manual_seed(seed)
    real = models.construct_network
    if "channels" in encoder_args:
        # construct_network (rl/models.py:868) puts channels=(16, 32, 32) in front of the encoder arguments, so a channel
        # list cannot reach ImpalaCNN through it; the class itself (rl/models.py:62-69) takes one
        models.construct_network = lambda head_name, dims, **kwargs: models.ImpalaCNN(dims, **kwargs)
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            return models.TVFModel(
                encoder="impala", encoder_args=dict(encoder_args), input_dims=input_dims, actions=N_ACTIONS, device="cpu",
                architecture="single", dtype=torch.float32, hidden_units=HIDDEN, encoder_activation_fn="relu",
                head_scale=args.model.head_scale, head_bias=args.model.head_bias, value_head_names=("ext",))
    finally:
        models.construct_network = real


def param_meta(net):
    return {n: {"shape": list(p.shape), "sha256": hashlib.sha256(p.detach().numpy().tobytes()).hexdigest()}
            for n, p in net.named_parameters()}


def bn_layers(net):
    return [(n, m) for n, m in net.named_modules() if type(m).__name__ == "BatchNorm2d"]


def kink_margins(torch, model, xs, pool):
    """The eval-mode forward of the minibatch, the smallest |pre-activation| any ReLU of it sees and the smallest gap
    between a max-pool window's maximum and its runner-up (inf without a pool), with the number of maps looked at."""
    import torch.nn.functional as F
    enc = model.policy_net.encoder
    pre, gaps = [], []

    def seen(t):
        pre.append(t.detach().abs().min().item())

    def pool_gap(c):
        win = F.unfold(F.pad(c.detach(), (1, 1, 1, 1), value=float("-inf")), 3, stride=2)
        top = win.view(c.shape[0], c.shape[1], 9, -1).topk(2, dim=2).values
        gaps.append((top[:, :, 0] - top[:, :, 1]).min().item())

    hooks = []
    for stack in enc.stacks:
        if pool:
            hooks.append(stack.firstconv.register_forward_hook(lambda _m, _i, o: pool_gap(o)))
        for block in stack.blocks:
            hooks.append(block.bn0.register_forward_hook(lambda _m, _i, o: seen(o)))   # conv0 reads relu(bn0(x))
            hooks.append(block.bn1.register_forward_hook(lambda _m, _i, o: seen(o)))   # conv1 reads relu(bn1(.))
    hooks.append(enc.stacks[-1].register_forward_hook(lambda _m, _i, o: seen(o)))      # the flattened map
    hooks.append(enc.register_forward_hook(lambda _m, _i, o: seen(o)))                 # the encoder output
    with torch.no_grad():
        cur = model.forward(xs, output="policy")
    for h in hooks:
        h.remove()
    return cur, min(pre), min(gaps) if gaps else float("inf"), len(pre) + len(gaps), len(hooks)


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
                     "hidden_units": HIDDEN, "mkl_env": PINNED, "n_train_forwards": N_TRAIN}
    for tag, cfg in SETS.items():
        dims = cfg["input_dims"]
        for seed in range(SEED, SEED + MAX_SEEDS):
            model = build(models, torch, args, seed, dims, cfg["encoder_args"])
            net = model.policy_net
            initial = param_meta(net)
            rng = np.random.default_rng(seed)
            rec = {}
            with torch.no_grad():
                for name, m in bn_layers(net):
                    m.weight.copy_(torch.from_numpy(rng.uniform(0.5, 1.5, m.weight.shape).astype(np.float32)))
                    m.bias.copy_(torch.from_numpy(rng.normal(0, 0.3, m.bias.shape).astype(np.float32)))
                    rec[f"{tag}_bn_{name}.weight"], rec[f"{tag}_bn_{name}.bias"] = m.weight.numpy().copy(), m.bias.numpy().copy()
            model.train()
            for k in range(N_TRAIN):
                xt = rng.integers(0, 256, size=(MB, *dims), dtype=np.uint8)
                with torch.no_grad():
                    r = model.forward(xt, output="policy", policy_temperature=1.0)
                rec[f"{tag}_train{k}_x"] = xt
                for key in HEADS:
                    rec[f"{tag}_train{k}_{key}"] = r[key].numpy().copy()
                for name, m in bn_layers(net):
                    for b in ("running_mean", "running_var", "num_batches_tracked"):
                        rec[f"{tag}_train{k}_buf_{name}.{b}"] = getattr(m, b).numpy().copy()
            model.eval()  # rl/rollout.py:927: everything behind the rollout runs on the running statistics
            xs = rng.integers(0, 256, size=(MB, *dims), dtype=np.uint8)
            cur, margin, gap, seen, expected = kink_margins(torch, model, xs, "down_sample" not in cfg["encoder_args"])
            if seen == expected and margin >= MARGIN and gap >= MARGIN:
                break
        else:
            raise SystemExit(f"{tag}: no seed with the required margins")
        out.update(rec)
        meta[tag] = {"seed": seed, "input_dims": list(dims), "hidden_units": HIDDEN, "relu_margin": margin,
                     "pool_margin": gap if np.isfinite(gap) else None, "maps_checked": seen,
                     "encoder_args": {k: (list(v) if isinstance(v, tuple) else v) for k, v in cfg["encoder_args"].items()},
                     "out_shape": list(net.encoder.out_shape), "params": initial,
                     "param_names": [n for n, _ in net.named_parameters()],
                     "state_dict_keys": list(net.state_dict().keys()),
                     "bn_layers": [n for n, _ in bn_layers(net)]}
        xf = rng.integers(0, 256, size=(MB, *dims), dtype=np.uint8)
        with torch.no_grad():
            r = model.forward(xf, output="policy", policy_temperature=1.0)
        for k in HEADS:
            out[f"{tag}_fwd_{k}"] = r[k].numpy().copy()
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
        model.eval()
        runner.policy_optimizer.zero_grad(set_to_none=True)
        res = runner.train_policy_minibatch(data, loss_scale=1.0)
        assert not model.policy_net.training
        out[f"{tag}_mb_result"] = np.asarray([res["loss"], res["kl_approx"], res["kl_true"], res["clip_frac"]], np.float64)
        meta[tag]["grad_none"] = [n for n, p in net.named_parameters() if p.grad is None]
        for n, p in net.named_parameters():
            if p.grad is not None:
                out[f"{tag}_grad_{n}"] = p.grad.detach().numpy().copy()
        for name, m in bn_layers(net):  # unchanged by eval-mode work
            assert int(m.num_batches_tracked) == N_TRAIN
            assert np.array_equal(m.running_mean.numpy(), out[f"{tag}_train{N_TRAIN - 1}_buf_{name}.running_mean"])
        print(f"{tag}: seed {seed} relu margin {margin:.3e} pool margin {gap:.3e} over {seen} maps, out_shape "
              f"{meta[tag]['out_shape']}, result", out[f"{tag}_mb_result"].tolist())

    path = os.path.join(HERE, "impala_batchnorm_golden.npz")
    np.savez_compressed(path, **out)
    json.dump(meta, open(os.path.join(HERE, "impala_batchnorm_golden.json"), "w"), indent=1)
    print("impala_batchnorm_golden:", len(out), "arrays,", sum(v.nbytes for v in out.values()) / 1e6, "MB raw,",
          os.path.getsize(path), "bytes on disk")


if __name__ == "__main__":
    if os.environ.get("MKL_CBWR") != PINNED["MKL_CBWR"]:
        sys.exit(subprocess.call([sys.executable, os.path.abspath(__file__)], env=dict(os.environ, **PINNED)))
    main()
