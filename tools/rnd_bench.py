#!/usr/bin/env python3
"""Time the RND launches at the sizes a run uses (MI355X; the table of profiles/rnd.md).

    python tools/rnd_bench.py [--steps 200] [--warmup 20] [--out FILE.json]

One process, HIP events on the current stream, the variants of a row interleaved step by step:
  rollout   RNDNets.prediction_error of a 128-image group of 4x84x84 uint8 observations (what RND adds to one env step
            of one group) next to the policy step it would follow: TVFModel(nature, single, observation normalisation)
            .forward of the same group, RND off
  train     one RND minibatch of 256 rows read through an index out of a 1024-row batch (RNDNets.train_minibatch with the
            statistics row) and its optimiser step
  --runner  the same in place: Runner.generate_rollout of 256 synthetic envs (two pipelined groups of 128) x 32 steps, RND on
            and off alternating rollout by rollout in one process, HIP events on the main stream around each rollout;
            reported per env step (a rollout's time / 33 policy steps); and Runner.train_rnd's minibatches
Launch counts are the entry-point calls of one invocation (ppo_gemm_f32 with a split-K workspace and the weight-gradient
entry points are two kernels each)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ppo_amd import _lib, models  # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3  # us


def summary(v):
    v = np.asarray(v)
    return {"median_us": float(np.median(v)), "p10_us": float(np.percentile(v, 10)), "p90_us": float(np.percentile(v, 90)),
            "n": int(v.size)}


def count_calls(rnd, fn):
    calls, orig = [], rnd._call
    rnd._call = lambda name, *a: (calls.append(name), orig(name, *a))[1]
    try:
        fn()
    finally:
        rnd._call = orig
    return calls


def runner_rows(rollouts, warmup):
    """Per-env-step time of a pipelined rollout with RND on and off, and the launches RND adds to a group's step."""
    from ppo_amd import envs, logger, rollout
    from ppo_amd.config import args as cfg
    N, A = 32, 256
    flags = ["--model_encoder=nature", "--model_architecture=single", "--env_type=synthetic", "--env_embed_time=False",
             "--seed=1", "--observation_normalization=True", "--disable_logging=True", "--device=cuda", f"--agents={A}",
             f"--n_steps={N}", "--env_warmup_period=5"]
    runners = {}
    for key, on in (("off", False), ("on", True)):
        cfg.setup(flags + [f"--rnd_enabled={on}"])
        torch.manual_seed(1)
        shape, n_actions = envs.get_env_spec()
        model = models.TVFModel(encoder="nature", input_dims=shape, actions=n_actions, device="cuda", architecture="single",
                                hidden_units=512, use_rnd=on, observation_normalization=True, head_scale=0.1, head_bias=True,
                                value_head_names=("ext", "int") if on else ("ext",))
        r = rollout.Runner(model, logger.Logger(quiet=True))
        r.vec_env = envs.create_envs_classic()
        r.reset()
        runners[key] = r
    groups = len(getattr(runners["on"].vec_env, "parts", [None]))
    times = {"on": [], "off": []}
    for k in range(warmup + rollouts):
        for key, r in runners.items():
            t = timed(r.generate_rollout) / (N + 1)
            if k >= warmup:
                times[key].append(t)
    on = runners["on"]
    calls = count_calls(on.rnd, lambda: on._policy_step(0, 0, A // groups, tag="i0" if groups > 1 else "i"))
    res = {"rollout_env_step_rnd_on": summary(times["on"]), "rollout_env_step_rnd_off": summary(times["off"]),
           "groups": groups, "group_size": A // groups, "steps_per_rollout": N,
           "rnd_entry_point_calls_per_group_step": len(calls)}
    res["rnd_added_us_per_env_step"] = res["rollout_env_step_rnd_on"]["median_us"] - res["rollout_env_step_rnd_off"]["median_us"]
    res["rnd_added_fraction_of_step_off"] = res["rnd_added_us_per_env_step"] / res["rollout_env_step_rnd_off"]["median_us"]
    on.calculate_returns()
    per_mb = []
    for _ in range(6):  # 8192 * 0.25 / 256 = 8 minibatches per call
        per_mb.append(timed(on.train_rnd) / 8)
    res["train_rnd_per_minibatch_256"] = summary(per_mb[1:])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--runner", action="store_true", help="time RND inside Runner.generate_rollout / train_rnd instead")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    _lib.require_gpu()
    if args.runner:
        res = runner_rows(max(args.steps // 33, 4), 2)
        res["device"] = torch.cuda.get_device_name(0)
        line = json.dumps(res)
        print(line)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            open(args.out, "w").write(line + "\n")
        return
    torch.manual_seed(1)
    dims, G, MB, BATCH = (4, 84, 84), 128, 256, 1024
    model = models.TVFModel(encoder="nature", input_dims=dims, actions=18, device="cuda", architecture="single",
                            hidden_units=512, use_rnd=True, observation_normalization=True, head_scale=0.1, head_bias=True,
                            value_head_names=("ext", "int"))
    rng = np.random.default_rng(0)
    obs = torch.from_numpy(rng.integers(0, 256, size=(BATCH, *dims), dtype=np.uint8)).cuda()
    model.obs_norm.update(obs)
    group = obs[:G].contiguous()
    index = torch.from_numpy(rng.permutation(BATCH)[:MB].astype(np.int32)).cuda()
    stats = torch.zeros(_lib.PPO_RND_STATS, device="cuda")
    rnd, net = model.rnd, model.policy_net
    err = torch.empty(G, device="cuda")

    variants = {
        "rollout_rnd_error_128": lambda: rnd.prediction_error(group, err=err, err_stride=1),
        "rollout_policy_forward_128": lambda: net.forward(group),
        "train_rnd_minibatch_256": lambda: rnd.train_minibatch(obs, index=index, stats=stats),
        "train_rnd_adam_step": lambda: rnd.adam_step(),
    }
    launches = {"rollout_rnd_error_128": count_calls(rnd, variants["rollout_rnd_error_128"]),
                "train_rnd_minibatch_256": count_calls(rnd, variants["train_rnd_minibatch_256"])}
    times = {k: [] for k in variants}
    for step in range(args.warmup + args.steps):
        for k, fn in variants.items():
            t = timed(fn)
            if step >= args.warmup:
                times[k].append(t)
    res = {k: summary(v) for k, v in times.items()}
    res["rnd_over_policy_forward"] = res["rollout_rnd_error_128"]["median_us"] / res["rollout_policy_forward_128"]["median_us"]
    res["launches"] = {k: {"entry_point_calls": len(v), "names": v} for k, v in launches.items()}
    res["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
