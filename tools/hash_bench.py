#!/usr/bin/env python3
"""Time state hashing at the sizes a run uses (MI355X; the table of DESIGN.md's state-hashing section).

    python tools/hash_bench.py [--rollouts 12] [--steps 200] [--out FILE.json]

One process, HIP events on the current stream, the variants interleaved:
  runner    Runner.generate_rollout of 256 synthetic envs (two pipelined groups of 128, 4x84x84) x 32 steps with hashing
            off and on (raw input, 16 bits, bonus 0.01) alternating rollout by rollout - the method of tools/rollout_ab.py;
            reported per env step (a rollout's time / 33 policy steps).  The synthetic env is not `atari`: all four planes
            are hashed (D = 28224), four times the bytes of the atari setting.  The `on` rollout includes the
            once-per-rollout table update and bonus.
  kernels   the hash launch of one group of 128 rows with one plane (D = 7056, the atari setting) and with all planes;
            the table update, the bonus and the two logged counts of a 128 x 256 rollout at 16 bits."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ppo_amd import _lib, hashing, models  # noqa: E402


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


def runner_rows(rollouts, warmup):
    from ppo_amd import envs, logger, rollout
    from ppo_amd.config import args as cfg
    N, A = 32, 256
    flags = ["--model_encoder=nature", "--model_architecture=single", "--env_type=synthetic", "--env_embed_time=False",
             "--seed=1", "--disable_logging=True", "--device=cuda", f"--agents={A}", f"--n_steps={N}", "--env_warmup_period=5"]
    runners = {}
    for key, extra in (("off", []), ("on", ["--hash_enabled=True", "--hash_bits=16", "--hash_bonus=0.01"])):
        cfg.setup(flags + extra)
        torch.manual_seed(1)
        shape, n_actions = envs.get_env_spec()
        model = models.TVFModel(encoder="nature", input_dims=shape, actions=n_actions, device="cuda", architecture="single",
                                hidden_units=512, head_scale=0.1, head_bias=True,
                                value_head_names=("ext", "int") if cfg.use_intrinsic_rewards else ("ext",))
        r = rollout.Runner(model, logger.Logger(quiet=True))
        r.vec_env = envs.create_envs_classic()
        r.reset()
        runners[key] = (r, flags + extra)
    times = {"on": [], "off": []}
    for k in range(warmup + rollouts):
        for key, (r, line) in runners.items():
            cfg.setup(line)
            t = timed(r.generate_rollout) / (N + 1)
            if k >= warmup:
                times[key].append(t)
    res = {"rollout_env_step_hash_on": summary(times["on"]), "rollout_env_step_hash_off": summary(times["off"]),
           "steps_per_rollout": N, "agents": A, "hashed_elements": int(runners["on"][0].hash.hasher.in_d)}
    res["hash_added_us_per_env_step"] = res["rollout_env_step_hash_on"]["median_us"] - res["rollout_env_step_hash_off"]["median_us"]
    res["hash_added_fraction_of_step_off"] = res["hash_added_us_per_env_step"] / res["rollout_env_step_hash_off"]["median_us"]
    return res


def kernel_rows(steps, warmup):
    rng = np.random.default_rng(0)
    obs = torch.from_numpy(rng.integers(0, 256, size=(128, 4, 84, 84), dtype=np.uint8)).cuda()
    one = hashing.LinearStateHasher((1, 84, 84), 16, device="cuda")
    full = hashing.LinearStateHasher((4, 84, 84), 16, device="cuda")
    N, A = 128, 256
    tr = hashing.StateHashTracker(one, N, A, bonus=0.01)
    tr.obs_hashes.copy_(torch.from_numpy(rng.integers(0, 2 ** 16, size=(N, A)).astype(np.int32)))
    rewards = torch.zeros((N, A), device="cuda")
    out = torch.empty(128, dtype=torch.int32, device="cuda")
    variants = {"hash_128_rows_one_plane_7056": lambda: one.hash_observations(obs, out=out),
                "hash_128_rows_all_planes_28224": lambda: full.hash_observations(obs, out=out),
                "counts_update_128x256_16_bits": tr.update_counts,
                "bonus_128x256": lambda: tr.add_bonus(rewards),
                "count_stats_16_bits": tr.launch_stats}
    times = {k: [] for k in variants}
    for step in range(warmup + steps):
        for k, fn in variants.items():
            t = timed(fn)
            if step >= warmup:
                times[k].append(t)
    return {k: summary(v) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rollouts", type=int, default=12)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    _lib.require_gpu()
    res = {"kernels": kernel_rows(a.steps, 20), "runner": runner_rows(a.rollouts, 2), "device": torch.cuda.get_device_name(0)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
