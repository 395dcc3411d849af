#!/usr/bin/env python3
"""Time the replay buffer at the sizes a run uses (MI355X; the table of DESIGN.md's experience-replay section).

    python tools/replay_bench.py [--size 32768] [--steps 30] [--rollouts 8] [--out FILE.json]

One process, the variants interleaved.  Each replay operation is timed twice: on the device with HIP events around the
call (the launch alone) and on the host with a synchronise before and after (what a training iteration waits for: the
index plan and its np.random draws, the upload of the index vectors, the launch, and for the diversity call the copy of
the M x M result and the float64 arithmetic on it).
  add        add_experience of a 128 x 128 rollout (16384 rows of 4x84x84 uint8, 462 MB) into a FULL buffer of --size rows,
             mode uniform (the DNA setting) - the entries it keeps, each to a drawn slot - and mode sequential (all 16384)
  gather     a distil batch of 16384 rows drawn without replacement from the full buffer, one gather launch
  diversity  estimate_replay_diversity(128): 128 x 128 exact squared distances of 28224-byte rows, and log_stats as a whole
  env step   Runner.generate_rollout of 256 synthetic envs (two pipelined groups of 128, 4x84x84) x 32 steps, replay off,
             per env step - the yardstick the three stand beside (the method of tools/hash_bench.py)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ppo_amd import _lib, logger, models, replay  # noqa: E402

SHAPE, ROLLOUT = (4, 84, 84), 128 * 128


def timed(fn):
    """(device us between two events around fn, host us from a synchronise before to one after)."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3, (time.perf_counter() - t0) * 1e6


def summary(v):
    v = np.asarray(v)
    return {"median_us": float(np.median(v)), "p10_us": float(np.percentile(v, 10)), "p90_us": float(np.percentile(v, 90)),
            "n": int(v.size)}


def replay_rows(size, steps, warmup):
    gen = torch.Generator(device="cuda").manual_seed(0)
    rollout_obs = torch.randint(0, 256, (ROLLOUT, *SHAPE), dtype=torch.uint8, device="cuda", generator=gen)
    aux = torch.zeros((ROLLOUT, replay.ExperienceReplayBuffer.N_AUX), device="cuda")
    bufs = {}
    for mode in ("uniform", "sequential"):
        buf = replay.ExperienceReplayBuffer(size, SHAPE, np.uint8, mode=mode, device="cuda")
        k = 0
        while buf.current_size < size:  # fill it
            aux[:, buf.AUX_STEP] = torch.arange(k * ROLLOUT, (k + 1) * ROLLOUT, device="cuda")
            buf.add_experience(rollout_obs, aux)
            k += 1
        bufs[mode] = buf
    buf = bufs["uniform"]
    out = torch.empty((ROLLOUT, *SHAPE), dtype=torch.uint8, device="cuda")
    sample_dev = torch.from_numpy(np.random.choice(size, ROLLOUT, replace=False).astype(np.int32)).cuda()
    index_dev = torch.from_numpy(np.random.choice(size, 128, replace=False).astype(np.int32)).cuda()

    def draw_and_gather():
        s = np.random.choice(size, ROLLOUT, replace=False)
        buf.gather(torch.from_numpy(s.astype(np.int32)).to("cuda", non_blocking=True), out)

    def pairwise_launch():
        replay._call(buf.lib, "ppo_replay_pairwise_sqdist_u8", buf._data.data_ptr(), size, buf.row_bytes, index_dev.data_ptr(),
                     128, buf._d2.data_ptr())

    log = logger.Logger(quiet=True)
    variants = {"add_uniform_full_buffer": lambda: bufs["uniform"].add_experience(rollout_obs, aux),
                "add_sequential_full_buffer": lambda: bufs["sequential"].add_experience(rollout_obs, aux),
                "gather_16384_rows_launch": lambda: buf.gather(sample_dev, out),
                "gather_16384_rows_with_draw": draw_and_gather,
                "pairwise_128_rows_launch": pairwise_launch,
                "estimate_replay_diversity_128": lambda: buf.estimate_replay_diversity(128),
                "log_stats": lambda: buf.log_stats(log)}
    dev, host = {k: [] for k in variants}, {k: [] for k in variants}
    for step in range(warmup + steps):
        for k, fn in variants.items():
            d, h = timed(fn)
            if step >= warmup:
                dev[k].append(d)
                host[k].append(h)
    res = {k: {"device": summary(dev[k]), "host": summary(host[k])} for k in variants}
    res["rows_kept_by_the_uniform_add"] = int(bufs["uniform"].stats_last_entries_added)
    res["buffer_rows"], res["row_bytes"] = size, buf.row_bytes
    return res


def env_step_row(rollouts, warmup):
    from ppo_amd import envs, rollout
    from ppo_amd.config import args as cfg
    N, A = 32, 256
    cfg.setup(["--model_encoder=nature", "--model_architecture=single", "--env_type=synthetic", "--env_embed_time=False",
               "--seed=1", "--disable_logging=True", "--device=cuda", f"--agents={A}", f"--n_steps={N}", "--env_warmup_period=5"])
    torch.manual_seed(1)
    shape, n_actions = envs.get_env_spec()
    model = models.TVFModel(encoder="nature", input_dims=shape, actions=n_actions, device="cuda", architecture="single",
                            hidden_units=512, head_scale=0.1, head_bias=True)
    r = rollout.Runner(model, logger.Logger(quiet=True))
    r.vec_env = envs.create_envs_classic()
    r.reset()
    times = []
    for k in range(warmup + rollouts):
        _d, h = timed(r.generate_rollout)
        if k >= warmup:
            times.append(h / (N + 1))
    return {"rollout_env_step": summary(times), "steps_per_rollout": N, "agents": A}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=32768, help="rows of the buffer (a multiple of 16384 fills exactly)")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--rollouts", type=int, default=8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    _lib.require_gpu()
    np.random.seed(0)
    res = {"replay": replay_rows(a.size, a.steps, 3), "runner": env_step_row(a.rollouts, 2), "device": torch.cuda.get_device_name(0)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
