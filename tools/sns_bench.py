#!/usr/bin/env python3
"""Time noise-scale estimation at the sizes a run uses (MI355X; the tables of DESIGN.md §7.9).

    python tools/sns_bench.py [--rollouts 6] [--steps 200] [--out FILE.json]

One process, HIP events on the current stream, the variants interleaved, medians with p10 - p90:
  kernels   on a flat buffer of the IMPALA net's size (4x84x84, 256 hidden units): the fused per-pass launch
            (ppo_grad_noise_pass_f32, accumulating form) against the two launches it replaces - ppo_accumulate_f32 and the
            optimiser's sum-of-g^2 launch.  That launch has no entry point of its own: it is taken as
            ppo_adam_step_f32 (sum of g^2 + Adam) minus ppo_adam_step_presummed_f32 (Adam alone), lr = 0 on scratch buffers.
            ppo_moments_f64 (two launches, float64) is timed as the form with an entry point.  A sample is REPS calls
            back to back between two events, divided by REPS.
  runner    256 synthetic envs x 128 steps, IMPALA, dual, TVF (128 heads): rollout, returns, then each phase timed on the
            host around a device synchronisation, with --sns_enabled off and on (period 1) alternating rollout by
            rollout on ONE runner; the estimates' seconds are the runner's own sns_time_* / t_s_heads log entries."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ppo_amd import _lib, models  # noqa: E402

REPS = 16


def timed(fn, reps=1):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps  # us


def summary(v, unit="us"):
    v = np.asarray(v)
    return {f"median_{unit}": float(np.median(v)), f"p10_{unit}": float(np.percentile(v, 10)),
            f"p90_{unit}": float(np.percentile(v, 90)), "n": int(v.size)}


def kernel_rows(steps, warmup):
    lib = _lib.load()
    n = models.DualHeadNet("impala", (4, 84, 84), 6, hidden_units=256, device="cuda").grad.numel()
    st = _lib.current_stream
    g = torch.randn(n, device="cuda")
    acc, w, m, v = (torch.zeros(n, device="cuda") for _ in range(4))
    ws = torch.zeros(lib.ppo_grad_noise_workspace_bytes(REPS) // 8, dtype=torch.float64, device="cuda")
    out = torch.zeros(REPS + 1, dtype=torch.float64, device="cuda")
    adam_ws = torch.ones(lib.ppo_adam_workspace_bytes() // 4, device="cuda")  # (the presummed step reads one partial)
    mom, mom_ws = torch.zeros(3, dtype=torch.float64, device="cuda"), torch.zeros(lib.ppo_moments_workspace_bytes() // 8,
                                                                                  dtype=torch.float64, device="cuda")
    norm = torch.zeros(1, device="cuda")
    p = lambda t: t.data_ptr()  # noqa: E731
    adam = (p(w), p(g), p(m), p(v), n, 1, 0.0, 0.9, 0.999, 1e-5, 20.0, 1.0, p(adam_ws))

    def check(rc):
        if rc:
            _lib.check(rc, "sns_bench")
    variants = {
        "fused_pass": lambda: check(lib.ppo_grad_noise_pass_f32(p(g), p(acc), n, 1, REPS, p(ws), st())),
        "accumulate": lambda: check(lib.ppo_accumulate_f32(p(acc), p(g), n, st())),
        "adam_with_sumsq": lambda: check(lib.ppo_adam_step_f32(*adam, p(norm), st())),
        "adam_presummed": lambda: check(lib.ppo_adam_step_presummed_f32(*adam, 1, p(norm), st())),
        "moments_f64": lambda: check(lib.ppo_moments_f64(p(g), n, p(mom), p(mom_ws), st())),
        "finish": lambda: check(lib.ppo_grad_noise_finish_f64(p(acc), n, REPS, REPS, p(ws), p(out), st())),
    }
    times = {k: [] for k in variants}
    for step in range(warmup + steps):
        for k, fn in variants.items():
            t = timed(fn, REPS)
            if step >= warmup:
                times[k].append(t)
    res = {k: summary(t) for k, t in times.items()}
    res["n_floats"] = n
    sumsq = res["adam_with_sumsq"]["median_us"] - res["adam_presummed"]["median_us"]
    res["sumsq_launch_us_by_difference"] = sumsq
    res["two_launch_us"] = res["accumulate"]["median_us"] + sumsq
    res["accumulate_plus_moments_us"] = res["accumulate"]["median_us"] + res["moments_f64"]["median_us"]
    return res


def runner_rows(rollouts, warmup):
    import train
    from ppo_amd import envs, logger, rollout
    from ppo_amd.config import args as cfg
    N, A = 128, 256
    flags = ["--model_encoder=impala", "--model_architecture=dual", "--env_type=synthetic", "--env_embed_time=False",
             "--seed=1", "--disable_logging=True", "--device=cuda", f"--agents={A}", f"--n_steps={N}", "--env_warmup_period=5",
             "--tvf_enabled=True", "--disable_ev=True", "--sns_enabled=True", "--sns_period=1"]
    cfg.setup(flags)
    torch.manual_seed(1)
    np.random.seed(1)
    log = logger.Logger(quiet=True)
    r = rollout.Runner(train.make_model(log), log)
    r.vec_env = envs.create_envs_classic()
    r.reset()
    phases = (("policy", r.train_policy), ("value", r.train_value), ("distil", r.train_distil))
    phase_s = {(k, on): [] for k, _ in phases for on in (False, True)}
    est_s = {k: [] for k in ("policy", "value", "distil", "value_heads")}
    for k in range(2 * (warmup + rollouts)):
        on = bool(k % 2)
        cfg.sns.enabled = on
        r.generate_rollout()
        r.calculate_returns()
        r._phase_stats = {}
        for name, fn in phases:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if k >= 2 * warmup:
                phase_s[(name, on)].append(time.perf_counter() - t0)
        r.batch_counter += 1
        if on and k >= 2 * warmup:
            for name in ("policy", "value", "distil"):
                est_s[name].append(log.vars[f"sns_time_{name}"].history[-1] * cfg.sns.period)
            est_s["value_heads"].append(log.vars["t_s_heads"].history[-1] * cfg.sns.period)
    res = {"agents": A, "n_steps": N, "tvf_heads": r.K, "b_small": cfg.sns.b_small, "b_big": cfg.sns.b_big,
           "max_heads": cfg.sns.max_heads, "policy_passes": N * A // cfg.sns.b_small,
           "parameters": {"policy_net": r.policy_net.n_parameters(), "value_net": r.value_net.n_parameters()}}
    for (name, on), v in phase_s.items():
        res[f"phase_{name}_sns_{'on' if on else 'off'}"] = summary(v, "s")
    for name, v in est_s.items():
        res[f"estimate_{name}"] = summary(v, "s")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rollouts", type=int, default=6)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    _lib.require_gpu()
    res = {"kernels": kernel_rows(a.steps, 20), "runner": runner_rows(a.rollouts, 1), "device": torch.cuda.get_device_name(0)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
