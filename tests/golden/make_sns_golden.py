#!/usr/bin/env python3
"""Generate tests/golden/sns_golden.json: the REFERENCE's simple noise scale (rl/sns.py) on the CPU.

Build container only (needs the reference checkout; see ref_shim.py):  python tests/golden/make_sns_golden.py

Everything comes from the reference's own functions, driven with stub runners; the file holds data only.

(i) `sequences`: rl.sns.process_noise_scale called CALLS times per label (policy, value, acc_head_3) in each smoothing
    mode, on a runner of N x A = 16 x 16.  The input pairs (g_small^2, g_big^2) are drawn from a seeded generator and
    shaped so that the first three make est_g2 - and with it the smoothed g2 - negative (the max(0, .) + 1e-4 clip), and
    every fourth has g_big^2 > g_small^2 (est_s < 0).  `policy` passes b_big = N * A as estimate_noise_scale does.  After
    every call the file records every log key written and the whole of noise_stats.
    `avg` mode runs as the reference has it.  `ema` mode - the reference's default - raises AttributeError there, because
    process_noise_scale calls get_ema_constant(horizon, period) without the runner the function's first parameter
    stands for (rl/sns.py:60, 62).  The generator therefore binds the runner into that call and leaves the function itself
    untouched: get_ema_constant(runner, horizon, period) is the evident intent, and the numbers are the reference's own
    arithmetic under it.
(ii) `fake`: rl.sns.log_fake_accumulated_gradient_norms under np.random.seed(FAKE_SEED) with an optimiser of d = 64
    parameters and horizons that include 0; the logged values and the next np.random.rand().
(iii) `estimate`: rl.sns.estimate_noise_scale on a stub: one 8-parameter vector theta, loss mean_b(x_b . theta), x integer
    valued in [-4, 4], 64 rows, b_small = 4, b_big = 32, np.random.seed(EST_SEED).  Stored: x, the sample drawn, the two
    squared norms handed to process_noise_scale and the next np.random.rand().
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
CALLS, SEQ_SEED, FAKE_SEED, EST_SEED = 14, 11, 23, 5
N, A = 16, 16
LABELS = ("policy", "value", "acc_head_3")


class StubLog:
    LM_MUTE, LM_DEFAULT = "mute", "default"

    def __init__(self):
        self.mode = self.LM_DEFAULT
        self.seen = {}

    def watch(self, key, value, **kw):
        self.seen[key] = float(value)

    def watch_mean(self, key, value, **kw):
        self.seen[key] = float(value)


class StubModel:
    device = "cpu"


class StubRunner:
    def __init__(self, horizons=None):
        self.N, self.A = N, A
        self.noise_stats = {}
        self.log = StubLog()
        self.model = StubModel()
        self.batch_counter = 0
        self.tvf_horizons = horizons


def plain_stats(stats):
    out = {}
    for k, v in stats.items():
        if hasattr(v, "maxlen"):
            out[k] = {"values": [float(x) for x in v], "maxlen": v.maxlen}
        elif isinstance(v, set):
            out[k] = sorted(int(x) for x in v)
        else:
            out[k] = float(v)
    return out


def input_pairs(label_index):
    rng = np.random.default_rng(SEQ_SEED + label_index)
    pairs = []
    for i in range(CALLS):
        g_small = float(rng.uniform(0.5, 2.0))
        if i < 3:
            g_big = g_small * 0.01  # est_g2 < 0: the smoothed g2 starts negative
        elif i % 4 == 3:
            g_big = g_small * float(rng.uniform(1.05, 1.5))  # est_s < 0
        else:
            g_big = g_small * float(rng.uniform(0.2, 0.9))
        pairs.append([g_small, g_big])
    return pairs


def main():
    from ref_shim import load_reference
    rl = load_reference(["--device=cpu", "--output_folder=/tmp/ref_golden_out"])
    import torch
    from rl import sns as ref_sns
    args = rl.config.args

    out = {"N": N, "A": A, "labels": list(LABELS), "sequences": {}}
    args.sns.enabled = True
    args.sns.period = 3
    args.sns.b_small, args.sns.b_big = 128, 2048
    out["config"] = {"period": args.sns.period, "b_small": args.sns.b_small, "b_big": args.sns.b_big,
                     "smoothing_horizon_avg": float(args.sns.smoothing_horizon_avg),
                     "smoothing_horizon_s": float(args.sns.smoothing_horizon_s),
                     "smoothing_horizon_g2": float(args.sns.smoothing_horizon_g2),
                     "smoothing_horizon_policy": float(args.sns.smoothing_horizon_policy)}
    original_ema = ref_sns.get_ema_constant
    for mode in ("avg", "ema"):
        args.sns.smoothing_mode = mode
        runner = StubRunner()
        if mode == "ema":
            # the reference's call site leaves the runner out (module docstring): bind it, keep the function
            ref_sns.get_ema_constant = lambda horizon, period, _r=runner: original_ema(_r, horizon, period)
        steps = []
        try:
            for li, label in enumerate(LABELS):
                for g_small, g_big in input_pairs(li):
                    runner.log.seen = {}
                    ratio = ref_sns.process_noise_scale(runner, g_small, g_big, label, b_big=N * A if label == "policy" else None)
                    steps.append({"label": label, "g_small": g_small, "g_big": g_big, "ratio": float(ratio),
                                  "log": dict(runner.log.seen), "noise_stats": plain_stats(runner.noise_stats)})
        finally:
            ref_sns.get_ema_constant = original_ema
        out["sequences"][mode] = steps
    out["ema_constant_16x16_0.2e6_3"] = float(original_ema(StubRunner(), 0.2e6, 3))

    # ---- (ii) fake noise
    args.sns.smoothing_mode = "avg"
    args.sns.b_small, args.sns.b_big, args.sns.max_heads = 4, 32, 3
    horizons = [0, 1, 3, 10, 30]
    runner = StubRunner(horizons)
    opt = torch.optim.SGD([torch.zeros(64, requires_grad=True)], lr=0.1)
    np.random.seed(FAKE_SEED)
    ref_sns.log_fake_accumulated_gradient_norms(runner, opt)
    out["fake"] = {"seed": FAKE_SEED, "d": 64, "horizons": horizons, "b_small": 4, "b_big": 32, "max_heads": 3,
                   "log": dict(runner.log.seen), "noise_stats": plain_stats(runner.noise_stats),
                   "next_rand": float(np.random.rand())}

    # ---- (iii) estimate_noise_scale on a stub
    x = np.random.default_rng(EST_SEED).integers(-4, 5, (64, 8)).astype(np.float32)
    theta = torch.zeros(8, requires_grad=True)
    opt = torch.optim.SGD([theta], lr=0.1)
    runner = StubRunner()
    seen = {}

    def mini_batch_func(data):
        (data["prev_state"] @ theta).mean().backward()

    def record(runner_, g_small, g_big, label, verbose=True, b_small=None, b_big=None):
        seen.update(g_small=float(g_small), g_big=float(g_big), label=label, b_big=b_big)

    choice = np.random.choice
    drawn = []

    def recording_choice(*a, **k):
        r = choice(*a, **k)
        drawn.append([int(v) for v in r])
        return r

    original_process = ref_sns.process_noise_scale
    ref_sns.process_noise_scale = record
    np.random.choice = recording_choice
    try:
        np.random.seed(EST_SEED)
        ref_sns.estimate_noise_scale(runner, {"prev_state": x}, mini_batch_func, opt, "value")
    finally:
        ref_sns.process_noise_scale = original_process
        np.random.choice = choice
    out["estimate"] = {"seed": EST_SEED, "x": x.astype(int).tolist(), "b_small": 4, "b_big": 32, "sample": drawn[0],
                       "g_small": seen["g_small"], "g_big": seen["g_big"], "next_rand": float(np.random.rand())}

    path = os.path.join(HERE, "sns_golden.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
