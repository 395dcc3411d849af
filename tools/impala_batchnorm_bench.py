"""Times the batch-norm entry points (ppo_batchnorm_*, csrc/batchnorm.hip) at the three residual-block geometries of the
84x84 IMPALA net, beside torch's own batch_norm on the same device (for orientation), and the env-steps/s of the training
loop on the synthetic env with and without batch_norm=True.  Prints the tables of profiles/impala_batchnorm.md.

    python tools/impala_batchnorm_bench.py [--batch 256] [--train-iterations 6] [--out FILE]

Kernel method: that of tools/impala_any_bench.py (three warm launches, then windows of back-to-back launches bracketed by
HIP events, at least 0.1 s and 10 launches each; all sides alternate, three windows of each, the median is reported).  A
`call` is an entry point: the batch form and the backward are two launches each.  Bytes are the algorithm's: the batch
form reads x twice and writes z (3 maps), the running form reads x and writes z (2), the backward with a residual reads
dz, x and the residual and writes dx (4); the partial sums are c * slices * 16 bytes and are not counted.
Training method: Runner iterations (rollout, returns, train) of one process per configuration are not comparable with
another process's to better than the machine's noise, so both models are built in this process and their iterations
alternate; the first two of each are warm-up; the median of the rest is reported."""
import argparse
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from impala_any_bench import _p, measure  # noqa: E402
from ppo_amd import _lib  # noqa: E402

SHAPES = [(16, 42, 42), (32, 21, 21), (32, 11, 11)]
EPS, MOM = 1e-5, 0.1
TRAIN_FLAGS = ["--agents=256", "--n_steps=64", "--model_architecture=single", "--model_encoder=impala", "--env_type=synthetic",
               "--env_embed_time=False", "--seed=1", "--policy_opt_mini_batch_size=2048", "--policy_opt_epochs=2",
               "--disable_logging=True"]


def kernels(B, lines):
    lib, dev = _lib.load(), torch.device("cuda")
    g = torch.Generator(device="cpu").manual_seed(1)
    lines += ["| map | call | launches | us per call | algorithmic GB | GB/s | torch us |", "|---|---|---|---|---|---|---|"]
    for c, h, w in SHAPES:
        shape = (B, c, h, w)
        x, dz, res = (torch.randn(shape, generator=g).to(dev) for _ in range(3))
        z, dx = torch.empty_like(x), torch.empty_like(x)
        gamma, beta = (torch.rand(c, generator=g) + 0.5).to(dev), torch.randn(c, generator=g).to(dev)
        rm, rv = torch.zeros(c, device=dev), torch.ones(c, device=dev)
        nbt = torch.zeros((), dtype=torch.int64, device=dev)
        dg, db = torch.empty(c, device=dev), torch.empty(c, device=dev)
        nbytes = int(lib.ppo_batchnorm_workspace_bytes(c))
        ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
        trm, trv = torch.zeros(c, device=dev), torch.ones(c, device=dev)
        xg = x.clone().requires_grad_(True)
        tg, tb = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)

        def torch_backward(_st):
            y = F.batch_norm(xg, trm, trv, tg, tb, False, MOM, EPS)
            torch.autograd.grad(y, (xg, tg, tb), dz)
            return 0

        calls = [
            ("batch forward", 2, 3,
             lambda st: lib.ppo_batchnorm_batch_forward_f32(_p(x), _p(gamma), _p(beta), _p(rm), _p(rv), _p(nbt), _p(z), None, None,
                                                            _p(ws), nbytes, B, c, h, w, EPS, MOM, st),
             lambda _st: (F.batch_norm(x, trm, trv, gamma, beta, True, MOM, EPS), 0)[1]),
            ("running forward", 1, 2,
             lambda st: lib.ppo_batchnorm_running_forward_f32(_p(x), _p(gamma), _p(beta), _p(rm), _p(rv), _p(z), B, c, h, w, EPS, st),
             lambda _st: (F.batch_norm(x, trm, trv, gamma, beta, False, MOM, EPS), 0)[1]),
            ("running backward (+ residual)", 2, 4,
             lambda st: lib.ppo_batchnorm_running_backward_f32(_p(dz), _p(x), _p(res), _p(gamma), _p(rm), _p(rv), _p(dx), _p(dg),
                                                               _p(db), _p(ws), nbytes, B, c, h, w, EPS, 0, st),
             torch_backward),  # (torch's: forward + autograd of the eval-mode layer, no residual - orientation only)
        ]
        for name, launches, maps, ours, theirs in calls:
            t, tt = measure([ours, theirs])
            gb = maps * x.numel() * 4 / 1e9
            lines.append(f"| {B}x{c}x{h}x{w} | {name} | {launches} | {t * 1e6:.1f} | {gb:.4f} | {gb / t:.0f} | {tt * 1e6:.1f} |")
            print(lines[-1], flush=True)


def training(iterations, lines):
    import numpy as np
    from ppo_amd import envs, logger, models, rollout
    from ppo_amd.config import args
    runners = {}
    for label, extra in (("batch_norm=False", []), ("batch_norm=True", ["--model_encoder_args={'batch_norm': True}"])):
        args.setup([*TRAIN_FLAGS, *extra])
        torch.manual_seed(1)
        np.random.seed(1)
        shape, nA = envs.get_env_spec()
        model = models.TVFModel("impala", encoder_args=args.model.encoder_args, input_dims=shape, actions=nA, device="cuda",
                                architecture="single", hidden_units=args.model.hidden_units, head_scale=0.1, head_bias=True)
        r = rollout.Runner(model, logger.Logger(quiet=True))
        r.vec_env = envs.create_envs_classic()
        r.reset()
        runners[label] = (r, list(extra))
    times = {k: ([], [], []) for k in runners}
    for _ in range(iterations + 2):
        for label, (r, _extra) in runners.items():  # (the flags the loop reads are the same for both)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r.generate_rollout()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            r.calculate_returns()
            r.train()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            for k, v in zip(times[label], (t1 - t0, t2 - t1, t2 - t0)):
                k.append(v)
    lines += ["", "| model | rollout ms | returns + train ms | iteration ms | env-steps/s |", "|---|---|---|---|---|"]
    for label, (r, _e) in runners.items():
        ro, tr, it = (statistics.median(v[2:]) for v in times[label])
        lines.append(f"| {label} | {ro * 1e3:.1f} | {tr * 1e3:.1f} | {it * 1e3:.1f} | {r.N * r.A / it:.0f} |")
        print(lines[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--train-iterations", type=int, default=6)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    _lib.require_gpu()
    lines = [f"Device: {torch.cuda.get_device_name(0)}; batch {a.batch}; microseconds per call (median of three windows).", ""]
    kernels(a.batch, lines)
    if a.train_iterations > 0:
        lines += ["", f"Training loop, synthetic env (4, 84, 84), 256 envs x 64 steps, 2 epochs of 2048-sample minibatches, exact "
                  f"float32; median of {a.train_iterations} alternating iterations."]
        training(a.train_iterations, lines)
    text = "\n".join(lines)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
