#!/usr/bin/env python3
"""Time the RTG encoder's pool kernels, forward and PPO minibatch next to torch on the same GPU (MI355X; the tables of
profiles/rtg_encoder.md).

    python tools/rtg_bench.py [--steps 30] [--reps 20] [--out FILE.json]

One process, HIP events on the current stream, after warm-up, the two sides alternating step by step:
  pool      ppo_maxpool2x2_relu_forward_f32 (with the gate byte) / _backward_f32 at the encoder's three pre-pool maps,
            (32, 41, 41), (64, 20, 20), (64, 10, 10), for n = 256 and n = 2048, against F.relu(F.max_pool2d(x, 2, 2)) and
            its autograd.  A step times `reps` back-to-back launches between two events, so a figure includes the launch
            cadence of the stream, on both sides.  bytes: what the algorithm has to move, from shapes - forward the read of
            `in` plus the writes of `out` and `gate`, backward the reads of `dout` and `gate` plus the write of `din`;
            hbm_frac: bytes / time over the MI355X's 8.0 TB/s HBM3E peak (specification; a float4 copy reaches about
            6.3).  Maps that fit the 256 MiB Infinity Cache stay resident between the launches of a step:
            `fits_infinity_cache` says which rows those are.
  forward   DualHeadNet("rtg").forward of 256 and 2048 uint8 observations (4, 84, 84), hidden 512, against a torch.nn
            twin with the same weights under no_grad
  ppo       ppo_minibatch (forward + PPO loss + backward, no optimiser step) of 256 observations against the twin's
            forward + oracle.model_torch.ppo_loss + backward
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ppo_amd import _lib, models  # noqa: E402

HBM_PEAK = 8.0e12  # bytes / s: HBM3E specification of the MI355X
INFINITY_CACHE = 256 << 20
POOL_MAPS = [(32, 41, 41), (64, 20, 20), (64, 10, 10)]


def timed(fn, reps=1):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps  # us


def summary(v):
    v = np.asarray(v)
    return {"median_us": float(np.median(v)), "p10_us": float(np.percentile(v, 10)), "p90_us": float(np.percentile(v, 90)),
            "n": int(v.size)}


def alternate(variants, steps, warmup, reps=1):
    times = {k: [] for k in variants}
    for step in range(warmup + steps):
        for k, fn in variants.items():
            t = timed(fn, reps)
            if step >= warmup:
                times[k].append(t)
    return {k: summary(v) for k, v in times.items()}


def pool_rows(steps, reps):
    lib = _lib.load()
    rows = []
    for n in (256, 2048):
        for c, h, w in POOL_MAPS:
            ho, wo = h // 2, w // 2
            x = torch.randn((n, c, h, w), device="cuda")
            out = torch.empty((n, c, ho, wo), device="cuda")
            gate = torch.empty((n, c, ho, wo), dtype=torch.uint8, device="cuda")
            dout = torch.randn((n, c, ho, wo), device="cuda")
            din = torch.empty_like(x)
            xg = x.clone().requires_grad_(True)
            y = F.relu(F.max_pool2d(xg, 2, 2))

            def hip_fwd():
                rc = lib.ppo_maxpool2x2_relu_forward_f32(x.data_ptr(), out.data_ptr(), gate.data_ptr(), n, c, h, w,
                                                         _lib.current_stream())
                _lib.check(rc, "ppo_maxpool2x2_relu_forward_f32")

            def hip_bwd():
                rc = lib.ppo_maxpool2x2_relu_backward_f32(dout.data_ptr(), gate.data_ptr(), din.data_ptr(), n, c, h, w,
                                                          _lib.current_stream())
                _lib.check(rc, "ppo_maxpool2x2_relu_backward_f32")

            def torch_fwd():
                with torch.no_grad():
                    F.relu(F.max_pool2d(x, 2, 2))

            def torch_bwd():
                torch.autograd.grad(y, xg, dout, retain_graph=True)

            hip_fwd()
            hip_bwd()
            assert torch.equal(out, y.detach()) and torch.equal(din, torch.autograd.grad(y, xg, dout, retain_graph=True)[0])
            t = alternate({"hip_forward": hip_fwd, "torch_forward": torch_fwd, "hip_backward": hip_bwd,
                           "torch_backward": torch_bwd}, steps, 5, reps)
            windows, elems = n * c * ho * wo, n * c * h * w
            fwd_bytes, bwd_bytes = elems * 4 + windows * 5, windows * 5 + elems * 4
            row = {"n": n, "map": [c, h, w], "forward_bytes": fwd_bytes, "backward_bytes": bwd_bytes,
                   "fits_infinity_cache": bool(fwd_bytes < INFINITY_CACHE), **t}
            for side, nbytes in (("forward", fwd_bytes), ("backward", bwd_bytes)):
                us = t[f"hip_{side}"]["median_us"]
                row[f"hip_{side}_tb_per_s"] = nbytes / us * 1e-6
                row[f"hip_{side}_hbm_frac"] = nbytes / (us * 1e-6) / HBM_PEAK
                row[f"torch_over_hip_{side}"] = t[f"torch_{side}"]["median_us"] / us
            rows.append(row)
            print(f"pool n={n} map={c}x{h}x{w}: forward {t['hip_forward']['median_us']:.1f} us (torch "
                  f"{t['torch_forward']['median_us']:.1f}), backward {t['hip_backward']['median_us']:.1f} us (torch "
                  f"{t['torch_backward']['median_us']:.1f})", file=sys.stderr, flush=True)
            del x, out, gate, dout, din, xg, y
            torch.cuda.empty_cache()
    return rows


class TorchTwin(torch.nn.Module):
    """RTG_LSTM + heads (rl/models.py:172-213, 364-368) in plain torch, weights copied from a DualHeadNet."""

    def __init__(self, net):
        super().__init__()
        sd = net.state_dict()
        self.p = torch.nn.ParameterDict({k.replace(".", "_"): torch.nn.Parameter(v.detach().clone()) for k, v in sd.items()})

    def forward(self, x):
        p = self.p
        h = x.float() / 255.0
        for name, stride, padding in (("conv1", 2, 0), ("conv2", 1, 1), ("conv3", 1, 1)):
            h = F.relu(F.max_pool2d(F.conv2d(h, p[f"encoder_{name}_weight"], p[f"encoder_{name}_bias"], stride=stride,
                                             padding=padding), 2, 2))
        feat = F.relu(F.linear(h.reshape(h.shape[0], -1), p["encoder_fc_weight"], p["encoder_fc_bias"]))
        return {"raw_policy": F.linear(feat, p["policy_head_weight"], p["policy_head_bias"]),
                "value": F.linear(feat, p["value_head_weight"], p["value_head_bias"]),
                "advantage": F.linear(feat, p["advantage_head_weight"], p["advantage_head_bias"])}


def net_rows(steps):
    from oracle import model_torch as R
    nA = 6
    torch.manual_seed(1)
    net = models.DualHeadNet("rtg", (4, 84, 84), nA, hidden_units=512, head_scale=0.1, head_bias=True, device="cuda")
    twin = TorchTwin(net).cuda()
    res = {}
    g = torch.Generator(device="cuda").manual_seed(2)
    for B in (256, 2048):
        x = torch.randint(0, 256, (B, 4, 84, 84), dtype=torch.uint8, device="cuda", generator=g)

        def torch_fwd():
            with torch.no_grad():
                twin(x)

        a, b = net.forward(x)["raw_policy"], twin(x)["raw_policy"]
        res[f"forward_{B}_max_abs_diff"] = float((a - b).abs().max())
        res[f"forward_{B}"] = alternate({"hip": lambda: net.forward(x), "torch": torch_fwd}, steps, 5)
    B = 256
    x = torch.randint(0, 256, (B, 4, 84, 84), dtype=torch.uint8, device="cuda", generator=g)
    actions = torch.randint(0, nA, (B,), dtype=torch.int32, device="cuda", generator=g)
    logp = torch.log_softmax(torch.randn(B, nA, device="cuda", generator=g), dim=1)
    pac = logp.gather(1, actions.long()[:, None])[:, 0].contiguous()
    adv, ret = torch.randn(B, device="cuda", generator=g), torch.randn(B, 1, device="cuda", generator=g)

    def torch_ppo():
        twin.zero_grad(set_to_none=True)
        o = twin(x)
        o["log_policy"] = torch.log_softmax(o["raw_policy"], dim=1)
        R.ppo_loss(o, actions.long(), pac, adv, ret).backward()

    res[f"ppo_minibatch_{B}"] = alternate({"hip": lambda: net.ppo_minibatch(x, actions, pac, logp, adv, ret),
                                           "torch": torch_ppo}, steps, 5)
    for k in (f"forward_256", "forward_2048", f"ppo_minibatch_{B}"):
        res[k]["torch_over_hip"] = res[k]["torch"]["median_us"] / res[k]["hip"]["median_us"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    _lib.require_gpu()
    res = {"pool": pool_rows(a.steps, a.reps), "net": net_rows(a.steps), "device": torch.cuda.get_device_name(0),
           "steps": a.steps, "reps": a.reps}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
