"""The optimiser launches on the flat buffers the nets really have: the Adam pair (grad_sumsq_kernel + adam_kernel) and
the SGD pair (grad_sumsq_kernel + sgd_kernel) of csrc/optim.hip over the IMPALA net's buffer (4 x 84 x 84, 256 hidden
units) and the 256-unit MLP's, alternating in one process after warm-up.  Meant to run under a kernel trace, which gives
the per-kernel times (profiles/sgd_step.md); on its own it prints the buffer sizes and HIP-event times per pair.
usage (GPU box): rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/optim_launch_times.py"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ppo_amd import _lib, models  # noqa: E402


def _p(t):
    return t.data_ptr()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=9)
    ap.add_argument("--launches", type=int, default=200)
    a = ap.parse_args()
    lib, st = _lib.load(), _lib.current_stream()
    nets = {"impala": models.DualHeadNet("impala", (4, 84, 84), 6, hidden_units=256, head_scale=0.1, head_bias=True),
            "mlp256": models.DualHeadNet("mlp", (11,), 3, hidden_units=256, head_scale=0.1, head_bias=True)}
    for name, net in nets.items():
        n = net.flat.numel()
        w, g = net.flat.clone(), torch.randn_like(net.flat) * 1e-3
        m, v = torch.zeros_like(w), torch.zeros_like(w)
        ws = torch.zeros(lib.ppo_adam_workspace_bytes() // 4, device=w.device)
        norm = torch.zeros(1, device=w.device)

        def adam():
            _lib.check(lib.ppo_adam_step_f32(_p(w), _p(g), _p(m), _p(v), n, 1, 2.5e-4, 0.9, 0.999, 1e-5, 20.0, 1.0, _p(ws),
                                             _p(norm), st), "adam")

        def sgd():
            _lib.check(lib.ppo_sgd_step_f32(_p(w), _p(g), n, 2.5e-4, 20.0, 1.0, _p(ws), _p(norm), st), "sgd")
        fns, times = {"adam": adam, "sgd": sgd}, {"adam": [], "sgd": []}
        for fn in fns.values():
            for _ in range(20):
                fn()
        torch.cuda.synchronize()
        for _ in range(a.blocks):
            for kind, fn in fns.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.launches):
                    fn()
                e1.record()
                e1.synchronize()
                times[kind].append(e0.elapsed_time(e1) * 1e3 / a.launches)
        for kind, t in times.items():
            print(f"OPTIM_PAIR {name} n={n} {kind}: median {statistics.median(t):.2f} us per pair "
                  f"(min {min(t):.2f}, max {max(t):.2f} over {a.blocks} blocks of {a.launches})")


if __name__ == "__main__":
    main()
