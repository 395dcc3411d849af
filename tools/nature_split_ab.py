"""The Nature-CNN convolutions, exact float32 (csrc/conv_strided.hip) against split-bf16 (csrc/conv_strided_bf16x3.hip):
which (layer, pass) pairs belong in models.NATURE_SPLIT.

Per layer at 4 x 84 x 84, n = 128 (a rollout group) and n = 256 (a minibatch), and per pass: the two launches alternate
in one process in blocks of launches timed by HIP events, after warm-up; printed are the median over blocks of each and
the spread (the larger max - min over blocks of the two).  A pair is listed only if the split median is below the
exact median by more than that spread at both n.  Then one whole 256-row policy minibatch and one 128-row rollout
forward of a nature DualHeadNet at `high` and `medium` (medium takes the table as models.NATURE_SPLIT has it), alternating
likewise.  The last lines compare the measured decision with the table.
usage (GPU box): python tools/nature_split_ab.py [--blocks 9] [--launches 50]"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ppo_amd import _lib, models  # noqa: E402

LAYERS = (("conv1", 4, 84, 32, 8, 4), ("conv2", 32, 20, 64, 4, 2), ("conv3", 64, 9, 64, 3, 1))  # name cin hw cout k stride


def ab(fns, blocks, launches, warmup=10):
    """fns: {name: callable} -> {name: [us per call, one per block]}, the blocks of the variants alternating."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(blocks):
        for name, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(launches):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ts[name].append(e0.elapsed_time(e1) / launches * 1e3)
    return ts


def summary(ts):
    med = {k: statistics.median(v) for k, v in ts.items()}
    spread = max(max(v) - min(v) for v in ts.values())
    return med, spread


def passes(lib, st, n, name, cin, hw, cout, k, stride):
    """{pass: {"exact" | "split": launch}} of one layer on random data (uint8 observations for conv1)."""
    ho = (hw - k) // stride + 1
    geom = (n, cin, hw, hw, cout, k, k, stride)
    g = torch.Generator(device="cuda").manual_seed(n + cin)
    if name == "conv1":
        x, mode = torch.randint(0, 256, (n, cin, hw, hw), dtype=torch.uint8, device="cuda", generator=g), _lib.PPO_IN_U8
    else:
        x, mode = torch.relu(torch.randn(n, cin, hw, hw, device="cuda", generator=g)), _lib.PPO_IN_NONE
    w = torch.randn(cout, cin, k, k, device="cuda", generator=g) / (cin * k * k) ** 0.5
    b = torch.randn(cout, device="cuda", generator=g) * 0.1
    dy = torch.randn(n, cout, ho, ho, device="cuda", generator=g)
    y, dx, dw, db = torch.empty_like(dy), torch.empty(n, cin, hw, hw, device="cuda"), torch.empty_like(w), torch.empty_like(b)
    _lib.check(lib.ppo_conv2d_strided_forward_f32(x.data_ptr(), mode, w.data_ptr(), b.data_ptr(), y.data_ptr(), 1, *geom, st), "gate")
    nbytes = int(lib.ppo_conv2d_strided_wgrad_workspace_bytes(*geom))
    ws = torch.empty(nbytes // 4, device="cuda")
    keep = (x, w, b, dy, y, dx, dw, db, ws)

    def launch(fn, *args):
        def run():
            rc = fn(*args, *geom, st)
            assert rc == 0, lib.ppo_last_error()
        run.keep = keep
        return run
    out = {}
    for tag, suffix in (("exact", "f32"), ("split", "bf16x3")):
        f = {p: getattr(lib, f"ppo_conv2d_strided_{p}_{suffix}") for p in ("forward", "backward_data", "backward_weight")}
        out.setdefault("forward", {})[tag] = launch(f["forward"], x.data_ptr(), mode, w.data_ptr(), b.data_ptr(), y.data_ptr(), 1)
        if name != "conv1":  # nothing back-propagates into the observations
            out.setdefault("backward_data", {})[tag] = launch(f["backward_data"], dy.data_ptr(), y.data_ptr(), w.data_ptr(), dx.data_ptr())
        out.setdefault("backward_weight", {})[tag] = launch(f["backward_weight"], x.data_ptr(), mode, dy.data_ptr(), y.data_ptr(),
                                                            dw.data_ptr(), db.data_ptr(), ws.data_ptr(), nbytes)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=9)
    ap.add_argument("--launches", type=int, default=50)
    a = ap.parse_args()
    _lib.require_gpu()
    lib, st = _lib.load(), _lib.current_stream()
    faster = {}
    print("layer  pass             n    exact us  split us  spread us  exact/split  split faster by more than the spread")
    for n in (128, 256):
        for name, cin, hw, cout, k, stride in LAYERS:
            for conv_pass, fns in passes(lib, st, n, name, cin, hw, cout, k, stride).items():
                med, spread = summary(ab(fns, a.blocks, a.launches))
                yes = med["exact"] - med["split"] > spread
                faster.setdefault((name, conv_pass), []).append(yes)
                print(f"{name}  {conv_pass:<15} {n:4d}  {med['exact']:8.2f}  {med['split']:8.2f}  {spread:9.2f}  "
                      f"{med['exact'] / med['split']:11.2f}  {'yes' if yes else 'no'}")
    measured = frozenset(pair for pair, v in faster.items() if all(v))

    # the whole net: one 256-row policy minibatch and one 128-row rollout forward, high against medium
    nets = {}
    for precision in ("high", "medium"):
        torch.manual_seed(3)
        nets[precision] = models.DualHeadNet("nature", (4, 84, 84), 6, hidden_units=512, head_scale=0.1, head_bias=True,
                                             device="cuda", precision=precision)
    rng = np.random.default_rng(5)
    B, nA = 256, 6
    x = torch.from_numpy(rng.integers(0, 256, size=(B, 4, 84, 84), dtype=np.uint8)).cuda()
    actions = torch.from_numpy(rng.integers(0, nA, size=(B,)).astype(np.int32)).cuda()
    old_lp = torch.log_softmax(torch.from_numpy(rng.normal(size=(B, nA)).astype(np.float32)), dim=1).cuda()
    old_pac = old_lp[torch.arange(B), actions.long()].contiguous()
    adv = torch.from_numpy(rng.normal(size=(B,)).astype(np.float32)).cuda()
    ret = torch.from_numpy(rng.normal(size=(B, 1)).astype(np.float32)).cuda()
    xr = x[:128].contiguous()
    work = {"policy minibatch n=256": lambda net: net.ppo_minibatch(x, actions, old_pac, old_lp, adv, ret),
            "rollout forward n=128": lambda net: net.forward(xr)}
    print(f"\nwhole net, medium with {len(models.NATURE_SPLIT)} split pairs")
    print("what                      high us  medium us  spread us  high/medium")
    for what, fn in work.items():
        fns = {p: (lambda net=net: fn(net)) for p, net in nets.items()}
        med, spread = summary(ab(fns, a.blocks, max(a.launches // 5, 4), warmup=3))
        print(f"{what:<24} {med['high']:8.1f}  {med['medium']:9.1f}  {spread:9.1f}  {med['high'] / med['medium']:11.3f}")

    print("\nmeasured:", sorted(measured))
    print("table   :", sorted(models.NATURE_SPLIT))
    print("NATURE_SPLIT agrees with the measurement" if measured == models.NATURE_SPLIT else
          f"NATURE_SPLIT differs: only measured {sorted(measured - models.NATURE_SPLIT)}, only in the table "
          f"{sorted(models.NATURE_SPLIT - measured)}")


if __name__ == "__main__":
    main()
