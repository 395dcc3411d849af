"""The specialised first-layer launches under --observation_scaling: what the signed uint8 input modes (PPO_IN_U8_CENTERED,
PPO_IN_U8_UNIT) cost against PPO_IN_U8.

Four launches of the first IMPALA layer on uint8 observations - the forward (ppo_conv3x3_forward_packed_f32), the fused
conv + max-pool with its argmax (ppo_conv3x3_pool_forward_packed_f32), the same through a row index
(ppo_conv3x3_pool_forward_packed_indexed_f32, the training minibatch) and the weight gradient
(ppo_conv3x3_backward_weight_f32) - at n = 128 (a rollout group) and n = 256 (a minibatch).  The three modes alternate in
one process in blocks of launches timed by HIP events, after warm-up; printed per launch are the median over blocks of
each mode, the block-to-block spread (the largest max - min over blocks of the three) and whether a signed mode's median
lies above PPO_IN_U8's by more than that spread.  The table is markdown (profiles/obs_scaling.md).
usage (GPU box): python tools/obs_scaling_ab.py [--geometry 4x84] [--blocks 9] [--launches 50]"""
import argparse
import ctypes
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ppo_amd import _lib  # noqa: E402

MODES = {"scaled": _lib.PPO_IN_U8, "centered": _lib.PPO_IN_U8_CENTERED, "unit": _lib.PPO_IN_U8_UNIT}
GEOMETRIES = {"4x84": (4, 84), "5x84": (5, 84), "3x64": (3, 64), "4x64": (4, 64)}


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


def launches_of(lib, st, n, cin, side):
    """{launch name: {mode name: callable}} on random bytes."""
    cout, ho = 16, side // 2
    g = torch.Generator(device="cuda").manual_seed(n + cin + side)
    x = torch.randint(0, 256, (n, cin, side, side), dtype=torch.uint8, device="cuda", generator=g)
    w = torch.randn(cout, cin, 3, 3, device="cuda", generator=g) / (9 * cin) ** 0.5
    b = torch.randn(cout, device="cuda", generator=g) * 0.1
    dy = torch.randn(n, cout, side, side, device="cuda", generator=g)
    index = torch.randperm(n, device="cuda", generator=g).to(torch.int32)
    packed = torch.empty(lib.ppo_conv3x3_packed_floats(cin, cout, 0), device="cuda")
    jobs = (_lib.PackJob * 1)(_lib.PackJob(w.data_ptr(), packed.data_ptr(), cin, cout, 0))
    _lib.check(lib.ppo_conv3x3_pack_weights_f32(ctypes.addressof(jobs), 1, st), "pack")
    y = torch.empty(n, cout, side, side, device="cuda")
    p = torch.empty(n, cout, ho, ho, device="cuda")
    amx = torch.empty(n, cout, ho, ho, dtype=torch.uint8, device="cuda")
    dw, db = torch.empty_like(w), torch.empty_like(b)
    nbytes = int(lib.ppo_conv3x3_wgrad_workspace_bytes(cin, cout))
    ws = torch.empty(nbytes // 4, device="cuda")
    keep = (x, w, b, dy, index, packed, y, p, amx, dw, db, ws)
    geo = (n, cin, cout, side, side)

    def launch(fn, *args):
        def run():
            rc = fn(*args, st)
            assert rc == 0, lib.ppo_last_error()
        run.keep = keep
        return run
    out = {}
    for name, mode in MODES.items():
        out.setdefault("forward", {})[name] = launch(lib.ppo_conv3x3_forward_packed_f32, x.data_ptr(), mode, packed.data_ptr(),
                                                     b.data_ptr(), None, y.data_ptr(), *geo)
        out.setdefault("conv + pool", {})[name] = launch(lib.ppo_conv3x3_pool_forward_packed_f32, x.data_ptr(), mode,
                                                         packed.data_ptr(), b.data_ptr(), p.data_ptr(), amx.data_ptr(), *geo)
        out.setdefault("conv + pool, indexed", {})[name] = launch(lib.ppo_conv3x3_pool_forward_packed_indexed_f32, x.data_ptr(),
                                                                  index.data_ptr(), mode, packed.data_ptr(), b.data_ptr(),
                                                                  p.data_ptr(), amx.data_ptr(), *geo)
        out.setdefault("weight gradient", {})[name] = launch(lib.ppo_conv3x3_backward_weight_f32, x.data_ptr(), mode, dy.data_ptr(),
                                                             dw.data_ptr(), db.data_ptr(), ws.data_ptr(), nbytes, *geo, 0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--geometry", choices=sorted(GEOMETRIES), default="4x84")
    ap.add_argument("--blocks", type=int, default=9)
    ap.add_argument("--launches", type=int, default=50)
    a = ap.parse_args()
    _lib.require_gpu()
    lib, st = _lib.load(), _lib.current_stream()
    cin, side = GEOMETRIES[a.geometry]
    print(f"first layer {cin} -> 16 on {side} x {side}, {a.blocks} blocks of {a.launches} launches per mode, on "
          f"{torch.cuda.get_device_name(0)}\n")
    print("| launch | n | scaled us | centered us | unit us | spread us | centered / scaled | unit / scaled | outside the spread |")
    print("|---|---|---|---|---|---|---|---|---|")
    for n in (128, 256):
        for what, fns in launches_of(lib, st, n, cin, side).items():
            ts = ab(fns, a.blocks, a.launches)
            med = {k: statistics.median(v) for k, v in ts.items()}
            spread = max(max(v) - min(v) for v in ts.values())
            outside = [k for k in ("centered", "unit") if med[k] - med["scaled"] > spread]
            print(f"| {what} | {n} | {med['scaled']:.2f} | {med['centered']:.2f} | {med['unit']:.2f} | {spread:.2f} | "
                  f"{med['centered'] / med['scaled']:.3f} | {med['unit'] / med['scaled']:.3f} | {', '.join(outside) or 'none'} |")


if __name__ == "__main__":
    main()
