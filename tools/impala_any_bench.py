"""Times the generic 3x3 convolution entry points (csrc/conv3x3_any.hip) layer by layer, beside the specialised kernels
where those exist, and prints the table of profiles/impala_any.md.

    python tools/impala_any_bench.py [--batch 256] [--out FILE]

Method: per entry point and layer, three warm launches, then windows of back-to-back launches on one stream bracketed by
HIP events (each window at least 0.1 s of work, at least 10 launches); generic and specialised windows alternate, three
of each, and the median window's time per launch is reported.  FLOPs are the algorithm's: 2 * 9 * cin * cout * h * w per
image for each of the three passes; the share of peak is against the 157.3 TFLOP/s f32 MFMA peak."""
import argparse
import hashlib
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ppo_amd import _lib  # noqa: E402

PEAK = 157.3e12
NONE, RELU, U8 = _lib.PPO_IN_NONE, _lib.PPO_IN_RELU, _lib.PPO_IN_U8
MODE = {NONE: "none", RELU: "relu", U8: "u8"}
# (label, cin, cout, h, w, in_mode, has a data gradient)
NETS = {
    "4x96x96 net (no specialised kernel)": [
        ("stack0.firstconv", 4, 16, 96, 96, U8, False), ("stack0.blocks", 16, 16, 48, 48, RELU, True),
        ("stack1.firstconv", 16, 32, 48, 48, NONE, True), ("stack1.blocks", 32, 32, 24, 24, RELU, True),
        ("stack2.firstconv", 32, 32, 24, 24, NONE, True), ("stack2.blocks", 32, 32, 12, 12, RELU, True)],
    "4x84x84 net (the specialised geometries)": [
        ("stack0.firstconv", 4, 16, 84, 84, U8, False), ("stack0.blocks", 16, 16, 42, 42, RELU, True),
        ("stack1.firstconv", 16, 32, 42, 42, NONE, True), ("stack1.blocks", 32, 32, 21, 21, RELU, True),
        ("stack2.firstconv", 32, 32, 21, 21, NONE, True), ("stack2.blocks", 32, 32, 11, 11, RELU, True)],
}


def _p(t):
    return None if t is None else t.data_ptr()


def window(launch, reps):
    st = _lib.current_stream()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        rc = launch(st)
        if rc != 0:
            _lib.check(rc, "launch")
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / reps


def measure(launches):
    """launches: the generic launch and, or None, the specialised one -> seconds per launch of each (median of 3 windows)."""
    reps = []
    for fn in launches:
        if fn is None:
            reps.append(0)
            continue
        for _ in range(3):
            window(fn, 1)
        t = window(fn, 3)
        reps.append(max(10, min(2000, int(0.1 / max(t, 1e-7)))))
    times = [[] for _ in launches]
    for _ in range(3):
        for k, fn in enumerate(launches):
            if fn is not None:
                times[k].append(window(fn, reps[k]))
    return [statistics.median(t) if t else None for t in times]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    _lib.require_gpu()
    lib, dev, B = _lib.load(), torch.device("cuda"), a.batch
    src = b"".join(open(os.path.join(ROOT, "ppo_amd", "csrc", f), "rb").read()
                   for f in ("conv3x3_any.hip", "conv3x3_any_index.h", "conv_gemm_tile.h"))
    lines = [f"Kernel sources (sha256 of conv3x3_any.hip + conv3x3_any_index.h + conv_gemm_tile.h): `{hashlib.sha256(src).hexdigest()[:16]}`",
             f"Device: {torch.cuda.get_device_name(0)}; batch {B}; times in microseconds per launch; `share` = algorithmic FLOPs / time / 157.3 TFLOP/s;",
             "`x spec` = generic time / specialised time (raw-weight entry points, same process, alternating windows).", ""]
    g = torch.Generator(device="cpu").manual_seed(1)
    for title, layers in NETS.items():
        lines += [f"### {title}", "", "| layer | geometry | pass | generic us | share | specialised us | x spec |", "|---|---|---|---|---|---|---|"]
        for label, cin, cout, h, w, mode, data_grad in layers:
            dims = (B, cin, cout, h, w)
            x = (torch.randint(0, 256, (B, cin, h, w), generator=g, dtype=torch.uint8) if mode == U8
                 else torch.randn(B, cin, h, w, generator=g)).to(dev)
            wt = (torch.randn(cout, cin, 3, 3, generator=g) / (9 * cin) ** 0.5).to(dev)
            b = torch.randn(cout, generator=g).to(dev)
            dy = torch.randn(B, cout, h, w, generator=g).to(dev)
            res = torch.randn(B, cout, h, w, generator=g).to(dev) if mode == RELU else None
            y, dx = torch.empty_like(dy), torch.empty(B, cin, h, w, device=dev)
            dw, db = torch.empty_like(wt), torch.empty_like(b)
            nb_any = int(lib.ppo_conv3x3_any_wgrad_workspace_bytes(*dims))
            nb_spec = int(lib.ppo_conv3x3_wgrad_workspace_bytes(cin, cout))
            ws_any, ws_spec = torch.empty(nb_any // 4, device=dev), torch.empty(nb_spec // 4, device=dev)
            gate = x if mode == RELU else None
            passes = [
                ("forward",
                 lambda st: lib.ppo_conv3x3_any_forward_f32(_p(x), mode, _p(wt), _p(b), _p(res), _p(y), *dims, st),
                 (lambda st: lib.ppo_conv3x3_forward_f32(_p(x), mode, _p(wt), _p(b), _p(res), _p(y), *dims, st))
                 if lib.ppo_conv3x3_forward_supported(mode, cin, cout, h, w) else None),
                ("backward-weight",
                 lambda st: lib.ppo_conv3x3_any_backward_weight_f32(_p(x), mode, _p(dy), _p(dw), _p(db), _p(ws_any), nb_any, *dims, 0, st),
                 (lambda st: lib.ppo_conv3x3_backward_weight_f32(_p(x), mode, _p(dy), _p(dw), _p(db), _p(ws_spec), nb_spec, *dims, 0, st))
                 if lib.ppo_conv3x3_backward_weight_supported(mode, cin, cout, h, w) else None)]
            if data_grad:
                passes.insert(1, (
                    "backward-data",
                    lambda st: lib.ppo_conv3x3_any_backward_data_f32(_p(dy), _p(wt), _p(gate), None, _p(dx), *dims, st),
                    (lambda st: lib.ppo_conv3x3_backward_data_f32(_p(dy), _p(wt), _p(gate), None, _p(dx), *dims, st))
                    if lib.ppo_conv3x3_backward_data_supported(cin, cout, h, w) else None))
            flops = 2.0 * 9 * cin * cout * h * w * B
            for name, generic, special in passes:
                tg, ts = measure([generic, special])
                lines.append(f"| {label} | {cin}->{cout} @ {h}x{w} ({MODE[mode]}) | {name} | {tg * 1e6:.1f} | {flops / tg / PEAK:.3f} | "
                             + (f"{ts * 1e6:.1f} | {tg / ts:.1f} |" if ts else "- | - |"))
                print(lines[-1], flush=True)
        lines.append("")
    text = "\n".join(lines)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
