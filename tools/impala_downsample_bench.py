"""Times the generic stride-2 3x3 convolution entry points (ppo_conv3x3s2_any_*, csrc/conv3x3_any.hip) at the two
stack-first geometries of the 84x84 net, beside what the same stack costs under down_sample='pool' on the generic
stride-1 kernels: ppo_conv3x3_any_* plus the max-pool launch of the same pass.  For orientation only - neither family is
tuned.  Prints the table of DESIGN.md's down_sample entry.

    python tools/impala_downsample_bench.py [--batch 256] [--out FILE]

Method: that of tools/impala_any_bench.py (three warm launches, then windows of back-to-back launches bracketed by HIP
events, at least 0.1 s and 10 launches each; the two sides alternate, three windows of each, the median is reported)."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from impala_any_bench import MODE, NONE, U8, _p, measure  # noqa: E402
from ppo_amd import _lib  # noqa: E402

# (cin, cout, h, w, in_mode, has a data gradient)
LAYERS = [(4, 16, 84, 84, U8, False), (16, 32, 42, 42, NONE, True)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    _lib.require_gpu()
    lib, dev, B = _lib.load(), torch.device("cuda"), a.batch
    lines = [f"Device: {torch.cuda.get_device_name(0)}; batch {B}; microseconds per launch (median of three windows).",
             "`stride 2`: one ppo_conv3x3s2_any_* launch.  `stride 1 + pool`: the ppo_conv3x3_any_* launch of the same pass and",
             "the max-pool launch that goes with it (forward: pool forward; backward: pool backward, charged to the weight",
             "gradient, which is the pass that cannot run without it).", "",
             "| geometry | pass | stride 2 us | stride 1 any us | pool us | stride 1 + pool us |", "|---|---|---|---|---|---|"]
    g = torch.Generator(device="cpu").manual_seed(1)
    for cin, cout, h, w, mode, data_grad in LAYERS:
        ho, wo = (h + 1) // 2, (w + 1) // 2
        dims = (B, cin, cout, h, w)
        x = (torch.randint(0, 256, (B, cin, h, w), generator=g, dtype=torch.uint8) if mode == U8
             else torch.randn(B, cin, h, w, generator=g)).to(dev)
        wt = (torch.randn(cout, cin, 3, 3, generator=g) / (9 * cin) ** 0.5).to(dev)
        b = torch.randn(cout, generator=g).to(dev)
        dy1, dy2 = torch.randn(B, cout, h, w, generator=g).to(dev), torch.randn(B, cout, ho, wo, generator=g).to(dev)
        y1, y2 = torch.empty_like(dy1), torch.empty_like(dy2)
        idx = torch.empty(B, cout, ho, wo, dtype=torch.uint8, device=dev)
        dx = torch.empty(B, cin, h, w, device=dev)
        dw, db = torch.empty_like(wt), torch.empty_like(b)
        nb1 = int(lib.ppo_conv3x3_any_wgrad_workspace_bytes(*dims))
        nb2 = int(lib.ppo_conv3x3s2_any_wgrad_workspace_bytes(*dims))
        ws1, ws2 = torch.empty(nb1 // 4, device=dev), torch.empty(nb2 // 4, device=dev)
        _lib.check(lib.ppo_conv3x3_any_forward_f32(_p(x), mode, _p(wt), _p(b), None, _p(y1), *dims, _lib.current_stream()), "forward")
        _lib.check(lib.ppo_maxpool3x3s2_forward_f32(_p(y1), _p(y2), _p(idx), B, cout, h, w, _lib.current_stream()), "pool")
        passes = [
            ("forward",
             lambda st: lib.ppo_conv3x3s2_any_forward_f32(_p(x), mode, _p(wt), _p(b), None, _p(y2), *dims, st),
             lambda st: lib.ppo_conv3x3_any_forward_f32(_p(x), mode, _p(wt), _p(b), None, _p(y1), *dims, st),
             lambda st: lib.ppo_maxpool3x3s2_forward_f32(_p(y1), _p(y2), _p(idx), B, cout, h, w, st)),
            ("backward-weight",
             lambda st: lib.ppo_conv3x3s2_any_backward_weight_f32(_p(x), mode, _p(dy2), _p(dw), _p(db), _p(ws2), nb2, *dims, 0, st),
             lambda st: lib.ppo_conv3x3_any_backward_weight_f32(_p(x), mode, _p(dy1), _p(dw), _p(db), _p(ws1), nb1, *dims, 0, st),
             lambda st: lib.ppo_maxpool3x3s2_backward_f32(_p(dy2), _p(idx), _p(dy1), B, cout, h, w, st))]
        if data_grad:
            passes.append((
                "backward-data",
                lambda st: lib.ppo_conv3x3s2_any_backward_data_f32(_p(dy2), _p(wt), None, None, _p(dx), *dims, st),
                lambda st: lib.ppo_conv3x3_any_backward_data_f32(_p(dy1), _p(wt), None, None, _p(dx), *dims, st), None))
        for name, s2, s1, pool in passes:
            t2, t1, tp = measure([s2, s1, pool])
            lines.append(f"| {cin}->{cout} @ {h}x{w} ({MODE[mode]}) | {name} | {t2 * 1e6:.1f} | {t1 * 1e6:.1f} | "
                         + (f"{tp * 1e6:.1f} | {(t1 + tp) * 1e6:.1f} |" if tp else f"- | {t1 * 1e6:.1f} |"))
            print(lines[-1], flush=True)
    text = "\n".join(lines)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
