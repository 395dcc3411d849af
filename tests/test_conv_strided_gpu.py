"""GPU: the strided-convolution kernels (csrc/conv_strided.hip) against float64 conv2d on the CPU.

Bar: on the same inputs torch's float32 CPU conv2d (and its autograd) is measured against the float64 result; the
kernel's max error may be at most 4 x that one.  Both accumulate in float32 and differ in summation order only.
Every output sits inside a larger buffer filled with a sentinel, which must survive around it; the weight gradient is
launched twice and must give the same bits; an unsupported geometry returns PPO_E_INVALID and launches nothing.

Measured max errors, kernel / torch float32 (MI355X; the table is also in profiles/nature_kernels.md):

    case        forward            backward-data      backward-weight    bias
    conv1_u8    3.320e-07 / 1.631e-06  -                    1.330e-05 / 3.854e-05  8.473e-06 / 2.085e-05
    conv1_f32   5.544e-07 / 2.335e-06  3.678e-07 / 6.704e-07  2.773e-05 / 4.147e-05  8.150e-06 / 1.712e-05
    conv2       4.853e-07 / 1.964e-06  2.974e-07 / 5.024e-07  7.062e-06 / 1.214e-05  2.592e-06 / 2.830e-06
    conv3       6.018e-07 / 1.103e-06  3.511e-07 / 5.264e-07  5.382e-06 / 1.156e-05  1.952e-06 / 2.334e-06
    n1_conv1    2.719e-07 / 7.972e-07  -                    1.964e-06 / 4.351e-06  1.105e-06 / 2.452e-06
    n1_conv2    3.439e-07 / 1.474e-06  1.934e-07 / 4.161e-07  1.136e-06 / 1.136e-06  3.576e-07 / 3.576e-07
    n1_conv3    1.876e-07 / 5.700e-07  6.153e-08 / 8.415e-08  2.384e-07 / 2.384e-07  0.000e+00 / 0.000e+00
    ragged      4.103e-07 / 6.772e-07  1.490e-07 / 1.651e-07  1.145e-06 / 1.145e-06  7.227e-07 / 7.227e-07
    mtail       3.709e-07 / 5.802e-07  2.665e-07 / 5.457e-07  1.855e-06 / 2.681e-06  1.086e-06 / 8.270e-07
    cout1       2.601e-07 / 2.167e-07  4.728e-08 / 4.728e-08  5.500e-07 / 5.500e-07  6.333e-08 / 6.333e-08
"""
import functools

import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
import torch.nn.functional as F  # noqa: E402

from ppo_amd import _lib  # noqa: E402

# name -> (n, cin, h, w, cout, kh, kw, stride, uint8 input)
CASES = {
    # the three Nature layers at their real sizes (84 -> 20 -> 9 -> 7)
    "conv1_u8": (3, 4, 84, 84, 32, 8, 8, 4, True),
    "conv1_f32": (3, 4, 84, 84, 32, 8, 8, 4, False),
    "conv2": (3, 32, 20, 20, 64, 4, 4, 2, False),
    "conv3": (3, 64, 9, 9, 64, 3, 3, 1, False),
    # n = 1 at the fixture geometry 36 -> 8 -> 3 -> 1 (the last one a single GEMM row)
    "n1_conv1": (1, 4, 36, 36, 32, 8, 8, 4, True),
    "n1_conv2": (1, 32, 8, 8, 64, 4, 4, 2, False),
    "n1_conv3": (1, 64, 3, 3, 64, 3, 3, 1, False),
    # (h - kh) % stride = 2, (w - kw) % stride = 1: the last rows / columns of the input are never read
    "ragged": (2, 3, 15, 14, 16, 4, 4, 3, False),
    # n*ho*wo = 60: no multiple of the 64-row tile; 20 output channels: no multiple of 16; a non-square window
    "mtail": (2, 5, 11, 13, 20, 3, 2, 2, False),
    # the smallest supported cout
    "cout1": (2, 2, 9, 9, 1, 3, 3, 2, False),
}
PAD = 4096       # sentinel floats on either side of an output
SENTINEL = -7.25e30
E_INVALID = -1


def _p(t):
    return None if t is None else t.data_ptr()


@functools.lru_cache(maxsize=None)
def reference(name):
    """Inputs and the float64 / float32 CPU results of one case, computed once."""
    n, cin, h, w, cout, kh, kw, stride, u8 = CASES[name]
    g = torch.Generator(device="cpu").manual_seed(sum(map(ord, name)) * 7919)
    if u8:
        raw = torch.randint(0, 256, (n, cin, h, w), generator=g, dtype=torch.uint8)
        x32, x64 = raw.float() / 255.0, raw.double() / 255.0
    else:
        raw = torch.randn(n, cin, h, w, generator=g)
        x32, x64 = raw, raw.double()
    wt = torch.randn(cout, cin, kh, kw, generator=g) / (cin * kh * kw) ** 0.5
    b = torch.randn(cout, generator=g) * 0.1
    ho, wo = (h - kh) // stride + 1, (w - kw) // stride + 1
    dy = torch.randn(n, cout, ho, wo, generator=g)
    pre64 = F.conv2d(x64, wt.double(), b.double(), stride=stride)
    gate = F.relu(pre64).float()          # the post-ReLU map every backward is gated by
    grad = torch.where(gate > 0, dy, torch.zeros_like(dy))
    res = {}
    for tag, (xx, ww, bb, gg) in {"64": (x64, wt.double(), b.double(), grad.double()), "32": (x32, wt, b, grad)}.items():
        xx, ww, bb = xx.clone().requires_grad_(True), ww.clone().requires_grad_(True), bb.clone().requires_grad_(True)
        pre = F.conv2d(xx, ww, bb, stride=stride)
        dx, dw, db = torch.autograd.grad(pre, (xx, ww, bb), gg)
        res[tag] = {"pre": pre.detach(), "relu": F.relu(pre.detach()), "dx": dx, "dw": dw, "db": db}
    return {"raw": raw, "w": wt, "b": b, "dy": dy, "gate": gate, **res}


def guarded(shape, dev):
    """An output of `shape` inside a sentinel-filled buffer: (whole buffer, the output view)."""
    numel = 1
    for s in shape:
        numel *= s
    buf = torch.full((PAD + numel + PAD,), SENTINEL, dtype=torch.float32, device=dev)
    return buf, buf[PAD:PAD + numel].view(shape)


def guards_intact(buf):
    return bool((buf[:PAD] == SENTINEL).all().item()) and bool((buf[-PAD:] == SENTINEL).all().item())


def report(name, op, got, r, key):
    """max error of the kernel and of torch float32, both against float64; asserts the 4 x bar."""
    ref64 = r["64"][key]
    err = (got.detach().cpu().double() - ref64).abs().max().item()
    err32 = (r["32"][key].double() - ref64).abs().max().item()
    print(f"NATURE_ERR {name} {op} kernel={err:.3e} torch_f32={err32:.3e}")
    assert err <= 4.0 * err32, f"{name} {op}: kernel error {err:.3e} > 4 x torch float32's {err32:.3e}"


@pytest.mark.parametrize("name", list(CASES))
def test_against_float64(name):
    n, cin, h, w, cout, kh, kw, stride, u8 = CASES[name]
    lib, dev, st = _lib.load(), torch.device("cuda"), _lib.current_stream()
    assert lib.ppo_conv2d_strided_supported(cin, cout, kh, kw, stride, h, w) == 1
    r = reference(name)
    x, wt, b, dy, gate = (r[k].to(dev) for k in ("raw", "w", "b", "dy", "gate"))
    mode = _lib.PPO_IN_U8 if u8 else _lib.PPO_IN_NONE
    geom = (n, cin, h, w, cout, kh, kw, stride)
    ho, wo = (h - kh) // stride + 1, (w - kw) // stride + 1

    for relu, key in ((1, "relu"), (0, "pre")):
        buf, out = guarded((n, cout, ho, wo), dev)
        _lib.check(lib.ppo_conv2d_strided_forward_f32(_p(x), mode, _p(wt), _p(b), _p(out), relu, *geom, st), "forward")
        assert guards_intact(buf)
        report(name, "forward" if relu else "forward_pre", out, r, key)

    if not u8:
        buf, dx = guarded((n, cin, h, w), dev)
        _lib.check(lib.ppo_conv2d_strided_backward_data_f32(_p(dy), _p(gate), _p(wt), _p(dx), *geom, st), "backward_data")
        assert guards_intact(buf)
        report(name, "backward_data", dx, r, "dx")

    nbytes = int(lib.ppo_conv2d_strided_wgrad_workspace_bytes(*geom))
    assert nbytes > 0
    results = []
    for fill in (float("nan"), 3.0):  # whatever the workspace held must not matter
        ws_buf, ws = guarded((nbytes // 4,), dev)
        ws.fill_(fill)
        wbuf, dw = guarded((cout, cin, kh, kw), dev)
        bbuf, db = guarded((cout,), dev)
        _lib.check(lib.ppo_conv2d_strided_backward_weight_f32(_p(x), mode, _p(dy), _p(gate), _p(dw), _p(db), _p(ws), nbytes,
                                                              *geom, st), "backward_weight")
        assert guards_intact(ws_buf) and guards_intact(wbuf) and guards_intact(bbuf)
        results.append((dw.clone(), db.clone()))
    assert torch.equal(results[0][0], results[1][0]) and torch.equal(results[0][1], results[1][1]), \
        "two weight-gradient launches on the same inputs differ"
    report(name, "backward_weight", results[0][0], r, "dw")
    report(name, "bias", results[0][1], r, "db")


def test_null_gate_and_bias():
    """gate = NULL is the plain convolution gradient, bias = NULL adds nothing, dbias = NULL is skipped."""
    name = "mtail"
    n, cin, h, w, cout, kh, kw, stride, _u8 = CASES[name]
    lib, dev, st = _lib.load(), torch.device("cuda"), _lib.current_stream()
    r = reference(name)
    x, wt, dy = (r[k].to(dev) for k in ("raw", "w", "dy"))
    geom = (n, cin, h, w, cout, kh, kw, stride)
    x64 = r["raw"].double().requires_grad_(True)
    w64 = r["w"].double().requires_grad_(True)
    pre = F.conv2d(x64, w64, None, stride=stride)
    dx64, dw64 = torch.autograd.grad(pre, (x64, w64), r["dy"].double())
    out = torch.empty(pre.shape, dtype=torch.float32, device=dev)
    _lib.check(lib.ppo_conv2d_strided_forward_f32(_p(x), 0, _p(wt), None, _p(out), 0, *geom, st), "forward")
    dx = torch.empty(x.shape, dtype=torch.float32, device=dev)
    _lib.check(lib.ppo_conv2d_strided_backward_data_f32(_p(dy), None, _p(wt), _p(dx), *geom, st), "backward_data")
    nbytes = int(lib.ppo_conv2d_strided_wgrad_workspace_bytes(*geom))
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
    dw = torch.empty(wt.shape, dtype=torch.float32, device=dev)
    _lib.check(lib.ppo_conv2d_strided_backward_weight_f32(_p(x), 0, _p(dy), None, _p(dw), None, _p(ws), nbytes, *geom, st),
               "backward_weight")
    for got, ref in ((out, pre.detach()), (dx, dx64), (dw, dw64)):
        assert (got.cpu().double() - ref).abs().max().item() <= 1e-5 * max(ref.abs().max().item(), 1.0)


@pytest.mark.parametrize("geom", [(2, 4, 7, 84, 32, 8, 8, 4),    # window taller than the image
                                  (2, 4, 84, 84, 32, 8, 8, 0),   # stride 0
                                  (2, 4, 84, 84, 0, 8, 8, 4),    # no output channels
                                  (0, 4, 84, 84, 32, 8, 8, 4)])  # empty batch
def test_unsupported_geometry_is_rejected(geom):
    n, cin, h, w, cout, kh, kw, stride = geom
    lib, dev, st = _lib.load(), torch.device("cuda"), _lib.current_stream()
    if n > 0:
        assert lib.ppo_conv2d_strided_supported(cin, cout, kh, kw, stride, h, w) == 0
    assert int(lib.ppo_conv2d_strided_wgrad_workspace_bytes(*geom)) == 0
    scratch = torch.full((1 << 16,), SENTINEL, dtype=torch.float32, device=dev)
    a, b, c, d, e = (scratch[i * 8192:(i + 1) * 8192] for i in range(5))
    calls = (lambda: lib.ppo_conv2d_strided_forward_f32(_p(a), 0, _p(b), _p(c), _p(d), 1, *geom, st),
             lambda: lib.ppo_conv2d_strided_backward_data_f32(_p(a), _p(b), _p(c), _p(d), *geom, st),
             lambda: lib.ppo_conv2d_strided_backward_weight_f32(_p(a), 0, _p(b), None, _p(c), _p(d), _p(e), 8192 * 4, *geom, st))
    for call in calls:
        assert call() == E_INVALID
        assert lib.ppo_last_error()
    torch.cuda.synchronize()
    assert bool((scratch == SENTINEL).all().item()), "a rejected call wrote something"


def test_small_workspace_and_bad_mode_are_rejected():
    n, cin, h, w, cout, kh, kw, stride, _u8 = CASES["cout1"]
    geom = (n, cin, h, w, cout, kh, kw, stride)
    lib, dev, st = _lib.load(), torch.device("cuda"), _lib.current_stream()
    r = reference("cout1")
    x, wt, dy = (r[k].to(dev) for k in ("raw", "w", "dy"))
    nbytes = int(lib.ppo_conv2d_strided_wgrad_workspace_bytes(*geom))
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
    dw = torch.full(wt.shape, SENTINEL, dtype=torch.float32, device=dev)
    assert lib.ppo_conv2d_strided_backward_weight_f32(_p(x), 0, _p(dy), None, _p(dw), None, _p(ws), nbytes - 4, *geom, st) == E_INVALID
    assert lib.ppo_conv2d_strided_backward_weight_f32(_p(x), _lib.PPO_IN_RELU, _p(dy), None, _p(dw), None, _p(ws), nbytes, *geom,
                                                      st) == E_INVALID
    out = torch.full(dy.shape, SENTINEL, dtype=torch.float32, device=dev)
    assert lib.ppo_conv2d_strided_forward_f32(_p(x), _lib.PPO_IN_RELU, _p(wt), None, _p(out), 0, *geom, st) == E_INVALID
    torch.cuda.synchronize()
    assert bool((dw == SENTINEL).all().item()) and bool((out == SENTINEL).all().item())
