"""GPU: the kernels Random Network Distillation adds - the leaky-ReLU forms of the strided convolutions, the one-channel
observation normalise, the prediction error / gradient / statistics launch and the two batch ops of the intrinsic-reward
normalisation.

Convolutions: against torch.nn.functional (conv2d + leaky_relu and their autograd, float64) on the same device, at the
project's per-kernel bar of 1e-4 of the tensor's max; bit-exact on integer-valued data, where every product and sum is
exact in float32 (slope 1.0 or a power of two); a gate of exactly 0 takes the slope branch, as torch's leaky_relu
backward does.  The backward launches are gated by the float64 result rounded to float32, so a pre-activation within
rounding of zero cannot put kernel and reference on different branches."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
import torch.nn.functional as F  # noqa: E402

from ppo_amd import _lib  # noqa: E402

# the three layers of the RND networks (rl/models.py:228-230) on one 36x36 channel (36 -> 8 -> 3 -> 1) and on 84x84
LAYERS36 = {"conv1": (1, 36, 36, 32, 8, 4), "conv2": (32, 8, 8, 64, 4, 2), "conv3": (64, 3, 3, 64, 3, 1)}
LAYERS84 = {"conv1": (1, 84, 84, 32, 8, 4), "conv2": (32, 20, 20, 64, 4, 2), "conv3": (64, 9, 9, 64, 3, 1)}
CASES = [(n, name, geo) for n in (1, 5, 8) for name, geo in LAYERS36.items()] + [(3, name, geo) for name, geo in LAYERS84.items()]
DEV = "cuda"


def _p(t):
    return None if t is None else t.data_ptr()


def conv_reference(x, w, b, dy, stride, slope, gate=None):
    """float64 on the device: the activation and the three gradients.  With `gate`, the activation's derivative is taken at
    the gate's values instead (what the backward launches are given)."""
    x, w, b = (t.double().clone().requires_grad_(True) for t in (x, w, b))
    pre = F.conv2d(x, w, b, stride=stride)
    act = F.leaky_relu(pre, slope)
    if gate is None:
        g = torch.autograd.grad(act, pre, dy.double(), retain_graph=True)[0]
    else:
        z = gate.double().clone().requires_grad_(True)
        g = torch.autograd.grad(F.leaky_relu(z, slope), z, dy.double())[0]
    dx, dw, db = torch.autograd.grad(pre, (x, w, b), g)
    return act.detach(), dx, dw, db


def run_kernels(x, w, b, dy, gate, stride, slope):
    lib, st = _lib.load(), _lib.current_stream()
    n, cin, h, wd = x.shape
    cout, _ci, kh, kw = w.shape
    geom = (n, cin, h, wd, cout, kh, kw, stride)
    out = torch.empty_like(dy)
    _lib.check(lib.ppo_conv2d_strided_forward_leaky_f32(_p(x), 0, _p(w), _p(b), _p(out), slope, *geom, st), "forward")
    dx = torch.empty_like(x)
    _lib.check(lib.ppo_conv2d_strided_backward_data_leaky_f32(_p(dy), _p(gate), _p(w), _p(dx), slope, *geom, st), "bwd data")
    nbytes = int(lib.ppo_conv2d_strided_wgrad_workspace_bytes(*geom))
    ws = torch.full((nbytes // 4,), float("nan"), device=DEV)
    dw, db = torch.empty_like(w), torch.empty_like(b)
    _lib.check(lib.ppo_conv2d_strided_backward_weight_leaky_f32(_p(x), 0, _p(dy), _p(gate), _p(dw), _p(db), _p(ws), nbytes, slope,
                                                                *geom, st), "bwd weight")
    torch.cuda.synchronize()
    return out, dx, dw, db


def rel(a, ref):
    return (a.double() - ref).abs().max().item() / max(ref.abs().max().item(), 1e-30)


@pytest.mark.parametrize("slope", [0.2, 1.0])
@pytest.mark.parametrize("n,name,geo", CASES, ids=[f"n{n}_{name}_{geo[1]}" for n, name, geo in CASES])
def test_leaky_convolutions_against_torch(n, name, geo, slope):
    cin, h, wd, cout, k, s = geo
    g = torch.Generator(device="cpu").manual_seed(1000 * n + h + len(name))
    x = torch.randn(n, cin, h, wd, generator=g).to(DEV)
    w = (torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5).to(DEV)
    b = (torch.randn(cout, generator=g) * 0.1).to(DEV)
    dy = torch.randn(n, cout, (h - k) // s + 1, (wd - k) // s + 1, generator=g).to(DEV)
    act, dx64, dw64, db64 = conv_reference(x, w, b, dy, s, slope)
    out, dx, dw, db = run_kernels(x, w, b, dy, act.float().contiguous(), s, slope)
    for what, got, ref in (("forward", out, act), ("backward_data", dx, dx64), ("backward_weight", dw, dw64), ("bias", db, db64)):
        e = rel(got, ref)
        print(f"LEAKY_ERR n={n} {name}@{h} slope={slope} {what} rel_err={e:.3e}")
        assert e <= 1e-4, (what, e)


@pytest.mark.parametrize("slope", [1.0, 0.25])
@pytest.mark.parametrize("name", list(LAYERS36))
def test_leaky_convolutions_exact_on_integers(name, slope):
    cin, h, wd, cout, k, s = LAYERS36[name]
    n = 5
    g = torch.Generator(device="cpu").manual_seed(77 + h)
    x = torch.randint(-3, 4, (n, cin, h, wd), generator=g).float().to(DEV)
    w = torch.randint(-2, 3, (cout, cin, k, k), generator=g).float().to(DEV)
    b = torch.randint(-2, 3, (cout,), generator=g).float().to(DEV)
    dy = torch.randint(-3, 4, (n, cout, (h - k) // s + 1, (wd - k) // s + 1), generator=g).float().to(DEV)
    act, dx64, dw64, db64 = conv_reference(x, w, b, dy, s, slope)
    if name == "conv1":
        assert (act == 0).any(), "integer data should put some pre-activations exactly at 0"
    out, dx, dw, db = run_kernels(x, w, b, dy, act.float().contiguous(), s, slope)
    # act == 0 exactly where the pre-activation is 0: the reference's derivative there is `slope`, and so is the kernels'
    for what, got, ref in (("forward", out, act), ("backward_data", dx, dx64), ("backward_weight", dw, dw64), ("bias", db, db64)):
        assert torch.equal(got.double(), ref), what


def test_zero_gate_takes_the_slope_branch():
    cin, h, wd, cout, k, s = LAYERS36["conv2"]
    n, slope = 5, 0.2
    g = torch.Generator(device="cpu").manual_seed(5)
    x = torch.randn(n, cin, h, wd, generator=g).to(DEV)
    w = torch.randn(cout, cin, k, k, generator=g).to(DEV) / 16
    b = torch.zeros(cout, device=DEV)
    dy = torch.randn(n, cout, 3, 3, generator=g).to(DEV)
    gate = torch.randn(n, cout, 3, 3, generator=g).to(DEV)
    gate[:, ::2] = 0.0          # half the channels: exactly zero (and -0.0 in one of them)
    gate[:, 2] = -0.0
    _act, dx64, dw64, db64 = conv_reference(x, w, b, dy, s, slope, gate=gate)
    _out, dx, dw, db = run_kernels(x, w, b, dy, gate, s, slope)
    assert rel(dx, dx64) <= 1e-4 and rel(dw, dw64) <= 1e-4 and rel(db, db64) <= 1e-4
    # the bias gradient isolates the branch: sum over (n, y, x) of dy * slope in the zeroed channels
    want = (dy.double() * slope).sum(dim=(0, 2, 3))[::2]
    assert (db.double()[::2] - want).abs().max().item() <= 1e-5 * want.abs().max().item()


def test_leaky_entry_points_reject_bad_arguments():
    lib, st = _lib.load(), _lib.current_stream()
    buf = torch.full((1 << 15,), -7.25e30, device=DEV)
    a, b, c, d, e = (buf[i * 4096:(i + 1) * 4096] for i in range(5))
    geom = (1, 1, 36, 36, 32, 8, 8, 4)
    for slope in (0.0, -0.2, 1.5, float("nan")):
        assert lib.ppo_conv2d_strided_forward_leaky_f32(_p(a), 0, _p(b), _p(c), _p(d), slope, *geom, st) == -1
        assert lib.ppo_conv2d_strided_backward_data_leaky_f32(_p(a), _p(b), _p(c), _p(d), slope, *geom, st) == -1
        assert lib.ppo_conv2d_strided_backward_weight_leaky_f32(_p(a), 0, _p(b), None, _p(c), _p(d), _p(e), 4096 * 4, slope,
                                                                *geom, st) == -1
    bad = (1, 1, 7, 36, 32, 8, 8, 4)  # window taller than the image
    assert lib.ppo_conv2d_strided_forward_leaky_f32(_p(a), 0, _p(b), _p(c), _p(d), 0.2, *bad, st) == -1
    torch.cuda.synchronize()
    assert bool((buf == -7.25e30).all().item()), "a rejected call wrote something"


# ---------------------------------------------------------------------------------------------- one-channel normalise
@pytest.mark.parametrize("hw", [(36, 36), (7, 9)])   # H*W a multiple of 4 (16-byte path) and not
@pytest.mark.parametrize("u8", [True, False])
@pytest.mark.parametrize("indexed", [False, True])
def test_channel_normalise_bit_equals_the_full_one(hw, u8, indexed):
    lib, st = _lib.load(), _lib.current_stream()
    rows, C, (H, W) = 9, 4, hw
    g = torch.Generator(device="cpu").manual_seed(H)
    x = (torch.randint(0, 256, (rows, C, H, W), generator=g, dtype=torch.uint8) if u8
         else torch.randn(rows, C, H, W, generator=g) * 3).to(DEV)   # * 3: some values reach the clamp
    mu = (torch.rand(C * H * W, generator=g) * (0.5 if u8 else 1.0)).to(DEV)
    std = (torch.rand(C * H * W, generator=g) * 0.3 + 0.02).to(DEV)
    eps = 1e-5
    index = torch.tensor([8, 2, 2, 0, 5], dtype=torch.int32, device=DEV) if indexed else None   # a repeat, the last row
    src = x[index.long()].contiguous() if indexed else x
    B = src.shape[0]
    full = torch.empty(B, C, H, W, device=DEV)
    _lib.check(lib.ppo_obs_normalize_f32(_p(src), int(u8), _p(mu), _p(std), eps, _p(full), B, C * H * W, st), "normalize")
    buf = torch.full((4096 + B * H * W + 4096,), -7.25e30, device=DEV)
    out = buf[4096:4096 + B * H * W].view(B, 1, H, W)
    _lib.check(lib.ppo_obs_normalize_channel_f32(_p(x), int(u8), _p(index), _p(mu), _p(std), eps, _p(out), B, C, H, W, C - 1, st),
               "normalize channel")
    torch.cuda.synchronize()
    assert torch.equal(out[:, 0], full[:, C - 1])
    assert float(out.abs().max()) == 5.0 or u8
    assert bool((buf[:4096] == -7.25e30).all()) and bool((buf[-4096:] == -7.25e30).all())
    # and another channel
    _lib.check(lib.ppo_obs_normalize_channel_f32(_p(x), int(u8), _p(index), _p(mu), _p(std), eps, _p(out), B, C, H, W, 1, st),
               "normalize channel")
    assert torch.equal(out[:, 0], full[:, 1])
    assert lib.ppo_obs_normalize_channel_f32(_p(x), int(u8), None, _p(mu), _p(std), eps, _p(out), B, C, H, W, C, st) == -1


# ---------------------------------------------------------------------------------------------- prediction error
@functools.lru_cache(maxsize=None)
def error_inputs(B, Fw):
    g = torch.Generator(device="cpu").manual_seed(B * 1000 + Fw)
    return torch.randn(B, Fw, generator=g), torch.randn(B, Fw, generator=g) * 0.7


@pytest.mark.parametrize("B,Fw", [(1, 512), (5, 512), (8, 512), (131, 512), (8, 24)])
def test_rnd_error_against_float64(B, Fw):
    lib, st = _lib.load(), _lib.current_stream()
    pred_c, target_c = error_inputs(B, Fw)
    pred, target = pred_c.to(DEV), target_c.to(DEV)
    p64, t64 = pred_c.double(), target_c.double()
    err64 = ((t64 - p64) ** 2).mean(dim=1)
    scale, stride = 0.37 / B, 3
    d64 = scale * 2.0 * (p64 - t64) / Fw
    canary = 123.25
    results = []
    for _ in range(2):
        err = torch.full((B, stride), canary, device=DEV)
        dpred = torch.full((B, Fw), canary, device=DEV)
        stats = torch.tensor([1.0, 2.0, 3.0, 0.5, 4.0], device=DEV)   # the launch adds to what is there
        _lib.check(lib.ppo_rnd_error_f32(_p(pred), _p(target), B, Fw, _p(err), stride, _p(dpred), scale, _p(stats), st), "error")
        torch.cuda.synchronize()
        results.append((err.clone(), dpred.clone(), stats.clone()))
    (err, dpred, stats), again = results
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(results[0], again)), \
        "two launches on the same inputs differ"   # as bit patterns: the variance of one row is NaN
    assert bool((err[:, 1:] == canary).all()), "cells between the strided elements were written"
    e = ((err[:, 0].cpu().double() - err64).abs() / err64).max().item()
    d = (dpred.cpu().double() - d64).abs().max().item() / d64.abs().max().item()
    print(f"RND_ERR B={B} F={Fw} err_rel={e:.3e} dpred_rel={d:.3e}")
    assert e <= 1e-6 and d <= 1e-6
    s = stats.cpu().double()
    want = [1.0 + err64.sum().item(), 2.0 + t64.mean().item(), 3.0 + (t64.var(dim=0).mean().item() if B > 1 else float("nan")),
            max(0.5, t64.abs().max().item()), 5.0]
    for i, wv in enumerate(want):
        if wv != wv:
            assert s[i] != s[i], "torch.var of one row is NaN"
        else:
            assert abs(s[i].item() - wv) <= 2e-6 * max(1.0, abs(wv)), (i, s[i].item(), wv)
    # the rollout's form: err only, unit stride, nothing else written
    err1 = torch.full((B + 2,), canary, device=DEV)
    _lib.check(lib.ppo_rnd_error_f32(_p(pred), _p(target), B, Fw, _p(err1), 1, None, 0.0, None, st), "error")
    torch.cuda.synchronize()
    assert torch.equal(err1[:B], err[:, 0]) and bool((err1[B:] == canary).all())


def test_rnd_error_rejects_bad_arguments():
    lib, st = _lib.load(), _lib.current_stream()
    a = torch.zeros(64, device=DEV)
    assert lib.ppo_rnd_error_f32(_p(a), _p(a), 0, 8, _p(a), 1, None, 0.0, None, st) == -1
    assert lib.ppo_rnd_error_f32(_p(a), _p(a), 2, 8, _p(a), 0, None, 0.0, None, st) == -1
    assert lib.ppo_rnd_error_f32(_p(a), None, 2, 8, _p(a), 1, None, 0.0, None, st) == -1
    assert lib.ppo_rnd_error_f32(_p(a), _p(a), 2, 8, None, 1, None, 0.0, None, st) == -1


# ---------------------------------------------------------------------------------------------- intrinsic-reward batch ops
@pytest.mark.parametrize("center", [False, True])
def test_scale_shift_clip_is_the_references_normalisation(center):
    """np.clip(r, -5, 5) / scale (a float64 division: the scale is a NumPy float64 scalar) [- mean], rl/rollout.py:929,
    1165, 1168; the mean comes from ppo_moments_f64 of the divided rewards, as Runner.calculate_returns will take it."""
    lib, st = _lib.load(), _lib.current_stream()
    rng = np.random.default_rng(3)
    r = rng.normal(size=(6, 5)).astype(np.float32) * 2
    r[2, 3], r[4, 0] = 7.0, -9.5   # beyond the clip
    scale = np.float64(0.8371) ** 0.5 + 1e-5
    want = np.clip(r, -5, 5).astype(np.float64) / scale
    x = torch.from_numpy(r).to(DEV)
    out = torch.empty_like(x)
    _lib.check(lib.ppo_scale_shift_clip_f32(_p(x), x.numel(), 5.0, float(scale), None, _p(out), st), "scale")
    assert np.array_equal(out.cpu().numpy(), want.astype(np.float32))
    assert out[2, 3].item() == np.float32(5.0 / scale) and out[4, 0].item() == np.float32(-5.0 / scale)
    if center:
        moments = torch.empty(3, dtype=torch.float64, device=DEV)
        ws = torch.empty(int(lib.ppo_moments_workspace_bytes()) // 8, dtype=torch.float64, device=DEV)
        _lib.check(lib.ppo_moments_f64(_p(out), out.numel(), _p(moments), _p(ws), st), "moments")
        _lib.check(lib.ppo_scale_shift_clip_f32(_p(out), out.numel(), 0.0, 1.0, _p(moments), _p(out), st), "shift")
        ref = want.astype(np.float32).astype(np.float64)
        ref = ref - ref.mean()
        assert np.abs(out.cpu().numpy() - ref).max() <= 1e-6 * np.abs(ref).max()
        assert abs(out.double().mean().item()) < 1e-7
    assert lib.ppo_scale_shift_clip_f32(_p(x), x.numel(), 5.0, 0.0, None, _p(out), st) == -1


def test_axpy_rounds_like_numpy():
    lib, st = _lib.load(), _lib.current_stream()
    rng = np.random.default_rng(4)
    a, b = rng.normal(size=1031).astype(np.float32), rng.normal(size=1031).astype(np.float32)
    dst, src = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    _lib.check(lib.ppo_axpy_f32(_p(dst), _p(src), 0.3, dst.numel(), st), "axpy")
    assert np.array_equal(dst.cpu().numpy(), a + np.float32(0.3) * b)
