"""GPU: the split-bf16 strided convolutions (csrc/conv_strided_bf16x3.hip, tile loop csrc/conv_gemm_tile_bf16x3.h)
against float64 conv2d on the CPU, on the ten cases of tests/test_conv_strided_gpu.py.

Bar, per element (derived in tests/conv_strided_split_torch.py, checked without a GPU by
tests/test_conv_strided_bf16x3_cpu.py):  |got - ref64| <= (2^-15 + 2 (K + 4) u) * A,  u = 2^-24, K the sum length, A the
same operation on absolute values.  The backward launches take the fixture's gate, so no ReLU can flip.  Every output
sits inside a sentinel-filled buffer that must survive; every launch runs twice and must give the same bits; operands
that are small integers must come out bit-equal to float64 (a wrong lane map or tap order is a hard mismatch); on the
K >= 256 forwards the result must differ from the exact launch's and be further from float64, i.e. the split loop ran.

Measured, worst element over the ten cases as a share of the bar (MI355X): forward 0.13 (mtail), backward-data 0.47
(cout1, K = 9), backward-weight 0.77 (n1_conv3, one product per element), bias 0.16 (n1_conv3); max forward error at K >= 256 8.5e-06 - 2.5e-05
against 2.9e-07 - 6.0e-07 of the exact launch.  Per case: the NATURE_SPLIT_ERR lines with -s.
"""
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
import torch.nn.functional as F  # noqa: E402

import conv_strided_split_torch as S  # noqa: E402
from ppo_amd import _lib  # noqa: E402
from test_conv_strided_gpu import CASES, E_INVALID, SENTINEL, guarded, guards_intact, reference  # noqa: E402


def _p(t):
    return None if t is None else t.data_ptr()


def launch_all(lib, suffix, x, mode, wt, b, dy, gate, geom, data_grad, relu=1):
    """Forward, backward-data (where asked) and backward-weight of one case through the `suffix` entry points, each
    output in a guarded buffer -> {"forward", "backward_data", "backward_weight", "bias"} on the device."""
    n, cin, h, w, cout, kh, kw, stride = geom
    dev, st = x.device, _lib.current_stream()
    ho, wo = (h - kh) // stride + 1, (w - kw) // stride + 1
    out = {}
    buf, y = guarded((n, cout, ho, wo), dev)
    _lib.check(getattr(lib, f"ppo_conv2d_strided_forward_{suffix}")(_p(x), mode, _p(wt), _p(b), _p(y), relu, *geom, st), "forward")
    assert guards_intact(buf)
    out["forward"] = y
    if data_grad:
        buf, dx = guarded((n, cin, h, w), dev)
        _lib.check(getattr(lib, f"ppo_conv2d_strided_backward_data_{suffix}")(_p(dy), _p(gate), _p(wt), _p(dx), *geom, st),
                   "backward_data")
        assert guards_intact(buf)
        out["backward_data"] = dx
    nbytes = int(lib.ppo_conv2d_strided_wgrad_workspace_bytes(*geom))
    assert nbytes > 0
    ws_buf, ws = guarded((nbytes // 4,), dev)
    ws.fill_(float("nan"))  # whatever the workspace held must not matter
    wbuf, dw = guarded((cout, cin, kh, kw), dev)
    bbuf, db = guarded((cout,), dev)
    _lib.check(getattr(lib, f"ppo_conv2d_strided_backward_weight_{suffix}")(_p(x), mode, _p(dy), _p(gate), _p(dw), _p(db), _p(ws),
                                                                            nbytes, *geom, st), "backward_weight")
    assert guards_intact(ws_buf) and guards_intact(wbuf) and guards_intact(bbuf)
    out["backward_weight"], out["bias"] = dw, db
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_every_pass_is_inside_the_bar_and_repeats_bit_for_bit(name):
    n, cin, h, w, cout, kh, kw, stride, u8 = CASES[name]
    lib, dev = _lib.load(), torch.device("cuda")
    r = reference(name)
    x, wt, b, dy, gate = (r[k].to(dev) for k in ("raw", "w", "b", "dy", "gate"))
    mode = _lib.PPO_IN_U8 if u8 else _lib.PPO_IN_NONE
    geom = (n, cin, h, w, cout, kh, kw, stride)
    runs = [launch_all(lib, "bf16x3", x, mode, wt, b, dy, gate, geom, not u8) for _ in range(2)]
    for op, got in runs[0].items():
        assert torch.equal(got, runs[1][op]), f"{name} {op}: two launches on the same inputs differ"
    pre = launch_all(lib, "bf16x3", x, mode, wt, b, dy, gate, geom, False, relu=0)["forward"]
    ref = {"forward": r["64"]["relu"], "forward_pre": r["64"]["pre"], "backward_data": r["64"]["dx"],
           "backward_weight": r["64"]["dw"], "bias": r["64"]["db"]}
    got = dict(runs[0], forward_pre=pre)
    failures = []
    for op, t in got.items():
        kind = "forward" if op == "forward_pre" else op
        e = (t.cpu().double() - ref[op]).abs()
        over = float((e / S.bar(name, kind).clamp_min(1e-300)).max())
        share = float((e / (2.0 ** -15 * S.magnitude(name, kind)).clamp_min(1e-300)).max())
        print(f"NATURE_SPLIT_ERR {name} {op} K={S.sum_length(name, kind)} max_err={float(e.max()):.3e} "
              f"of_bar={over:.3f} of_split_term={share:.3f}")
        if over > 1.0:
            failures.append((op, over))
    assert not failures, (name, failures)


@pytest.mark.parametrize("name", ["mtail", "ragged", "conv3"])
def test_small_integers_are_exact(name):
    """Integers in [-2, 2] are bf16 numbers (lo = 0) and every partial sum is an integer below 2^24: all three passes
    and the bias sum must be bit-equal to float64, whatever the order of summation."""
    n, cin, h, w, cout, kh, kw, stride, u8 = CASES[name]
    assert not u8
    lib, dev = _lib.load(), torch.device("cuda")
    g = torch.Generator(device="cpu").manual_seed(11 + len(name))
    ho, wo = (h - kh) // stride + 1, (w - kw) // stride + 1

    def ints(*shape):
        return torch.randint(-2, 3, shape, generator=g).float()
    x, wt, b, dy = ints(n, cin, h, w), ints(cout, cin, kh, kw), ints(cout), ints(n, cout, ho, wo)
    gate = torch.randint(0, 2, (n, cout, ho, wo), generator=g).float()
    grad = torch.where(gate > 0, dy, torch.zeros_like(dy)).double()
    x64, w64, b64 = (t.double().requires_grad_(True) for t in (x, wt, b))
    pre = F.conv2d(x64, w64, b64, stride=stride)
    dx, dw, db = torch.autograd.grad(pre, (x64, w64, b64), grad)
    want = {"forward": F.relu(pre.detach()), "backward_data": dx, "backward_weight": dw, "bias": db}
    xd, wd, bd, dyd, gd = (t.to(dev) for t in (x, wt, b, dy, gate))
    got = launch_all(lib, "bf16x3", xd, _lib.PPO_IN_NONE, wd, bd, dyd, gd, (n, cin, h, w, cout, kh, kw, stride), True)
    for op, t in got.items():
        bad = int((t.cpu().double() != want[op]).sum())
        assert bad == 0, f"{name} {op}: {bad} of {t.numel()} elements differ from the exact integer result"


@pytest.mark.parametrize("name", [c for c in CASES if S.sum_length(c, "forward") >= 256])
def test_the_split_loop_really_ran(name):
    """K >= 256: the split forward is not the exact launch's bits, and it is further from float64."""
    n, cin, h, w, cout, kh, kw, stride, u8 = CASES[name]
    lib, dev = _lib.load(), torch.device("cuda")
    r = reference(name)
    x, wt, b, dy, gate = (r[k].to(dev) for k in ("raw", "w", "b", "dy", "gate"))
    mode = _lib.PPO_IN_U8 if u8 else _lib.PPO_IN_NONE
    geom = (n, cin, h, w, cout, kh, kw, stride)
    errs = {}
    outs = {}
    for suffix in ("f32", "bf16x3"):
        outs[suffix] = launch_all(lib, suffix, x, mode, wt, b, dy, gate, geom, False, relu=0)["forward"]
        errs[suffix] = float((outs[suffix].cpu().double() - r["64"]["pre"]).abs().max())
    print(f"NATURE_SPLIT_RAN {name} exact={errs['f32']:.3e} split={errs['bf16x3']:.3e}")
    assert not torch.equal(outs["f32"], outs["bf16x3"])
    assert errs["bf16x3"] > errs["f32"]


@pytest.mark.parametrize("geom", [(2, 4, 7, 84, 32, 8, 8, 4),    # window taller than the image
                                  (2, 4, 84, 84, 32, 8, 8, 0),   # stride 0
                                  (2, 4, 84, 84, 0, 8, 8, 4),    # no output channels
                                  (0, 4, 84, 84, 32, 8, 8, 4)])  # empty batch
def test_unsupported_geometry_is_rejected(geom):
    lib, dev, st = _lib.load(), torch.device("cuda"), _lib.current_stream()
    scratch = torch.full((1 << 16,), SENTINEL, dtype=torch.float32, device=dev)
    a, b, c, d, e = (scratch[i * 8192:(i + 1) * 8192] for i in range(5))
    calls = (lambda: lib.ppo_conv2d_strided_forward_bf16x3(_p(a), 0, _p(b), _p(c), _p(d), 1, *geom, st),
             lambda: lib.ppo_conv2d_strided_backward_data_bf16x3(_p(a), _p(b), _p(c), _p(d), *geom, st),
             lambda: lib.ppo_conv2d_strided_backward_weight_bf16x3(_p(a), 0, _p(b), None, _p(c), _p(d), _p(e), 8192 * 4, *geom, st))
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
    fn = lib.ppo_conv2d_strided_backward_weight_bf16x3
    assert fn(_p(x), 0, _p(dy), None, _p(dw), None, _p(ws), nbytes - 4, *geom, st) == E_INVALID
    assert fn(_p(x), _lib.PPO_IN_RELU, _p(dy), None, _p(dw), None, _p(ws), nbytes, *geom, st) == E_INVALID
    out = torch.full(dy.shape, SENTINEL, dtype=torch.float32, device=dev)
    assert lib.ppo_conv2d_strided_forward_bf16x3(_p(x), _lib.PPO_IN_RELU, _p(wt), None, _p(out), 0, *geom, st) == E_INVALID
    torch.cuda.synchronize()
    assert bool((dw == SENTINEL).all().item()) and bool((out == SENTINEL).all().item())
