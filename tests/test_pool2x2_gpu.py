"""GPU: the fused 2x2 max-pool + ReLU kernels (csrc/pool2x2.hip) against torch on the CPU.

Reference: F.max_pool2d(x, 2, 2, return_indices=True), F.relu and autograd of F.relu(F.max_pool2d(x, 2, 2)) - what the
reference's RTG encoder applies behind every convolution (rl/models.py:203-205).  Both passes are exact: a maximum has no
rounding and each din element receives at most one term, so the bar is torch.equal, not a tolerance.

Per shape two inputs: normal ones, and integers -2..2 as floats, where about a third of the windows tie (torch gives the
gradient to the first maximum in row-major order) and many pooled values are exactly 0 (ReLU derivative 0 at 0).  Every
device tensor a kernel writes sits between canary elements that must survive, and din is filled with NaN before the
backward launch, so an unwritten trailing row or column shows."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
import torch.nn.functional as F  # noqa: E402

from ppo_amd import _lib  # noqa: E402

E_INVALID = -1
CLOSED = 4
PAD = 64  # canary elements on either side (a multiple of 2 floats: the framed tensor keeps its 8-byte alignment)
CASES = [
    (3, 5, 2, 2),       # one window
    (2, 3, 3, 3),       # both sides odd
    (2, 4, 7, 8),       # odd height
    (2, 4, 8, 7),       # odd width
    (2, 32, 17, 22),    # the small test net's first pool
    (1, 32, 41, 41),    # the 84x84 net's first pool
    (1, 64, 20, 20),    # even, aligned
    (1025, 64, 2, 2),   # 65600 planes: beyond a blockIdx.y grid
]
KINDS = ["normal", "ints"]


def ptr(t):
    return None if t is None else t.data_ptr()


def launch(name, *a):
    lib = _lib.load()
    return getattr(lib, name)(*a, _lib.current_stream())


def call(name, *a):
    rc = launch(name, *a)
    assert rc == 0, _lib.load().ppo_last_error()


class Framed:
    """A device tensor of `shape` between PAD canary elements, starting `offset` elements into its allocation."""

    def __init__(self, shape, dtype, fill=None, offset=0):
        n = int(np.prod(shape))
        self.canary = 77 if dtype == torch.uint8 else -12345.0
        self.flat = torch.full((offset + n + 2 * PAD,), self.canary, dtype=dtype, device="cuda")
        self.lo, self.hi = offset + PAD, offset + PAD + n
        self.t = self.flat[self.lo:self.hi].view(shape)
        if fill is not None:
            self.t.fill_(fill)

    def intact(self):
        return bool((self.flat[:self.lo] == self.canary).all()) and bool((self.flat[self.hi:] == self.canary).all())


def draw(shape, kind, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "ints":
        return torch.randint(-2, 3, shape, generator=g).float()
    return torch.randn(shape, generator=g)


def reference(x, dout=None):
    """(relu(pool(x)), gate, din) by torch on the CPU; gate: the window tap ky*2+kx of torch's index, 4 where pooled <= 0
    (or NaN: not > 0)."""
    n, c, h, w = x.shape
    pooled, idx = F.max_pool2d(x, 2, 2, return_indices=True)
    ho, wo = pooled.shape[2:]
    iy, ix = idx // w, idx % w
    oy = torch.arange(ho).view(1, 1, ho, 1)
    ox = torch.arange(wo).view(1, 1, 1, wo)
    tap = (iy - 2 * oy) * 2 + (ix - 2 * ox)
    assert int(tap.min()) >= 0 and int(tap.max()) <= 3
    gate = torch.where(pooled > 0, tap, torch.full_like(tap, CLOSED)).to(torch.uint8)
    din = None
    if dout is not None:
        xg = x.clone().requires_grad_(True)
        F.relu(F.max_pool2d(xg, 2, 2)).backward(dout)
        din = xg.grad
    return F.relu(pooled), gate, din


_REFS = {}


def case_data(shape, kind):
    """Inputs and torch's results of one (shape, kind), computed once and shared by the tests that read them."""
    key = (shape, kind)
    if key not in _REFS:
        n, c, h, w = shape
        x = draw(shape, kind, seed=h * 1000 + w)
        dout = draw((n, c, h // 2, w // 2), "normal", seed=h * 1000 + w + 1)
        _REFS[key] = (x, dout, *reference(x, dout))
    return _REFS[key]


def run_forward(x, with_gate=True, offset=0):
    n, c, h, w = x.shape
    xin = Framed(x.shape, torch.float32, offset=offset)
    xin.t.copy_(x)
    out = Framed((n, c, h // 2, w // 2), torch.float32, fill=float("nan"))
    gate = Framed((n, c, h // 2, w // 2), torch.uint8, fill=99) if with_gate else None
    call("ppo_maxpool2x2_relu_forward_f32", ptr(xin.t), ptr(out.t), ptr(gate.t) if gate else None, n, c, h, w)
    torch.cuda.synchronize()
    assert out.intact() and xin.intact() and (gate is None or gate.intact())
    assert torch.equal(xin.t.cpu(), x) or bool(torch.isnan(x).any())  # the input is read only
    return out.t.cpu(), (gate.t.cpu() if gate else None)


def run_backward(dout, gate, shape, offset=0):
    n, c, h, w = shape
    din = Framed(shape, torch.float32, fill=float("nan"), offset=offset)
    g, a = dout.cuda(), gate.cuda()
    call("ppo_maxpool2x2_relu_backward_f32", ptr(g), ptr(a), ptr(din.t), n, c, h, w)
    torch.cuda.synchronize()
    assert din.intact()
    return din.t.cpu()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", CASES, ids=lambda s: "x".join(map(str, s)))
def test_forward_matches_torch(shape, kind):
    x, _dout, want_out, want_gate, _din = case_data(shape, kind)
    if kind == "ints" and want_gate.numel() >= 500:
        # the input is what it is meant to be: ties and exact zeros in numbers
        assert float((want_out == 0).float().mean()) > 0.05 and float((want_gate == CLOSED).float().mean()) > 0.05
    out, gate = run_forward(x)
    assert torch.equal(out, want_out)
    assert torch.equal(gate, want_gate)
    out_only, _ = run_forward(x, with_gate=False)  # an inference forward: gate = NULL
    assert torch.equal(out_only, want_out)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", CASES, ids=lambda s: "x".join(map(str, s)))
def test_backward_matches_autograd(shape, kind):
    """din from (dout, the kernel's own gate) against autograd; every element written (din starts as NaN)."""
    x, dout, _out, want_gate, want_din = case_data(shape, kind)
    _o, gate = run_forward(x)
    assert torch.equal(gate, want_gate)
    din = run_backward(dout, gate, shape)
    assert not bool(torch.isnan(din).any())
    assert torch.equal(din, want_din)
    n, c, h, w = shape
    if h % 2:
        assert float(din[:, :, h - 1, :].abs().max()) == 0.0
    if w % 2:
        assert float(din[:, :, :, w - 1].abs().max()) == 0.0


@pytest.mark.parametrize("shape", [(1, 64, 20, 20), (2, 4, 7, 8)], ids=lambda s: "x".join(map(str, s)))
def test_even_width_at_a_4_byte_aligned_base(shape):
    """An even row length whose base is only 4-byte aligned takes the scalar form: same results."""
    x, dout, want_out, want_gate, want_din = case_data(shape, "ints")
    out, gate = run_forward(x, offset=1)
    assert torch.equal(out, want_out) and torch.equal(gate, want_gate)
    assert torch.equal(run_backward(dout, gate, shape, offset=1), want_din)


@pytest.mark.parametrize("shape", CASES, ids=lambda s: "x".join(map(str, s)))
def test_nan_propagates(shape):
    """One NaN in the input: its window's pooled value and output are NaN, as torch's; its gate byte says closed (NaN is
    not > 0), every other window is untouched."""
    x = case_data(shape, "normal")[0].clone()
    x[-1, -1, 1, 0] = float("nan")
    want_out, want_gate, _ = reference(x)
    assert bool(torch.isnan(want_out[-1, -1, 0, 0])) and int(torch.isnan(want_out).sum()) == 1
    assert int(want_gate[-1, -1, 0, 0]) == CLOSED
    out, gate = run_forward(x)
    assert np.array_equal(out.numpy(), want_out.numpy(), equal_nan=True)
    assert torch.equal(gate, want_gate)
    out_only, _ = run_forward(x, with_gate=False)
    assert np.array_equal(out_only.numpy(), want_out.numpy(), equal_nan=True)


@pytest.mark.parametrize("name", ["ppo_maxpool2x2_relu_forward_f32", "ppo_maxpool2x2_relu_backward_f32"])
def test_refusals(name):
    lib = _lib.load()
    a = torch.zeros(64, dtype=torch.float32, device="cuda")
    b = torch.full((64,), 5.0, dtype=torch.float32, device="cuda")
    gate = torch.zeros(64, dtype=torch.uint8, device="cuda")
    fwd = name.endswith("forward_f32")
    good = (ptr(a), ptr(b), ptr(gate)) if fwd else (ptr(a), ptr(gate), ptr(b))
    assert launch(name, *good, 1, 1, 2, 2) == 0
    bad = [(good, (1, 1, 1, 2)), (good, (1, 1, 2, 1)), (good, (0, 1, 2, 2)), (good, (1, 0, 2, 2)), (good, (-1, 1, 2, 2)),
           (good, (1 << 15, 1 << 15, 2, 2)), (good, (1 << 14, 1 << 14, 2, 2)),  # 2^30 planes; 2^30 elements
           ((None, good[1], good[2]), (1, 1, 2, 2)), ((good[0], None, good[2]), (1, 1, 2, 2))]
    if not fwd:
        bad.append(((good[0], good[1], None), (1, 1, 2, 2)))  # (the forward's gate is nullable)
    torch.cuda.synchronize()
    b.fill_(5.0)
    for ptrs, dims in bad:
        assert launch(name, *ptrs, *dims) == E_INVALID, (ptrs, dims)
        assert name.encode() in lib.ppo_last_error(), (dims, lib.ppo_last_error())
    torch.cuda.synchronize()
    assert bool((b == 5.0).all())  # nothing was launched
