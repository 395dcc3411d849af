"""GPU: the 16-channel resident stack kernel (csrc/stack_fused.hip stack_shift_kernel) keeps its map in LDS with two zero
pad floats behind every row and, forward, already ReLU'd, so that its K loop is operand read + MFMA only.  What it
computes must stay, bit for bit, what four convolution launches compute: forward against
ppo_conv3x3_forward_packed_f32 x 4, backward-data against ppo_conv3x3_backward_data_packed_f32 x 4, on all four
written maps.

Inputs are seeded normal data with what a wrong pad, a stale pad or a misplaced ReLU would trip over planted in them:
the outermost columns and rows carry large magnitudes (a tap that wraps into the neighbouring row, or reads a pad
somebody wrote, moves the result by far more than round-off), the forward input has exact zeros, -0.0 and negative
values, the backward masks have zeros of both signs and values of both signs.  Batch 258 at 32x32 is the smallest
at which a workgroup (the launch has at most 256, one per CU) takes a second image: the pads and the ReLU'd state
have to survive the image loop.
"""
import ctypes
import functools

import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from ppo_amd import _lib  # noqa: E402

C = 16
CASES = [(32, 1), (32, 3), (32, 258), (42, 2)]


def _p(t):
    return None if t is None else t.data_ptr()


def _plant_edges(t, big):
    """Outermost rows and columns at +-big (both signs, so that the ReLU passes some and stops others)."""
    sign = torch.where(torch.rand(t.shape, device=t.device) < 0.5, -1.0, 1.0)
    edge = torch.zeros(t.shape[-2:], dtype=torch.bool, device=t.device)
    edge[0, :] = edge[-1, :] = edge[:, 0] = edge[:, -1] = True
    return torch.where(edge, big * sign, t)


def _plant_zeros(t, share=0.05):
    """A share of exact +0.0 and as many -0.0, anywhere in the map."""
    r = torch.rand(t.shape, device=t.device)
    t = torch.where(r < share, torch.zeros_like(t), t)
    return torch.where((r >= share) & (r < 2 * share), -torch.zeros_like(t), t)


@functools.lru_cache(maxsize=None)
def _weights():
    lib = _lib.load()
    dev = torch.device("cuda")
    torch.manual_seed(20)
    ws = [torch.randn(C, C, 3, 3, device=dev) / 12.0 for _ in range(4)]  # block0.conv0, block0.conv1, block1.conv0, block1.conv1
    bs = [torch.randn(C, device=dev) * 0.1 for _ in range(4)]
    pf = [torch.empty(lib.ppo_conv3x3_packed_floats(C, C, 0), device=dev) for _ in range(4)]
    pb = [torch.empty(lib.ppo_conv3x3_packed_floats(C, C, 1), device=dev) for _ in range(4)]
    jobs = (_lib.PackJob * 8)(*[_lib.PackJob(_p(w), _p(q), C, C, 0) for w, q in zip(ws, pf)],
                              *[_lib.PackJob(_p(w), _p(q), C, C, 1) for w, q in zip(ws, pb)])
    _lib.check(lib.ppo_conv3x3_pack_weights_f32(ctypes.addressof(jobs), 8, _lib.current_stream()), "pack")
    torch.cuda.synchronize()
    return bs, pf, pb


@functools.lru_cache(maxsize=None)
def _run(hw, n):
    """Both passes, fused and as four launches each, computed once per case."""
    lib = _lib.load()
    st = _lib.current_stream()
    dev = torch.device("cuda")
    bs, pf, pb = _weights()
    torch.manual_seed(hw * 1000 + n)
    x = _plant_zeros(_plant_edges(torch.randn(n, C, hw, hw, device=dev), 1e3)).contiguous()
    assert (x == 0).any() and torch.signbit(x[x == 0]).any() and (x < 0).any() and (x.abs() == 1e3).any()

    def fwd(src, layer, res):
        out = torch.empty_like(src)
        _lib.check(lib.ppo_conv3x3_forward_packed_f32(_p(src), _lib.PPO_IN_RELU, _p(pf[layer]), _p(bs[layer]), _p(res), _p(out),
                                                      n, C, C, hw, hw, st), "forward packed")
        return out

    a0 = fwd(x, 0, None)
    q0 = fwd(a0, 1, x)
    a1 = fwd(q0, 2, None)
    q1 = fwd(a1, 3, q0)
    want_f = [a0, q0, a1, q1]
    got_f = [torch.full_like(x, float("nan")) for _ in range(4)]
    wp = (ctypes.c_void_p * 4)(*[_p(t) for t in pf])
    bp = (ctypes.c_void_p * 4)(*[_p(t) for t in bs])
    _lib.check(lib.ppo_impala_stack_tail_forward_f32(_p(x), wp, bp, *[_p(t) for t in got_f], n, C, hw, hw, st), "stack forward")

    # backward-data: gates with zeros of both signs and values of both signs (the forward maps, zeros planted), in
    # processing order a1, q0, a0, p; weights block1.conv1, block1.conv0, block0.conv1, block0.conv0
    g = _plant_edges(torch.randn(n, C, hw, hw, device=dev), 1e3).contiguous()
    masks = [_plant_zeros(t).contiguous() for t in (a1, q0, a0, x)]
    for m in masks:
        assert (m == 0).any() and torch.signbit(m[m == 0]).any() and (m < 0).any() and (m > 0).any()

    def bwd(dy, layer, mask, dres):
        dx = torch.empty_like(dy)
        _lib.check(lib.ppo_conv3x3_backward_data_packed_f32(_p(dy), _p(pb[layer]), _p(mask), _p(dres), _p(dx), n, C, C, hw, hw, st),
                   "backward-data packed")
        return dx

    da1 = bwd(g, 3, masks[0], None)
    g1 = bwd(da1, 2, masks[1], g)
    da0 = bwd(g1, 1, masks[2], None)
    g0 = bwd(da0, 0, masks[3], g1)
    want_b = [da1, g1, da0, g0]
    got_b = [torch.full_like(g, float("nan")) for _ in range(4)]
    wtp = (ctypes.c_void_p * 4)(*[_p(pb[i]) for i in (3, 2, 1, 0)])
    mp = (ctypes.c_void_p * 4)(*[_p(m) for m in masks])
    _lib.check(lib.ppo_impala_stack_tail_backward_f32(_p(g), wtp, mp, *[_p(t) for t in got_b], n, C, hw, hw, st), "stack backward")
    torch.cuda.synchronize()

    def verdict(names, want, got):  # (the maps themselves are not kept: 258 images x 16 maps)
        return {k: dict(finite=bool(torch.isfinite(w).all()), max=float(w.abs().max()), equal=torch.equal(g_, w),
                        differing=int((g_ != w).sum())) for k, w, g_ in zip(names, want, got)}

    return verdict(("a0", "q0", "a1", "q1"), want_f, got_f), verdict(("da1", "g1", "da0", "g0"), want_b, got_b)


def _check(verdicts):
    assert len(verdicts) == 4
    for name, v in verdicts.items():
        assert v["finite"], name
        assert v["max"] > 100.0, name  # the planted edges reach every map
        assert v["equal"], (name, v["differing"])


@pytest.mark.parametrize("hw,n", CASES)
def test_forward_16_channel_stack_is_bit_identical_to_four_convolutions(hw, n):
    assert _lib.load().ppo_impala_stack_tail_supported(C, hw, hw) == 1
    _check(_run(hw, n)[0])


@pytest.mark.parametrize("hw,n", CASES)
def test_backward_16_channel_stack_is_bit_identical_to_four_convolutions(hw, n):
    _check(_run(hw, n)[1])
