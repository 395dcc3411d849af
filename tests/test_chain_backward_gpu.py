"""GPU: ppo_impala_stack_chain_backward_f32 - the backward-data pass of the last stack and of the previous stack's
blocks in one launch (csrc/stack_fused.hip) - against the four launches it replaces, bit for bit (torch.equal, no
tolerance): directly at the entry point (masks and argmax of a real training forward, and adversarial ones), and
through DualHeadNet.ppo_minibatch, where the launch replaces them from FUSE_CHAIN_BWD_MIN_BATCH images up.

n = 257 makes workgroup 0 walk a second image (the grid is one workgroup per CU, 256): whatever the first image left
in LDS - halo rows, guard cells, the argmax bytes parked in the second small map - meets the second one there."""
import ctypes
import functools

import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from ppo_amd import _lib, models  # noqa: E402

GEOMETRIES = {"84x84": ((4, 84, 84), 6, 21, 11), "64x64": ((3, 64, 64), 15, 16, 8)}  # dims, actions, h = w, ho = wo
C = 32
NEW = "ppo_impala_stack_chain_backward_f32"
PPO_OK, PPO_E_INVALID, PPO_E_ALIGN = 0, -1, -3  # include/ppo_amd.h
OUTPUTS = ("da1", "g1", "da0", "g0", "dc", "g_prev", "post_da1", "post_g1", "post_da0", "post_g0")


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


@functools.lru_cache(maxsize=None)
def _net(geom):
    """Seeded random weights, non-zero biases; only its packed weights and pointer tables are used by the entry-point
    tests (stack 2 = the last stack, stack 1 = the previous one, both 32 channels)."""
    dims, nA, _hw, _ho = GEOMETRIES[geom]
    torch.manual_seed(5)
    net = models.DualHeadNet("impala", dims, nA, hidden_units=256, head_scale=0.1, head_bias=True, device="cuda")
    for name, prm in net.params.items():
        if name.endswith(".bias"):
            prm.normal_(0, 0.1)
    net.mark_weights_changed()
    net._refresh_packed()
    return net


def _inputs(geom, n, kind):
    """g plus the gates (a1, q0, a0, p of both stacks) and argmax: of a training forward through
    ppo_impala_stack_chain_forward_f32 (`real`), or adversarial - taps uniform over 0..8, gate magnitudes |N(0,1)| times
    a value of {-1, -0.0, +0.0, 1}, so every tap and both sides (and both zeros) of the strict `> 0` gate occur everywhere."""
    net, lib = _net(geom), _lib.load()
    _dims, _nA, hw, ho = GEOMETRIES[geom]
    gen = torch.Generator(device="cuda").manual_seed(1000 * n + hw + (kind == "real"))
    big, small = (n, C, hw, hw), (n, C, ho, ho)
    g = torch.randn(small, device="cuda", generator=gen)
    if kind == "real":
        p_prev = torch.randn(big, device="cuda", generator=gen) * 1.5
        pre = net._stack_tail_ptrs(1, C, hw, hw)
        full = net._stack_full_ptrs(2, C, C, hw, hw)
        pa0, pq0, pa1, pq1 = (torch.empty(big, device="cuda") for _ in range(4))
        p, a0, q0, a1, q1 = (torch.empty(small, device="cuda") for _ in range(5))
        argmax = torch.empty(small, dtype=torch.uint8, device="cuda")
        _lib.check(lib.ppo_impala_stack_chain_forward_f32(_p(p_prev), pre[0], pre[1], _p(pa0), _p(pq0), _p(pa1), _p(pq1), full[0],
                                                          full[1], _p(p), _p(argmax), _p(a0), _p(q0), _p(a1), _p(q1), n, C, hw, hw,
                                                          _lib.current_stream()), "chain forward")
        masks, post_masks = (a1, q0, a0, p), (pa1, pq0, pa0, p_prev)
    else:
        signs = torch.tensor([-1.0, -0.0, 0.0, 1.0], device="cuda")

        def gate(shape):
            pick = torch.randint(0, 4, shape, device="cuda", generator=gen)
            return torch.randn(shape, device="cuda", generator=gen).abs() * signs[pick]

        masks, post_masks = tuple(gate(small) for _ in range(4)), tuple(gate(big) for _ in range(4))
        argmax = torch.randint(0, 9, small, device="cuda", generator=gen).to(torch.uint8)
    return g, masks, post_masks, argmax


@functools.lru_cache(maxsize=None)
def _replaced_launches(geom, n, kind):
    """The ten maps as the four launches of the parent write them (computed once per case)."""
    net, lib, st = _net(geom), _lib.load(), _lib.current_stream()
    _dims, _nA, hw, ho = GEOMETRIES[geom]
    g, masks, post_masks, argmax = _inputs(geom, n, kind)
    big, small = (n, C, hw, hw), (n, C, ho, ho)
    out = {k: torch.full(small if i < 4 else big, float("nan"), device="cuda") for i, k in enumerate(OUTPUTS)}
    m = (ctypes.c_void_p * 4)(*[t.data_ptr() for t in masks])
    pm = (ctypes.c_void_p * 4)(*[t.data_ptr() for t in post_masks])
    _lib.check(lib.ppo_impala_stack_tail_backward_f32(_p(g), net._stack_tail_bwd_ptrs(2, C, ho, ho), m, _p(out["da1"]),
                                                      _p(out["g1"]), _p(out["da0"]), _p(out["g0"]), n, C, ho, ho, st), "tail")
    _lib.check(lib.ppo_maxpool3x3s2_backward_f32(_p(out["g0"]), _p(argmax), _p(out["dc"]), n, C, hw, hw, st), "pool bwd")
    _lib.check(lib.ppo_conv3x3_backward_data_packed_f32(_p(out["dc"]), _p(net._pk[("encoder.stacks.2.firstconv", 1)]), None,
                                                        None, _p(out["g_prev"]), n, C, C, hw, hw, st), "firstconv^T")
    _lib.check(lib.ppo_impala_stack_tail_backward_f32(_p(out["g_prev"]), net._stack_tail_bwd_ptrs(1, C, hw, hw), pm,
                                                      _p(out["post_da1"]), _p(out["post_g1"]), _p(out["post_da0"]),
                                                      _p(out["post_g0"]), n, C, hw, hw, st), "tail (previous stack)")
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("kind", ["real", "adversarial"])
@pytest.mark.parametrize("n", [1, 3, 257])
@pytest.mark.parametrize("geom", list(GEOMETRIES))
def test_chained_launch_writes_the_bits_of_the_four_launches_it_replaces(geom, n, kind):
    net, lib = _net(geom), _lib.load()
    _dims, _nA, hw, ho = GEOMETRIES[geom]
    g, masks, post_masks, argmax = _inputs(geom, n, kind)
    want = _replaced_launches(geom, n, kind)
    big, small = (n, C, hw, hw), (n, C, ho, ho)
    got = {k: torch.full(small if i < 4 else big, float("nan"), device="cuda") for i, k in enumerate(OUTPUTS)}
    w = net._stack_chain_bwd_ptrs(2, 1 << 30)
    assert w is not None
    m = (ctypes.c_void_p * 4)(*[t.data_ptr() for t in masks])
    pm = (ctypes.c_void_p * 4)(*[t.data_ptr() for t in post_masks])
    _lib.check(lib.ppo_impala_stack_chain_backward_f32(_p(g), w[0], m, _p(argmax), *[_p(got[k]) for k in OUTPUTS[:6]], w[1], pm,
                                                       *[_p(got[k]) for k in OUTPUTS[6:]], n, C, hw, hw,
                                                       _lib.current_stream()), NEW)
    torch.cuda.synchronize()
    for k in OUTPUTS:
        assert not torch.isnan(want[k]).any(), k  # (every element was written: the comparison below compares results)
        assert torch.equal(got[k], want[k]), (k, int((got[k] != want[k]).sum()))


# ------------------------------------------------------------------------------------------ through the net
REPLACED_AT = {  # launches of the two 32-channel stacks that the chained launch stands in for: (name, h of its map)
    "ppo_impala_stack_tail_backward_f32": ("hw", "ho"), "ppo_conv3x3_backward_data_packed_f32": ("hw",),
    "ppo_maxpool3x3s2_backward_f32": ("hw",)}


def _minibatch(geom, precision, min_batch, monkeypatch):
    dims, nA, _hw, _ho = GEOMETRIES[geom]
    B = 3
    if min_batch is not None:
        monkeypatch.setattr(models, "FUSE_CHAIN_BWD_MIN_BATCH", min_batch)
    torch.manual_seed(11)
    net = models.DualHeadNet("impala", dims, nA, hidden_units=256, head_scale=0.1, head_bias=True, device="cuda",
                             precision=precision)
    gen = torch.Generator(device="cuda").manual_seed(7)
    x = torch.randint(0, 256, (B, *dims), dtype=torch.uint8, device="cuda", generator=gen)
    raw = net.forward(x)["raw_policy"].clone()
    old_lp = torch.log_softmax(raw + 0.1 * torch.randn(B, nA, device="cuda", generator=gen), dim=1).contiguous()
    actions = torch.randint(0, nA, (B,), dtype=torch.int32, device="cuda", generator=gen)
    pac = old_lp.gather(1, actions.long()[:, None])[:, 0].contiguous()
    adv = torch.randn(B, device="cuda", generator=gen)
    ret = torch.randn(B, 1, device="cuda", generator=gen)
    calls, orig = [], net._call

    def call(fn, *a):
        calls.append((fn, a))
        return orig(fn, *a)

    net._call = call
    net.ppo_minibatch(x, actions, pac, old_lp, adv, ret, eps_clip=0.2, ent_coef=0.01, vf_coef=0.5, loss_scale=1.0)
    torch.cuda.synchronize()
    monkeypatch.undo()
    return net.grad.clone(), calls


def _replaced_in(calls, geom):
    """The recorded launches that belong to the four the chained launch replaces (32 channels at h x w or ho x wo)."""
    _dims, _nA, hw, ho = GEOMETRIES[geom]
    size = {"hw": hw, "ho": ho}
    found = []
    for fn, a in calls:
        for where in REPLACED_AT.get(fn, ()):
            # (..., n, [cin,] cout / channels, h, w): a 32 -> 32 layer at that map size
            if tuple(a[-2:]) == (size[where], size[where]) and a[-3] == C and (fn != "ppo_conv3x3_backward_data_packed_f32"
                                                                             or a[-4] == C):
                found.append((fn, size[where]))
    return found


@pytest.mark.parametrize("geom", list(GEOMETRIES))
def test_net_gradients_and_launch_lists_with_and_without_the_chained_launch(geom, monkeypatch):
    _dims, _nA, hw, ho = GEOMETRIES[geom]
    grad_new, calls_new = _minibatch(geom, "high", 1, monkeypatch)
    grad_old, calls_old = _minibatch(geom, "high", None, monkeypatch)
    assert models.FUSE_CHAIN_BWD_MIN_BATCH > 5  # the default leaves small batches on the separate launches
    assert torch.equal(grad_new, grad_old), int((grad_new != grad_old).sum())
    names_new, names_old = [fn for fn, _a in calls_new], [fn for fn, _a in calls_old]
    assert names_new.count(NEW) == 1 and _replaced_in(calls_new, geom) == []
    # the default at B = 3 is the parent's list: the four launches in the parent's order, nothing of the new path
    assert NEW not in names_old
    assert _replaced_in(calls_old, geom) == [("ppo_impala_stack_tail_backward_f32", ho), ("ppo_maxpool3x3s2_backward_f32", hw),
                                             ("ppo_conv3x3_backward_data_packed_f32", hw),
                                             ("ppo_impala_stack_tail_backward_f32", hw)]
    # ... and every other launch of the pass is there on both sides, in the same order
    rest_new = [fn for fn in names_new if fn != NEW]
    dropped = [fn for fn, _s in _replaced_in(calls_old, geom)]
    rest_old = list(names_old)
    for fn in dropped:
        rest_old.remove(fn)
    assert rest_new == rest_old


def test_reduced_precision_keeps_its_own_launches(monkeypatch):
    _grad, calls = _minibatch("84x84", "medium", 1, monkeypatch)
    assert NEW not in [fn for fn, _a in calls]


# ------------------------------------------------------------------------------------------ argument validation
def test_arguments_are_validated_before_any_launch():
    lib = _lib.load()
    hw, n = 21, 2
    buf = torch.zeros(64, device="cuda")  # stands in for every tensor: no call below reaches a launch
    ok = ctypes.c_void_p(buf.data_ptr())
    off = ctypes.c_void_p(buf.data_ptr() + 4)  # 4-byte aligned, not 16
    w5, w4 = (ctypes.c_void_p * 5)(*[buf.data_ptr()] * 5), (ctypes.c_void_p * 4)(*[buf.data_ptr()] * 4)

    def call(**kw):
        a = dict(g=ok, w=w5, masks=w4, argmax=ok, da1=ok, g1=ok, da0=ok, g0=ok, dc=ok, g_prev=ok, post_w=w4, post_masks=w4,
                 post_da1=ok, post_g1=ok, post_da0=ok, post_g0=ok, n=n, c=C, h=hw, w_=hw)
        a.update(kw)
        return lib.ppo_impala_stack_chain_backward_f32(*a.values(), _lib.current_stream())

    assert call(n=0) == PPO_OK
    assert call(n=0, g=None) == PPO_OK  # nothing to do comes first
    for name in ("g", "w", "masks", "argmax", "da1", "g1", "da0", "g0", "dc", "g_prev", "post_w", "post_masks", "post_da1",
                 "post_g1", "post_da0", "post_g0"):
        assert call(**{name: None}) == PPO_E_INVALID, name
        assert b"null" in lib.ppo_last_error()
    assert call(w=(ctypes.c_void_p * 5)(*([buf.data_ptr()] * 4 + [None]))) == PPO_E_INVALID
    assert call(post_masks=(ctypes.c_void_p * 4)(*([buf.data_ptr()] * 3 + [None]))) == PPO_E_INVALID
    assert call(w=(ctypes.c_void_p * 5)(*([buf.data_ptr()] * 4 + [off.value]))) == PPO_E_ALIGN
    assert call(post_w=(ctypes.c_void_p * 4)(*([off.value] + [buf.data_ptr()] * 3))) == PPO_E_ALIGN
    assert call(argmax=ctypes.c_void_p(buf.data_ptr() + 1)) == PPO_E_ALIGN
    for c, h in ((32, 11), (16, 21), (32, 42), (64, 21)):
        assert call(c=c, h=h, w_=h) == PPO_E_INVALID, (c, h)
        assert b"no kernel" in lib.ppo_last_error()
    assert call(n=-1) == PPO_E_INVALID
    torch.cuda.synchronize()
