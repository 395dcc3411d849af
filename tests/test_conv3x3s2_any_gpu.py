"""GPU: the generic 3x3 / stride 2 / padding 1 convolution kernels (csrc/conv3x3_any.hip, the ppo_conv3x3s2_any_* entry
points) against float64 torch - F.conv2d(..., stride=2, padding=1) and its autograd - on the same tensors.

Bar: the project's own for convolution outputs and gradients - rel 1e-4 of the reference tensor's max
(tests/test_conv_gpu.py).  Every output sits inside a larger buffer filled with a sentinel, which must survive around it;
every entry point is launched twice and must give the same bits; a rejected call launches nothing.
"""
import functools

import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
import torch.nn.functional as F  # noqa: E402

from ppo_amd import _lib  # noqa: E402

# (n, cin, cout, h, w) of the INPUT; the output map is (h + 1) // 2 x (w + 1) // 2
GEOMETRIES = [
    (1, 1, 1, 1, 1),        # only the centre tap
    (2, 1, 2, 2, 1),        # one output; the even side never touches the far padding
    (2, 2, 1, 1, 2),        # the same, transposed
    (3, 2, 3, 3, 4),        # odd and even sides together
    (4, 2, 16, 5, 6),       # small, non-square
    (5, 3, 5, 7, 9),        # odd channel counts, h != w
    (2, 17, 33, 5, 6),      # one past the channel tiles
    (3, 12, 16, 33, 31),    # neither GEMM's M is a multiple of the 64-row tile
    (2, 16, 32, 42, 42),    # the 84x84 net's second stack
    (2, 4, 16, 84, 84),     # the uint8 first layer
]
PAD = 4096       # sentinel floats on either side of an output
SENTINEL = -7.25e30
E_INVALID = -1
NONE, RELU, U8 = _lib.PPO_IN_NONE, _lib.PPO_IN_RELU, _lib.PPO_IN_U8


def _p(t):
    return None if t is None else t.data_ptr()


def _id(g):
    return "x".join(str(v) for v in g)


def _out_hw(h, w):
    return (h + 1) // 2, (w + 1) // 2


def test_geometry_lists_agree():
    """The host walk of the offset arithmetic (tests/test_conv3x3s2_any_index.py) covers exactly these geometries."""
    import test_conv3x3s2_any_index
    assert test_conv3x3s2_any_index.GEOMETRIES == GEOMETRIES


@functools.lru_cache(maxsize=None)
def reference(geom):
    """Inputs (CPU) and the float64 results of one geometry, computed once and left unchanged."""
    n, cin, cout, h, w = geom
    ho, wo = _out_hw(h, w)
    g = torch.Generator(device="cpu").manual_seed(hash(geom) % (1 << 31))
    x = torch.randn(n, cin, h, w, generator=g)
    xu = torch.randint(0, 256, (n, cin, h, w), generator=g, dtype=torch.uint8)
    wt = torch.randn(cout, cin, 3, 3, generator=g) / (9 * cin) ** 0.5
    b = torch.randn(cout, generator=g) * 0.5 + 0.25
    res = torch.randn(n, cout, ho, wo, generator=g)
    dy = torch.randn(n, cout, ho, wo, generator=g)
    dres = torch.randn(n, cin, h, w, generator=g)
    r = {"x": x, "xu": xu, "w": wt, "b": b, "res": res, "dy": dy, "dres": dres}
    w64, b64, dy64 = wt.double(), b.double(), dy.double()
    for mode, src in ((NONE, x.double()), (RELU, x.double()), (U8, xu.double() / 255.0)):
        if mode == U8 and cin > 12:
            continue
        xin = src.clone().requires_grad_(True)
        wv, bv = w64.clone().requires_grad_(True), b64.clone().requires_grad_(True)
        fx = F.relu(xin) if mode == RELU else xin
        out = F.conv2d(fx, wv, bv, stride=2, padding=1)
        assert tuple(out.shape) == (n, cout, ho, wo)
        dx, dw, db = torch.autograd.grad(out, (xin, wv, bv), dy64)
        r[mode] = {"out": out.detach(), "nobias": F.conv2d(fx, wv, None, stride=2, padding=1).detach(), "dx": dx, "dw": dw,
                   "db": db}
    return r


def guarded(shape, dev):
    """An output of `shape` inside a sentinel-filled buffer: (whole buffer, the output view)."""
    numel = 1
    for s in shape:
        numel *= s
    buf = torch.full((PAD + numel + PAD,), SENTINEL, dtype=torch.float32, device=dev)
    return buf, buf[PAD:PAD + numel].view(shape)


def guards_intact(buf):
    return bool((buf[:PAD] == SENTINEL).all().item()) and bool((buf[-PAD:] == SENTINEL).all().item())


def check(what, got, ref, rel=1e-4):
    err = (got.detach().cpu().double() - ref).abs().max().item()
    bar = rel * max(ref.abs().max().item(), 1e-30)
    print(f"S2_ERR {what} err={err:.3e} bar={bar:.3e}")
    assert err <= bar, f"{what}: max error {err:.3e} > {bar:.3e}"


def twice(launch, shape, dev):
    """Run launch(out) into two guarded buffers; the guards hold and the bits agree.  Returns the result."""
    outs = []
    for _ in range(2):
        buf, out = guarded(shape, dev)
        _lib.check(launch(out), "launch")
        assert guards_intact(buf)
        outs.append(out)
    assert torch.equal(outs[0], outs[1]), "two launches on the same inputs differ"
    assert not bool((outs[0] == SENTINEL).any().item()), "an output element was never written"
    return outs[0]


@pytest.mark.parametrize("geom", GEOMETRIES, ids=_id)
def test_forward_against_float64(geom):
    n, cin, cout, h, w = geom
    lib, dev, st = _lib.load(), torch.device("cuda"), _lib.current_stream()
    assert lib.ppo_conv3x3s2_any_supported(cin, cout, h, w) == 1
    r = reference(geom)
    x, xu, wt, b, res = (r[k].to(dev) for k in ("x", "xu", "w", "b", "res"))
    shape, dims = (n, cout, *_out_hw(h, w)), (n, cin, cout, h, w)
    fwd = lib.ppo_conv3x3s2_any_forward_f32
    out = twice(lambda o: fwd(_p(x), NONE, _p(wt), _p(b), None, _p(o), *dims, st), shape, dev)
    check(f"{_id(geom)} forward", out, r[NONE]["out"])
    out = twice(lambda o: fwd(_p(x), NONE, _p(wt), None, None, _p(o), *dims, st), shape, dev)
    check(f"{_id(geom)} forward_nobias", out, r[NONE]["nobias"])
    out = twice(lambda o: fwd(_p(x), NONE, _p(wt), None, _p(res), _p(o), *dims, st), shape, dev)
    check(f"{_id(geom)} forward_nobias_residual", out, r[NONE]["nobias"] + r["res"].double())
    out = twice(lambda o: fwd(_p(x), RELU, _p(wt), _p(b), _p(res), _p(o), *dims, st), shape, dev)
    check(f"{_id(geom)} forward_relu_residual", out, r[RELU]["out"] + r["res"].double())
    out = twice(lambda o: fwd(_p(x), RELU, _p(wt), None, None, _p(o), *dims, st), shape, dev)
    check(f"{_id(geom)} forward_relu_nobias", out, r[RELU]["nobias"])
    if cin <= 12:
        out = twice(lambda o: fwd(_p(xu), U8, _p(wt), _p(b), None, _p(o), *dims, st), shape, dev)
        check(f"{_id(geom)} forward_u8", out, r[U8]["out"])
        out = twice(lambda o: fwd(_p(xu), U8, _p(wt), None, _p(res), _p(o), *dims, st), shape, dev)
        check(f"{_id(geom)} forward_u8_nobias_residual", out, r[U8]["nobias"] + r["res"].double())


@pytest.mark.parametrize("geom", GEOMETRIES, ids=_id)
def test_backward_data_against_float64(geom):
    n, cin, cout, h, w = geom
    lib, dev, st = _lib.load(), torch.device("cuda"), _lib.current_stream()
    r = reference(geom)
    x, wt, dy, dres = (r[k].to(dev) for k in ("x", "w", "dy", "dres"))
    shape, dims = (n, cin, h, w), (n, cin, cout, h, w)
    bwd = lib.ppo_conv3x3s2_any_backward_data_f32
    dx = twice(lambda o: bwd(_p(dy), _p(wt), None, None, _p(o), *dims, st), shape, dev)
    check(f"{_id(geom)} backward_data", dx, r[NONE]["dx"])
    dx = twice(lambda o: bwd(_p(dy), _p(wt), None, _p(dres), _p(o), *dims, st), shape, dev)
    check(f"{_id(geom)} backward_data_dres", dx, r[NONE]["dx"] + r["dres"].double())
    dx = twice(lambda o: bwd(_p(dy), _p(wt), _p(x), None, _p(o), *dims, st), shape, dev)
    check(f"{_id(geom)} backward_data_relu", dx, r[RELU]["dx"])
    # through the ReLU of the forward's load transform (derivative 0 at 0), plus a skip-connection gradient
    dx = twice(lambda o: bwd(_p(dy), _p(wt), _p(x), _p(dres), _p(o), *dims, st), shape, dev)
    check(f"{_id(geom)} backward_data_relu_dres", dx, r[RELU]["dx"] + r["dres"].double())
    # an exact zero in relu_src gates the gradient off
    x0 = torch.zeros_like(x)
    dx = twice(lambda o: bwd(_p(dy), _p(wt), _p(x0), _p(dres), _p(o), *dims, st), shape, dev)
    assert torch.equal(dx, dres)


@pytest.mark.parametrize("geom", GEOMETRIES, ids=_id)
def test_backward_weight_against_float64(geom):
    n, cin, cout, h, w = geom
    lib, dev, st = _lib.load(), torch.device("cuda"), _lib.current_stream()
    r = reference(geom)
    x, xu, dy = (r[k].to(dev) for k in ("x", "xu", "dy"))
    dims = (n, cin, cout, h, w)
    bww = lib.ppo_conv3x3s2_any_backward_weight_f32
    nbytes = int(lib.ppo_conv3x3s2_any_wgrad_workspace_bytes(*dims))
    assert nbytes > 0
    for mode, src in ((NONE, x), (RELU, x), (U8, xu)):
        if mode not in r:
            continue
        results = []
        for fill in (float("nan"), 3.0):  # whatever the workspace held must not matter
            ws_buf, ws = guarded((nbytes // 4,), dev)
            ws.fill_(fill)
            wbuf, dw = guarded((cout, cin, 3, 3), dev)
            bbuf, db = guarded((cout,), dev)
            _lib.check(bww(_p(src), mode, _p(dy), _p(dw), _p(db), _p(ws), nbytes, *dims, 0, st), "backward_weight")
            assert guards_intact(ws_buf) and guards_intact(wbuf) and guards_intact(bbuf)
            results.append((dw.clone(), db.clone()))
        assert torch.equal(results[0][0], results[1][0]) and torch.equal(results[0][1], results[1][1]), \
            "two weight-gradient launches on the same inputs differ"
        check(f"{_id(geom)} backward_weight mode={mode}", results[0][0], r[mode]["dw"])
        check(f"{_id(geom)} bias mode={mode}", results[0][1], r[mode]["db"])
        # accumulate: the same sum added to what is there (x + x is exact in float32)
        _lib.check(bww(_p(src), mode, _p(dy), _p(dw), _p(db), _p(ws), nbytes, *dims, 1, st), "backward_weight accumulate")
        assert guards_intact(wbuf) and guards_intact(bbuf)
        assert torch.equal(dw, 2.0 * results[0][0]) and torch.equal(db, 2.0 * results[0][1])
        check(f"{_id(geom)} backward_weight accumulated mode={mode}", dw, 2.0 * r[mode]["dw"])
        # dbias is nullable
        _lib.check(bww(_p(src), mode, _p(dy), _p(dw), None, _p(ws), nbytes, *dims, 0, st), "backward_weight without dbias")
        assert torch.equal(dw, results[0][0]) and torch.equal(db, 2.0 * results[0][1])


@pytest.mark.parametrize("geom", [(3, 5, 7, 9, 8), (2, 17, 33, 5, 6), (2, 16, 16, 20, 19)], ids=_id)
def test_exact_on_integer_data(geom):
    """Small-integer operands make every product and partial sum exact in float32, so any operand-mapping mistake
    (wrong lane -> element map, swapped or mirrored taps, a stride applied to the wrong side) shows as a hard mismatch,
    in all three kernels."""
    n, cin, cout, h, w = geom
    lib, dev, st = _lib.load(), torch.device("cuda"), _lib.current_stream()
    g = torch.Generator(device="cpu").manual_seed(7 + cin)
    x = torch.randint(-3, 4, (n, cin, h, w), generator=g).double().requires_grad_(True)
    wt = torch.randint(-2, 3, (cout, cin, 3, 3), generator=g).double().requires_grad_(True)
    b = torch.randint(-5, 6, (cout,), generator=g).double().requires_grad_(True)
    dy = torch.randint(-3, 4, (n, cout, *_out_hw(h, w)), generator=g).double()
    ref = F.conv2d(x, wt, b, stride=2, padding=1)
    rdx, rdw, rdb = torch.autograd.grad(ref, (x, wt, b), dy)
    xd, wd, bd, dyd = (t.detach().float().to(dev) for t in (x, wt, b, dy))
    dims = (n, cin, cout, h, w)
    out = torch.empty(ref.shape, dtype=torch.float32, device=dev)
    _lib.check(lib.ppo_conv3x3s2_any_forward_f32(_p(xd), NONE, _p(wd), _p(bd), None, _p(out), *dims, st), "forward")
    assert torch.equal(out.cpu(), ref.detach().float())
    dx = torch.empty(xd.shape, dtype=torch.float32, device=dev)
    _lib.check(lib.ppo_conv3x3s2_any_backward_data_f32(_p(dyd), _p(wd), None, None, _p(dx), *dims, st), "backward_data")
    assert torch.equal(dx.cpu(), rdx.float())
    nbytes = int(lib.ppo_conv3x3s2_any_wgrad_workspace_bytes(*dims))
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
    dw, db = torch.empty(wd.shape, dtype=torch.float32, device=dev), torch.empty(cout, dtype=torch.float32, device=dev)
    _lib.check(lib.ppo_conv3x3s2_any_backward_weight_f32(_p(xd), NONE, _p(dyd), _p(dw), _p(db), _p(ws), nbytes, *dims, 0, st),
               "backward_weight")
    assert torch.equal(dw.cpu(), rdw.float()) and torch.equal(db.cpu(), rdb.float())


@pytest.mark.parametrize("geom", [(2, 0, 16, 8, 8),          # cin = 0
                                  (2, 4, 16, 0, 8),          # h = 0
                                  (2, 4, 16, 8, 4097),       # w = 4097
                                  (0, 4, 16, 8, 8),          # n = 0
                                  (2, 4, 0, 8, 8),           # cout = 0
                                  (64, 1, 1, 4096, 4096),    # an input of 2^30 elements
                                  (1, 1, 256, 4096, 4096)],  # an output of 2^30 elements
                         ids=_id)
def test_bad_arguments_are_rejected(geom):
    n, cin, cout, h, w = geom
    lib, dev, st = _lib.load(), torch.device("cuda"), _lib.current_stream()
    in_range = all(1 <= v <= 4096 for v in (cin, cout, h, w))
    assert lib.ppo_conv3x3s2_any_supported(cin, cout, h, w) == int(in_range)
    assert int(lib.ppo_conv3x3s2_any_wgrad_workspace_bytes(*geom)) == 0
    scratch = torch.full((1 << 16,), SENTINEL, dtype=torch.float32, device=dev)
    a, b, c, d, e = (scratch[i * 8192:(i + 1) * 8192] for i in range(5))
    calls = (lambda: lib.ppo_conv3x3s2_any_forward_f32(_p(a), NONE, _p(b), _p(c), None, _p(d), *geom, st),
             lambda: lib.ppo_conv3x3s2_any_backward_data_f32(_p(a), _p(b), None, None, _p(d), *geom, st),
             lambda: lib.ppo_conv3x3s2_any_backward_weight_f32(_p(a), NONE, _p(b), _p(c), _p(d), _p(e), 8192 * 4, *geom, 0, st))
    for call in calls:
        assert call() == E_INVALID
        assert lib.ppo_last_error()
    torch.cuda.synchronize()
    assert bool((scratch == SENTINEL).all().item()), "a rejected call wrote something"


def test_null_pointers_small_workspace_and_bad_mode_are_rejected():
    geom = (4, 2, 16, 5, 6)
    lib, dev, st = _lib.load(), torch.device("cuda"), _lib.current_stream()
    r = reference(geom)
    x, wt, dy = (r[k].to(dev) for k in ("x", "w", "dy"))
    nbytes = int(lib.ppo_conv3x3s2_any_wgrad_workspace_bytes(*geom))
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
    dw = torch.full(wt.shape, SENTINEL, dtype=torch.float32, device=dev)
    out = torch.full(dy.shape, SENTINEL, dtype=torch.float32, device=dev)
    dx = torch.full(x.shape, SENTINEL, dtype=torch.float32, device=dev)
    fwd, bwd, bww = (lib.ppo_conv3x3s2_any_forward_f32, lib.ppo_conv3x3s2_any_backward_data_f32,
                     lib.ppo_conv3x3s2_any_backward_weight_f32)
    assert bww(_p(x), NONE, _p(dy), _p(dw), None, _p(ws), nbytes - 4, *geom, 0, st) == E_INVALID
    assert bww(_p(x), 3, _p(dy), _p(dw), None, _p(ws), nbytes, *geom, 0, st) == E_INVALID
    assert bww(None, NONE, _p(dy), _p(dw), None, _p(ws), nbytes, *geom, 0, st) == E_INVALID
    assert bww(_p(x), NONE, None, _p(dw), None, _p(ws), nbytes, *geom, 0, st) == E_INVALID
    assert bww(_p(x), NONE, _p(dy), None, None, _p(ws), nbytes, *geom, 0, st) == E_INVALID
    assert bww(_p(x), NONE, _p(dy), _p(dw), None, None, nbytes, *geom, 0, st) == E_INVALID
    assert fwd(_p(x), 3, _p(wt), None, None, _p(out), *geom, st) == E_INVALID
    assert fwd(None, NONE, _p(wt), None, None, _p(out), *geom, st) == E_INVALID
    assert fwd(_p(x), NONE, None, None, None, _p(out), *geom, st) == E_INVALID
    assert fwd(_p(x), NONE, _p(wt), None, None, None, *geom, st) == E_INVALID
    assert bwd(None, _p(wt), None, None, _p(dx), *geom, st) == E_INVALID
    assert bwd(_p(dy), None, None, None, _p(dx), *geom, st) == E_INVALID
    assert bwd(_p(dy), _p(wt), None, None, None, *geom, st) == E_INVALID
    torch.cuda.synchronize()
    assert all(bool((t == SENTINEL).all().item()) for t in (dw, out, dx))
