"""GPU: the signed uint8 preparations (--observation_scaling=centered|unit, PPO_IN_U8_CENTERED / PPO_IN_U8_UNIT) in every
kernel that reads uint8 observations, against tests/obs_scaling_torch.py (the reference's torch expressions).

* All 256 bytes through each load, bit for bit: one-tap probes (a weight tensor that picks one input pixel, or a
  one-hot dy for the weight gradient) turn a convolution into a table look-up of f(byte).
* Padding stays 0.0f: f(0) is -0.5 / -3 under these modes, so a staging path that converts its zero fill is wrong on
  every border pixel of the first layer.  Data from {0, 255} (f = -+0.5 / -+3) with small-integer weights and dy make every
  product and sum exact in float32: forward, conv + pool and weight gradient of the four specialised first-layer
  geometries are bit-equal to float64 at n = 1, n = 3 and the batch that wraps the persistent item loop (where the next
  item's band is prefetched into registers), an all-zero image among them.
* Random bytes against float64 per element at n = 3: |got - ref| <= bar_factor(K) A, A the contraction on |f(x)|.
* The generic 3x3 (stride 1 and 2) and the strided families, the split-bf16 strided forms at their own bar, the
  observation normaliser's three launches and the normed hash inputs.

Outputs sit in sentinel-guarded buffers and every launch runs twice, as in tests/test_conv_float64_gpu.py."""
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
import torch.nn.functional as F  # noqa: E402

import conv_float64_torch as C  # noqa: E402
import hash_numpy as HN  # noqa: E402
import obs_scaling_torch as O  # noqa: E402
from ppo_amd import _lib, hashing  # noqa: E402
from test_conv_float64_gpu import _p, guarded, guards_intact, pack, twice  # noqa: E402

FIRST_LAYERS = [(4, 16, 84, 84), (5, 16, 84, 84), (3, 16, 64, 64), (4, 16, 64, 64)]
IDS = [C.case_id(c) for c in FIRST_LAYERS]
U = 2.0 ** -24


def _env():
    return _lib.load(), torch.device("cuda"), _lib.current_stream()


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()) % (1 << 31))


def every_byte(shape, g):
    """uint8 tensor of `shape` (at least 256 elements) in which every byte value occurs, shuffled."""
    numel = int(np.prod(shape))
    assert numel >= 256
    v = (torch.arange(numel) % 256).to(torch.uint8)
    return v[torch.randperm(numel, generator=g)].view(shape)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ------------------------------------------------------------------------------------------------------------ launches
def run_forward(case, n, xu, wt, b, mode, packed):
    lib, dev, st = _env()
    ck, cm, h, w = case
    src, wdev = xu.to(dev), wt.to(dev)
    if packed:
        wdev = pack(lib, st, wdev, ck, cm, 0)
    fn = lib.ppo_conv3x3_forward_packed_f32 if packed else lib.ppo_conv3x3_forward_f32
    bd = None if b is None else b.to(dev)
    return twice(lambda o: fn(_p(src), mode, _p(wdev), _p(bd), None, _p(o), n, ck, cm, h, w, st), (n, cm, h, w), dev).cpu()


def run_pool(case, n, xu, wt, b, mode, packed, train=True, index=None):
    """-> (pooled, argmax or None) on the CPU; with `index` through the packed + indexed entry point (row i of the launch
    reads image index[i] of xu)."""
    lib, dev, st = _env()
    ck, cm, h, w = case
    ho, wo = (h + 1) // 2, (w + 1) // 2
    src, wdev, bd = xu.to(dev), wt.to(dev), b.to(dev)
    if packed or index is not None:
        wdev = pack(lib, st, wdev, ck, cm, 0)
    idx = None if index is None else index.to(dev)
    runs = []
    for _ in range(2):
        pbuf, p = guarded((n, cm, ho, wo), dev)
        abuf, amx = guarded((n, cm, ho, wo), dev, dtype=torch.uint8, sentinel=255)
        a = _p(amx) if train else None
        if index is not None:
            rc = lib.ppo_conv3x3_pool_forward_packed_indexed_f32(_p(src), _p(idx), mode, _p(wdev), _p(bd), _p(p), a, n, ck, cm, h, w, st)
        elif packed:
            rc = lib.ppo_conv3x3_pool_forward_packed_f32(_p(src), mode, _p(wdev), _p(bd), _p(p), a, n, ck, cm, h, w, st)
        else:
            rc = lib.ppo_conv3x3_pool_forward_f32(_p(src), mode, _p(wdev), _p(bd), _p(p), a, n, ck, cm, h, w, st)
        _lib.check(rc, "pool forward")
        assert guards_intact(pbuf, p) and guards_intact(abuf, amx, 255)
        runs.append((p, amx))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), "two launches differ"
    return runs[0][0].cpu(), (runs[0][1].cpu() if train else None)


def run_wgrad(case, n, xu, dy, mode):
    lib, dev, st = _env()
    ck, cm, h, w = case
    src, dyd = xu.to(dev), dy.to(dev)
    nbytes = int(lib.ppo_conv3x3_wgrad_workspace_bytes(ck, cm))
    results = []
    for fill in (float("nan"), 3.0):
        ws_buf, ws = guarded((nbytes // 4,), dev)
        ws.fill_(fill)
        wbuf, dw = guarded((cm, ck, 3, 3), dev)
        bbuf, db = guarded((cm,), dev)
        _lib.check(lib.ppo_conv3x3_backward_weight_f32(_p(src), mode, _p(dyd), _p(dw), _p(db), _p(ws), nbytes, n, ck, cm, h, w, 0,
                                                       st), "backward_weight")
        assert guards_intact(ws_buf, ws) and guards_intact(wbuf, dw) and guards_intact(bbuf, db)
        results.append((dw.cpu(), db.cpu()))
    assert torch.equal(results[0][0], results[1][0]) and torch.equal(results[0][1], results[1][1]), "two launches differ"
    return results[0]


def check_argmax(amx, c64, p64):
    """Every argmax byte names a tap inside the image that holds the window's maximum."""
    n, cm, h, w = c64.shape
    ho, wo = p64.shape[2:]
    assert int(amx.max()) <= 8
    taps = F.unfold(F.pad(c64, (1, 1, 1, 1), value=float("-inf")).view(n * cm, 1, h + 2, w + 2), 3, stride=2)
    chosen = torch.gather(taps, 1, amx.long().view(n * cm, 1, ho * wo)).view(n, cm, ho, wo)
    assert torch.equal(chosen, p64)


# ---------------------------------------------------------------------------------- 1. all 256 bytes through each load
@pytest.mark.parametrize("scaling", O.SIGNED)
@pytest.mark.parametrize("case", FIRST_LAYERS, ids=IDS)
def test_all_bytes_through_the_forward_band_staging(case, scaling):
    ck, cm, h, w = case
    xu = every_byte((1, ck, h, w), _gen("fwd", case))
    wt = torch.zeros(cm, ck, 3, 3)
    for co in range(cm):
        wt[co, co % ck, 1, 1] = 1.0  # the centre tap of one channel: out[co] = f(x[co % ck])
    want = O.prep(xu, scaling)[:, [co % ck for co in range(cm)]]
    for packed in (False, True):
        got = run_forward(case, 1, xu, wt, None, O.IN_MODE[scaling], packed)
        assert same_bits(got, want), f"{int((got != want).sum())} of {want.numel()} elements differ"


# `accumulators`: the opt-in conv1_pool.hip form (ppo_conv1_pool_form(0)), which has the Atari first layer only
POOL_FORMS = [(c, "lds") for c in FIRST_LAYERS] + [((4, 16, 84, 84), "accumulators")]


@pytest.mark.parametrize("scaling", O.SIGNED)
@pytest.mark.parametrize("case,form", POOL_FORMS, ids=[f"{C.case_id(c)}-{f}" for c, f in POOL_FORMS])
def test_all_bytes_through_the_fused_pool_staging(case, form, scaling):
    """Bytes at the even pixels (the centres of the pooling windows), 0 elsewhere: f is increasing, so a window's maximum
    is f(its centre byte)."""
    ck, cm, h, w = case
    ho, wo = h // 2, w // 2
    xu = torch.zeros((2, ck, h, w), dtype=torch.uint8)
    xu[:, :, ::2, ::2] = every_byte((2, ck, ho, wo), _gen("pool", case))
    wt = torch.zeros(cm, ck, 3, 3)
    for co in range(cm):
        wt[co, co % ck, 1, 1] = 1.0
    want = O.prep(xu, scaling)[:, [co % ck for co in range(cm)]][:, :, ::2, ::2]
    lib = _lib.load()
    before = lib.ppo_conv1_pool_form(0 if form == "accumulators" else 1)
    try:
        for packed, train in ((False, True), (True, False)):
            got, amx = run_pool(case, 2, xu, wt, torch.zeros(cm), O.IN_MODE[scaling], packed, train)
            assert same_bits(got, want), f"{int((got != want).sum())} of {want.numel()} elements differ"
            if train:  # byte 0 at the centre ties with its neighbours: tap 0, 1, 3 or 4 then; any other byte wins alone
                centre = xu[:, [co % ck for co in range(cm)]][:, :, ::2, ::2] > 0
                assert bool((amx[centre] == 4).all())
    finally:
        lib.ppo_conv1_pool_form(before)


@pytest.mark.parametrize("scaling", O.SIGNED)
@pytest.mark.parametrize("case", FIRST_LAYERS, ids=IDS)
def test_all_bytes_through_the_weight_gradient_staging(case, scaling):
    """dy of channel co is 1 at one interior pixel p_co and 0 elsewhere: dw[co, ci, ky, kx] = f(x[ci, p_co + (ky-1, kx-1)])."""
    ck, cm, h, w = case
    g = _gen("wgrad", case)
    xu = torch.randint(0, 256, (1, ck, h, w), generator=g, dtype=torch.uint8)
    spots = [(3 + 6 * (co // 4), 3 + 6 * (co % 4)) for co in range(cm)]
    vals = every_byte((cm, ck, 3, 3), g)
    dy = torch.zeros(1, cm, h, w)
    for co, (y, x) in enumerate(spots):
        xu[0, :, y - 1:y + 2, x - 1:x + 2] = vals[co]
        dy[0, co, y, x] = 1.0
    assert len(set(vals.flatten().tolist())) == 256
    dw, db = run_wgrad(case, 1, xu, dy, O.IN_MODE[scaling])
    assert same_bits(dw, O.prep(vals, scaling)) and torch.equal(db, torch.ones(cm))


@pytest.mark.parametrize("scaling", O.SIGNED)
def test_all_bytes_through_the_generic_and_strided_loads(scaling):
    lib, dev, st = _env()
    mode = O.IN_MODE[scaling]
    # 3x3 at any geometry: 3 -> 5 on 7 x 9, n = 2
    n, cin, cout, h, w = 2, 3, 5, 7, 9
    xu = every_byte((n, cin, h, w), _gen("any"))
    wt = torch.zeros(cout, cin, 3, 3)
    for co in range(cout):
        wt[co, co % cin, 1, 1] = 1.0
    pick = [co % cin for co in range(cout)]
    xd, wd = xu.to(dev), wt.to(dev)
    got = twice(lambda o: lib.ppo_conv3x3_any_forward_f32(_p(xd), mode, _p(wd), None, None, _p(o), n, cin, cout, h, w, st),
                (n, cout, h, w), dev).cpu()
    assert same_bits(got, O.prep(xu, scaling)[:, pick])
    # its stride-2 form reads the even pixels (120 of them): three data sets put every byte at one
    seen = set()
    for part in range(3):
        xs = xu.clone()
        xs[:, :, ::2, ::2] = ((torch.arange(120) + 120 * part) % 256).to(torch.uint8).view(n, cin, 4, 5)
        xsd = xs.to(dev)
        got = twice(lambda o: lib.ppo_conv3x3s2_any_forward_f32(_p(xsd), mode, _p(wd), None, None, _p(o), n, cin, cout, h, w, st),
                    (n, cout, (h + 1) // 2, (w + 1) // 2), dev).cpu()
        assert same_bits(got, O.prep(xs, scaling)[:, pick][:, :, ::2, ::2])
        seen |= set(xs[:, :, ::2, ::2].flatten().tolist())
    assert len(seen) == 256
    # strided: the Nature first layer (8x8 / 4, 32 filters) on 4 x 36 x 36, n = 2; tap (0, 0) of one channel
    n, cin, h, w, cout, k, s = 2, 4, 36, 36, 32, 8, 4
    ho = (h - k) // s + 1
    xu = torch.zeros((n, cin, h, w), dtype=torch.uint8)
    xu[:, :, :ho * s:s, :ho * s:s] = every_byte((n, cin, ho, ho), _gen("strided"))
    wt = torch.zeros(cout, cin, k, k)
    for co in range(cout):
        wt[co, co % cin, 0, 0] = 1.0
    pick = [co % cin for co in range(cout)]
    xd, wd = xu.to(dev), wt.to(dev)
    for name in ("ppo_conv2d_strided_forward_f32",):
        got = twice(lambda o: getattr(lib, name)(_p(xd), mode, _p(wd), None, _p(o), 0, n, cin, h, w, cout, k, k, s, st),
                    (n, cout, ho, ho), dev).cpu()
        assert same_bits(got, O.prep(xu, scaling)[:, pick][:, :, :ho * s:s, :ho * s:s])
    got = twice(lambda o: lib.ppo_conv2d_strided_forward_leaky_f32(_p(xd), mode, _p(wd), None, _p(o), 1.0, n, cin, h, w, cout, k, k, s,
                                                                   st), (n, cout, ho, ho), dev).cpu()
    assert same_bits(got, O.prep(xu, scaling)[:, pick][:, :, :ho * s:s, :ho * s:s])  # slope 1: the identity


# ------------------------------------------------------------------------------------------------ 2. padding stays zero
def two_level(case, n, g):
    """uint8 [n, ck, h, w] from {0, 255}; image 0 all zero when there are several, else a zero frame two pixels wide."""
    ck, cm, h, w = case
    xu = (torch.randint(0, 2, (n, ck, h, w), generator=g) * 255).to(torch.uint8)
    if n > 1:
        xu[0] = 0
    else:
        xu[:, :, :2], xu[:, :, -2:], xu[:, :, :, :2], xu[:, :, :, -2:] = 0, 0, 0, 0
    return xu


def ns(op, case):
    return (1, 3, C.wrapping_n(op, case[2]))


@pytest.mark.parametrize("scaling", O.SIGNED)
@pytest.mark.parametrize("case", FIRST_LAYERS, ids=IDS)
def test_padding_is_zero_in_the_forward(case, scaling):
    ck, cm, h, w = case
    for n in ns("conv", case):
        g = _gen("pad-fwd", case, n)
        xu = two_level(case, n, g)
        wt = torch.randint(-2, 3, (cm, ck, 3, 3), generator=g).float()
        b = torch.randint(-5, 6, (cm,), generator=g).float()
        ref = F.conv2d(O.prep(xu, scaling).double(), wt.double(), b.double(), padding=1)
        got = run_forward(case, n, xu, wt, b, O.IN_MODE[scaling], packed=n != 3)
        bad = got.double() != ref
        assert not bool(bad.any()), f"n={n}: {int(bad.sum())} elements differ, {int(bad[:, :, 1:-1, 1:-1].sum())} of them interior"


@pytest.mark.parametrize("scaling", O.SIGNED)
@pytest.mark.parametrize("case", FIRST_LAYERS, ids=IDS)
def test_padding_is_zero_in_the_fused_pool(case, scaling):
    ck, cm, h, w = case
    lib = _lib.load()
    forms = (1, 0) if case == (4, 16, 84, 84) else (1,)
    for n in ns("pool", case):
        g = _gen("pad-pool", case, n)
        xu = two_level(case, n, g)
        wt = torch.randint(-2, 3, (cm, ck, 3, 3), generator=g).float()
        b = torch.randint(-5, 6, (cm,), generator=g).float()
        c64 = F.conv2d(O.prep(xu, scaling).double(), wt.double(), b.double(), padding=1)
        p64 = F.max_pool2d(c64, 3, 2, 1)
        for form in forms:
            before = lib.ppo_conv1_pool_form(form)
            try:
                got, amx = run_pool(case, n, xu, wt, b, O.IN_MODE[scaling], packed=n != 3)
            finally:
                lib.ppo_conv1_pool_form(before)
            bad = got.double() != p64
            assert not bool(bad.any()), f"n={n} form={form}: {int(bad.sum())} pooled values differ"
            check_argmax(amx, c64, p64)
        if n == 3:  # the minibatch form: rows through an index
            index = torch.tensor([2, 0, 1, 2, 2], dtype=torch.int32)
            got, amx = run_pool(case, 5, xu, wt, b, O.IN_MODE[scaling], True, index=index)
            assert torch.equal(got.double(), p64[index.long()])
            check_argmax(amx, c64[index.long()], p64[index.long()])


@pytest.mark.parametrize("scaling", O.SIGNED)
@pytest.mark.parametrize("case", FIRST_LAYERS, ids=IDS)
def test_padding_is_zero_in_the_weight_gradient(case, scaling):
    ck, cm, h, w = case
    for n in ns("wgrad", case):
        assert 6 * n * h * w < 2 ** 23  # |dy| <= 2, |f| <= 3, halves: every partial sum is exact in float32
        g = _gen("pad-wgrad", case, n)
        xu = two_level(case, n, g)
        dy = torch.randint(-2, 3, (n, cm, h, w), generator=g).float()
        xin = O.prep(xu, scaling)
        rw = torch.nn.grad.conv2d_weight(xin.double(), (cm, ck, 3, 3), dy.double(), padding=1)
        dw, db = run_wgrad(case, n, xu, dy, O.IN_MODE[scaling])
        assert torch.equal(dw.double(), rw), f"n={n}: {int((dw.double() != rw).sum())} of {rw.numel()} elements differ"
        assert torch.equal(db.double(), dy.double().sum((0, 2, 3)))


# --------------------------------------------------------------------------------------- 3. random bytes against float64
def over_bar(got, ref, A, K, tag, factor=C.bar_factor):
    e = (got.double() - ref).abs()
    bar = factor(K) * A
    worst = float((e / bar.clamp_min(1e-300)).max())
    print(f"OBS_SCALING_ERR {tag} K={K} max_err={float(e.max()):.3e} of_bar={worst:.3f}")
    bad = int((e > bar).sum())
    assert bad == 0, f"{tag}: {bad} of {ref.numel()} elements over the bar ({worst:.2f} x)"


@pytest.mark.parametrize("scaling", O.SIGNED)
@pytest.mark.parametrize("case", FIRST_LAYERS, ids=IDS)
def test_random_bytes_against_float64(case, scaling):
    ck, cm, h, w = case
    n, mode = 3, O.IN_MODE[scaling]
    inp = C.forward_inputs(case, n, "plain")
    xu, wt, b = inp["xu"], inp["w"], inp["b"]
    xin = O.prep(xu, scaling)
    K = C.sum_length("forward", case, n)
    ref, A = C.forward_eval(xin, wt, b, None, "f64"), C.forward_eval(xin, wt, b, None, "abs")
    tag = f"{C.case_id(case)} {scaling}"
    for packed in (False, True):
        over_bar(run_forward(case, n, xu, wt, b, mode, packed), ref, A, K, f"{tag} forward packed={packed}")
    # conv + pool: |max a - max b| <= max |a - b|, and the argmax names a tap within twice the bound of the maximum
    bound = C.bar_factor(K) * A
    p64, pbound = F.max_pool2d(ref, 3, 2, 1), F.max_pool2d(bound, 3, 2, 1)
    for packed in (False, True):
        p, amx = run_pool(case, n, xu, wt, b, mode, packed)
        e = (p.double() - p64).abs()
        print(f"OBS_SCALING_ERR {tag} pool packed={packed} max(e/bound)={float((e / pbound).max()):.3e}")
        assert int((e > pbound).sum()) == 0
        assert int(amx.max()) <= 8
        taps = F.unfold(F.pad(ref, (1, 1, 1, 1), value=float("-inf")).view(n * cm, 1, h + 2, w + 2), 3, stride=2)
        chosen = torch.gather(taps, 1, amx.long().view(n * cm, 1, -1)).view(p64.shape)
        assert bool(torch.isfinite(chosen).all()) and int((chosen < p64 - 2.0 * pbound).sum()) == 0
    # weight gradient
    winp = C.backward_weight_inputs(case, n, "plain")
    xin = O.prep(winp["xu"], scaling)
    Kw = C.sum_length("backward_weight", case, n)
    dw, db = run_wgrad(case, n, winp["xu"], winp["dy"], mode)
    (rw, rb), (Aw, Ab) = C.backward_weight_eval(xin, winp["dy"], "f64"), C.backward_weight_eval(xin, winp["dy"], "abs")
    over_bar(dw, rw, Aw, Kw, f"{tag} backward_weight dw")
    over_bar(db, rb, Ab, Kw, f"{tag} backward_weight db")


# ------------------------------------------------------------------------------------------ 4. the other kernel families
@pytest.mark.parametrize("scaling", O.SIGNED)
@pytest.mark.parametrize("stride", [1, 2])
def test_generic_3x3_against_float64(stride, scaling):
    lib, dev, st = _env()
    mode = O.IN_MODE[scaling]
    n, cin, cout, h, w = 2, 3, 5, 7, 9
    ho, wo = ((h + 1) // 2, (w + 1) // 2) if stride == 2 else (h, w)
    g = _gen("any64", stride)
    xu = torch.randint(0, 256, (n, cin, h, w), generator=g, dtype=torch.uint8)
    xu[0, :, 0] = 0  # zeros on a border
    wt, b = torch.randn(cout, cin, 3, 3, generator=g) / 5, torch.randn(cout, generator=g)
    dy = torch.randn(n, cout, ho, wo, generator=g)
    xin = O.prep(xu, scaling)
    family = "ppo_conv3x3s2_any" if stride == 2 else "ppo_conv3x3_any"
    xd, wd, bd, dyd = xu.to(dev), wt.to(dev), b.to(dev), dy.to(dev)
    got = twice(lambda o: getattr(lib, family + "_forward_f32")(_p(xd), mode, _p(wd), _p(bd), None, _p(o), n, cin, cout, h, w, st),
                (n, cout, ho, wo), dev).cpu()
    ref = F.conv2d(xin.double(), wt.double(), b.double(), stride=stride, padding=1)
    A = F.conv2d(xin.double().abs(), wt.double().abs(), b.double().abs(), stride=stride, padding=1)
    over_bar(got, ref, A, 9 * cin, f"{family} {scaling} forward")
    nbytes = int(getattr(lib, family + "_wgrad_workspace_bytes")(n, cin, cout, h, w))
    outs = []
    for _ in range(2):
        ws_buf, ws = guarded((max(nbytes // 4, 1),), dev)
        wbuf, dw = guarded((cout, cin, 3, 3), dev)
        bbuf, db = guarded((cout,), dev)
        _lib.check(getattr(lib, family + "_backward_weight_f32")(_p(xd), mode, _p(dyd), _p(dw), _p(db), _p(ws), nbytes, n, cin, cout,
                                                                h, w, 0, st), "backward_weight")
        assert guards_intact(ws_buf, ws) and guards_intact(wbuf, dw) and guards_intact(bbuf, db)
        outs.append((dw.cpu(), db.cpu()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    rw = torch.nn.grad.conv2d_weight(xin.double(), (cout, cin, 3, 3), dy.double(), stride=stride, padding=1)
    Aw = torch.nn.grad.conv2d_weight(xin.double().abs(), (cout, cin, 3, 3), dy.double().abs(), stride=stride, padding=1)
    over_bar(outs[0][0], rw, Aw, n * ho * wo, f"{family} {scaling} backward_weight")
    assert torch.allclose(outs[0][1].double(), dy.double().sum((0, 2, 3)), rtol=0, atol=float(C.bar_factor(n * ho * wo) * dy.abs().sum()))
    # {0, 255} and small integers: exact, so a converted padding tap (f(0) instead of 0) is a hard mismatch
    xq = (torch.randint(0, 2, (n, cin, h, w), generator=g) * 255).to(torch.uint8)
    xq[0] = 0
    wq = torch.randint(-2, 3, (cout, cin, 3, 3), generator=g).float()
    xqd, wqd = xq.to(dev), wq.to(dev)
    got = twice(lambda o: getattr(lib, family + "_forward_f32")(_p(xqd), mode, _p(wqd), None, None, _p(o), n, cin, cout, h, w, st),
                (n, cout, ho, wo), dev).cpu()
    assert torch.equal(got.double(), F.conv2d(O.prep(xq, scaling).double(), wq.double(), None, stride=stride, padding=1))


def strided_bar_bf16x3(K):
    """tests/conv_strided_split_torch.py: the split's dropped terms plus float32 summation with one more rounding."""
    return 2.0 ** -15 + 2.0 * (K + 4) * U


@pytest.mark.parametrize("scaling", O.SIGNED)
@pytest.mark.parametrize("suffix", ["f32", "bf16x3"])
def test_strided_nature_first_layer_against_float64(suffix, scaling):
    lib, dev, st = _env()
    mode = O.IN_MODE[scaling]
    n, cin, h, w, cout, k, s = 2, 4, 36, 36, 32, 8, 4
    ho = (h - k) // s + 1
    geom = (n, cin, h, w, cout, k, k, s)
    factor = C.bar_factor if suffix == "f32" else strided_bar_bf16x3
    g = _gen("strided64")
    xu = torch.randint(0, 256, (n, cin, h, w), generator=g, dtype=torch.uint8)
    wt, b = torch.randn(cout, cin, k, k, generator=g) / 16, torch.randn(cout, generator=g) / 4
    dy = torch.randn(n, cout, ho, ho, generator=g)
    xin = O.prep(xu, scaling)
    xd, wd, bd, dyd = xu.to(dev), wt.to(dev), b.to(dev), dy.to(dev)
    pre = F.conv2d(xin.double(), wt.double(), b.double(), stride=s)
    A = F.conv2d(xin.double().abs(), wt.double().abs(), b.double().abs(), stride=s)
    for relu in (0, 1):
        got = twice(lambda o: getattr(lib, f"ppo_conv2d_strided_forward_{suffix}")(_p(xd), mode, _p(wd), _p(bd), _p(o), relu, *geom, st),
                    (n, cout, ho, ho), dev).cpu()
        over_bar(got, torch.relu(pre) if relu else pre, A, cin * k * k, f"strided_{suffix} {scaling} forward relu={relu}", factor)
    gate = torch.relu(pre).float()
    gd = gate.to(dev)
    gdy = torch.where(gate > 0, dy, torch.zeros_like(dy))
    nbytes = int(lib.ppo_conv2d_strided_wgrad_workspace_bytes(*geom))
    outs = []
    for _ in range(2):
        ws_buf, ws = guarded((nbytes // 4,), dev)
        wbuf, dw = guarded((cout, cin, k, k), dev)
        bbuf, db = guarded((cout,), dev)
        _lib.check(getattr(lib, f"ppo_conv2d_strided_backward_weight_{suffix}")(_p(xd), mode, _p(dyd), _p(gd), _p(dw), _p(db), _p(ws),
                                                                               nbytes, *geom, st), "backward_weight")
        assert guards_intact(ws_buf, ws) and guards_intact(wbuf, dw) and guards_intact(bbuf, db)
        outs.append((dw.cpu(), db.cpu()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    rw = torch.nn.grad.conv2d_weight(xin.double(), (cout, cin, k, k), gdy.double(), stride=s)
    Aw = torch.nn.grad.conv2d_weight(xin.double().abs(), (cout, cin, k, k), gdy.double().abs(), stride=s)
    over_bar(outs[0][0], rw, Aw, n * ho * ho, f"strided_{suffix} {scaling} backward_weight", factor)
    over_bar(outs[0][1], gdy.double().sum((0, 2, 3)), gdy.double().abs().sum((0, 2, 3)), n * ho * ho,
             f"strided_{suffix} {scaling} bias", factor)


# --------------------------------------------------------------------------------------------- 5. normaliser and hashing
@pytest.mark.parametrize("scaling", O.SCALINGS)
def test_normaliser_launches_match_torch(scaling):
    lib, dev, st = _env()
    code = O.OBS_PREP[scaling]
    C_, H, W, B = 2, 12, 12, 37
    Fd = C_ * H * W
    g = _gen("norm")
    x = every_byte((B, C_, H, W), g)
    xin = O.prep(x, scaling)
    lo, hi = float(xin.min()), float(xin.max())
    mu = (torch.rand(Fd, generator=g) * (hi - lo) + lo).float()
    std = (torch.rand(Fd, generator=g) * 0.25 * (hi - lo) + 0.02).float()
    eps = 0.003
    want = torch.clamp((xin.view(B, Fd) - mu) / (std + eps), -5, 5)
    assert 0 < int((want.abs() == 5).sum()) < want.numel()  # the clamp is reached, and is not all there is
    mud, stdd = mu.to(dev), std.to(dev)
    # an aligned copy (four bytes per lane) and one a byte off (one byte per lane)
    flat = torch.zeros(x.numel() + 1, dtype=torch.uint8, device=dev)
    flat[1:].copy_(x.view(-1))
    for xd in (x.to(dev), flat[1:].view(B, C_, H, W)):
        mbuf, mom = guarded((2 * Fd,), dev, dtype=torch.float64, sentinel=-7.25e30)
        _lib.check(lib.ppo_obs_moments_f64(_p(xd), code, B, Fd, _p(mom), st), "moments")
        assert guards_intact(mbuf, mom, -7.25e30)
        s1, s2 = xin.double().view(B, Fd).sum(0), xin.double().view(B, Fd).pow(2).sum(0)
        assert torch.equal(mom[:Fd].cpu(), s1)  # 24-bit terms, 37 of them: the float64 sum is exact
        assert torch.allclose(mom[Fd:].cpu(), s2, rtol=(B + 1) * 2.0 ** -53, atol=0)
        got = twice(lambda o: lib.ppo_obs_normalize_f32(_p(xd), code, _p(mud), _p(stdd), eps, _p(o), B, Fd, st), (B, Fd), dev).cpu()
        assert same_bits(got, want)
        for channel in (0, C_ - 1):
            sl = slice(channel * H * W, (channel + 1) * H * W)
            got = twice(lambda o: lib.ppo_obs_normalize_channel_f32(_p(xd), code, None, _p(mud), _p(stdd), eps, _p(o), B, C_, H, W,
                                                                    channel, st), (B, 1, H, W), dev).cpu()
            assert same_bits(got.view(B, H * W), want[:, sl])
            index = torch.tensor([5, 0, 36, 5, 17], dtype=torch.int32)
            idx = index.to(dev)
            got = twice(lambda o: lib.ppo_obs_normalize_channel_f32(_p(xd), code, _p(idx), _p(mud), _p(stdd), eps, _p(o), 5, C_, H, W,
                                                                    channel, st), (5, 1, H, W), dev).cpu()
            assert same_bits(got.view(5, H * W), want[index.long()][:, sl])


def hash_input(obs, planes, mode, scaling, quantize, mu, std, eps):
    """The normed hash inputs of tests/hash_numpy.py with prep_for_model's scaling applied to the byte first."""
    o = np.asarray(obs)
    if quantize:
        o = o - o % np.uint8(quantize)
    o = o[:, :planes].reshape(o.shape[0], -1)
    p = o.astype(np.float32) / np.float32(255)
    if scaling != "scaled":
        p = p - np.float32(0.5)
    if scaling == "unit":
        p = p * np.float32(6)
    d = o.shape[1]
    m, s = (np.asarray(a, np.float32).reshape(-1)[:d] for a in (mu, std))
    x = np.clip((p - m) / (s + np.float32(eps)), np.float32(-5), np.float32(5))
    assert x.dtype == np.float32
    return x if mode == "normed" else x + np.float32(3)


class Norm:
    """What hash_observations reads of an ObsNormalizer."""

    def __init__(self, mu, std, eps, scaling):
        self.mu, self.std = (torch.from_numpy(np.ascontiguousarray(a, np.float32).reshape(-1)).cuda() for a in (mu, std))
        self.norm_eps, self.F, self.observation_scaling = float(eps), self.mu.numel(), scaling


@pytest.mark.parametrize("scaling", O.SCALINGS)
@pytest.mark.parametrize("shape,planes,B", [((2, 12, 12), 1, 37), ((2, 12, 12), 2, 5), ((3, 5, 7), 3, 37)])
def test_normed_hashes_match_numpy(shape, planes, B, scaling):
    rng = np.random.default_rng(sum(shape) * 100 + B)
    obs = rng.integers(0, 256, (B, *shape), dtype=np.uint8)
    k = {"scaled": 1.0, "centered": 1.0, "unit": 6.0}[scaling]
    off = 0.0 if scaling == "scaled" else 0.5
    mu = ((rng.uniform(0.2, 0.6, shape) - off) * k).astype(np.float32)
    std = (rng.uniform(0.05, 0.3, shape) * k).astype(np.float32)
    pad = np.zeros((1, *shape), np.uint8) + 7
    dev = torch.from_numpy(np.concatenate([pad, obs, pad])).cuda()[1:1 + B]
    for mode, q, bias, bits in (("normed", 1, 0.0, 5), ("normed_offset", 8, 0.5, 16), ("normed", 0, 0.5, 24)):
        h = hashing.LinearStateHasher((planes, *shape[1:]), bits, device="cuda", bias=bias)
        out = torch.full((B + 2,), -7, dtype=torch.int32, device="cuda")
        h.hash_observations(dev, out=out[1:B + 1], quantize=q, mode=mode, norm=Norm(mu, std, 0.003, scaling))
        assert int(out[0]) == -7 and int(out[-1]) == -7
        got = out[1:B + 1].cpu().numpy()
        want, p, bound = HN.project(hash_input(obs, planes, mode, scaling, q, mu, std, 0.003), h.weight.cpu().numpy(),
                                    h.bias.cpu().numpy())
        assert not (np.abs(p) <= bound).any(), "an input of this test lies inside the rounding bound: pick another seed"
        assert np.array_equal(got, want), (mode, q, bias, bits, np.flatnonzero(got != want))
        assert np.array_equal(got, h.hash_observations(dev, quantize=q, mode=mode, norm=Norm(mu, std, 0.003, scaling)).cpu().numpy())
        if scaling != "scaled":  # and it is not what the scaled preparation hashes to
            other = HN.project(hash_input(obs, planes, mode, "scaled", q, mu, std, 0.003), h.weight.cpu().numpy(), h.bias.cpu().numpy())[0]
            assert bits < 16 or not np.array_equal(want, other)
