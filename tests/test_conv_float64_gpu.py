"""GPU: the exact-float32 3x3 convolution anchors - ppo_conv3x3_forward_f32, ppo_conv3x3_backward_data_f32,
ppo_conv3x3_backward_weight_f32, ppo_conv3x3_pool_forward_f32 and their _packed forms, the launches every fused form is
tested bit-identical to - against float64 on the same tensors, per element (tests/conv_float64_torch.py has the
references, the data sets and the cases; tests/test_conv_float64_cpu.py checks, without a GPU, that the bars below mean
something).

Per-element bar, no element left out: |got - ref| <= 2 (K + 3) 2^-24 A, with A the same contraction on absolute values
(+ |bias|, |residual|, |dres|) and K the sum length: a wrong small output next to large ones cannot hide.
Aggregate bar: rms(e / A) of the kernel <= 4 x that of plain float32 torch on the CPU on the same tensors (the 4 for the
different summation tree), wherever the CPU test finds an emulated bf16 split 10 x worse: a dispatch that took a
reduced-precision path fails it.  Integer data: bit-equal to float64 at n = 3 and at a batch that wraps the persistent
item loop, which a dropped or doubled item cannot pass.  Every output sits inside a sentinel-filled buffer, which must
survive around it; every launch runs twice and must give the same bits.

Prints CONV64_ERR <case> <what> max(e/A) rms(e/A) and the ratio to float32's rms; profiles/conv_exact_float64.md
records them."""
import ctypes

import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
import torch.nn.functional as F  # noqa: E402

import conv_float64_torch as C  # noqa: E402
from ppo_amd import _lib  # noqa: E402

NONE, RELU, U8 = C.NONE, C.RELU, C.U8
MODE_NAME = {NONE: "none", RELU: "relu", U8: "u8"}
PAD = 4096       # sentinel elements on either side of an output
SENTINEL = -7.25e30
FWD_CASES = [c for c in C.CASES if C.table(c)["forward"]]
BWD_CASES = [c for c in C.CASES if C.table(c)["backward_data"]]
WG_CASES = [c for c in C.CASES if C.table(c)["backward_weight"]]
POOL_CASES = [c for c in C.CASES if C.table(c)["pool"]]
# the float geometries whose launches have a 16-byte and a narrow epilogue (launch_conv, csrc/conv3x3.hip: channel planes
# and bands that are whole float4s)
WIDE_CASES = [c for c in C.CASES if c[2] not in (21, 11)]
# (n, data set, packed weights): n = 3 on both data sets with raw and packed weights; n = 1 and the wrapping n ("wrap")
# with one mode, packed weights, plain data
SETUPS = [(3, "plain", False), (3, "plain", True), (3, "ranged", False), (3, "ranged", True), (1, "plain", True),
          ("wrap", "plain", True)]


def _ids(cases):
    return [C.case_id(c) for c in cases]


def _sid(s):
    return "-".join(str(v) if not isinstance(v, bool) else ("packed" if v else "raw") for v in s)


def _p(t):
    return None if t is None else t.data_ptr()


def _env():
    return _lib.load(), torch.device("cuda"), _lib.current_stream()


def guarded(shape, dev, shift=0, dtype=torch.float32, sentinel=SENTINEL):
    """An output of `shape` inside a sentinel-filled buffer, `shift` elements past the buffer's (256-byte aligned) start
    + PAD: (whole buffer, the output view)."""
    numel = 1
    for s in shape:
        numel *= s
    buf = torch.full((PAD + shift + numel + PAD,), sentinel, dtype=dtype, device=dev)
    return buf, buf[PAD + shift:PAD + shift + numel].view(shape)


def guards_intact(buf, out, sentinel=SENTINEL):
    lo = (out.data_ptr() - buf.data_ptr()) // buf.element_size()
    hi = lo + out.numel()
    return bool((buf[:lo] == sentinel).all().item()) and bool((buf[hi:] == sentinel).all().item())


def shifted(t, shift):
    """A copy of t whose first element sits `shift` floats past a 256-byte boundary."""
    if t is None or shift == 0:
        return t
    buf = torch.empty(t.numel() + 8, dtype=t.dtype, device=t.device)
    v = buf[shift:shift + t.numel()].view(t.shape)
    v.copy_(t)
    return v


def twice(launch, shape, dev, shift=0):
    """Run launch(out) into two guarded buffers; the guards hold and the bits agree.  Returns the result."""
    outs = []
    for _ in range(2):
        buf, out = guarded(shape, dev, shift)
        _lib.check(launch(out), "launch")
        assert guards_intact(buf, out), "wrote outside its output"
        outs.append(out)
    assert torch.equal(outs[0], outs[1]), "two launches on the same inputs differ"
    assert not bool((outs[0] == SENTINEL).any().item()), "an output element was never written"
    return outs[0]


def judge(tag, got, ref, A, K, f32, aggregate=True):
    """The per-element bar on every element, and (aggregate) rms(e/A) <= 4 x float32's."""
    mx, rms, bad = C.err_stats(got.detach().cpu(), ref, A, K)
    r32 = C.err_stats(f32, ref, A, K)[1]
    ratio = rms / max(r32, 1e-300)
    print(f"CONV64_ERR {tag} K={K} max={mx:.3e} rms={rms:.3e} f32_rms={r32:.3e} ratio={ratio:.2f} "
          f"bar={C.bar_factor(K):.3e} aggregate={'yes' if aggregate else 'no'}")
    assert bad == 0, f"{tag}: {bad} of {ref.numel()} elements over the bar, max e/A {mx:.3e} > {C.bar_factor(K):.3e}"
    if aggregate:
        assert rms <= 4.0 * r32, f"{tag}: rms(e/A) {rms:.3e} is {ratio:.1f} x float32's {r32:.3e}"


def pack(lib, st, wt, cin, cout, transposed):
    pf = torch.full((lib.ppo_conv3x3_packed_floats(cin, cout, transposed),), float("nan"), device=wt.device)
    jobs = (_lib.PackJob * 1)(_lib.PackJob(_p(wt), _p(pf), cin, cout, transposed))
    _lib.check(lib.ppo_conv3x3_pack_weights_f32(ctypes.addressof(jobs), 1, st), "pack")
    return pf


def _resolve_n(n, op, case):
    return C.wrapping_n(op, case[2]) if n == "wrap" else n


def forward_variants(case, every):
    """(what, mode, bias?, residual?): every admitted form, or the one that exercises most (ReLU on load + residual
    where there is one; the float input - the double-buffered loop - for the first layer)."""
    modes = C.admitted(case)["forward"]
    v = [("bias", NONE, True, False), ("nobias", NONE, False, False)]
    if RELU in modes:
        v.append(("relu_residual", RELU, True, True))
    if U8 in modes:
        v.append(("u8", U8, True, False))
    if every:
        return v
    return [v[2]] if RELU in modes else [v[0]]


def run_forward(lib, st, dev, case, n, inp, mode, wdev, packed, b, res, shift=0):
    ck, cm, h, w = case
    src = (inp["xu"] if mode == U8 else inp["x"]).to(dev)
    fn = lib.ppo_conv3x3_forward_packed_f32 if packed else lib.ppo_conv3x3_forward_f32
    bd = None if b is None else b.to(dev)
    rd = None if res is None else shifted(res.to(dev), shift)
    return twice(lambda o: fn(_p(src), mode, _p(wdev), _p(bd), _p(rd), _p(o), n, ck, cm, h, w, st), (n, cm, h, w), dev, shift)


@pytest.mark.parametrize("setup", SETUPS, ids=_sid)
@pytest.mark.parametrize("case", FWD_CASES, ids=_ids(FWD_CASES))
def test_forward_per_element(case, setup):
    lib, dev, st = _env()
    n, data, packed = setup
    every = n == 3
    n = _resolve_n(n, "conv", case)
    ck, cm, h, w = case
    inp = C.forward_inputs(case, n, data)
    K = C.sum_length("forward", case, n)
    wdev = inp["w"].to(dev)
    if packed:
        wdev = pack(lib, st, wdev, ck, cm, 0)
    for what, mode, bias, residual in forward_variants(case, every):
        xin = C.loaded(inp, mode)
        b, res = (inp["b"] if bias else None), (inp["res"] if residual else None)
        got = run_forward(lib, st, dev, case, n, inp, mode, wdev, packed, b, res)
        ref, A = C.forward_eval(xin, inp["w"], b, res, "f64"), C.forward_eval(xin, inp["w"], b, res, "abs")
        judge(f"{C.case_id(case)} forward_{what} {_sid(setup)} n={n}", got, ref, A, K, C.forward_eval(xin, inp["w"], b, res, "f32"))


def run_backward_data(lib, st, dev, case, n, inp, wdev, packed, gated, shift=0):
    ck, cm, h, w = case
    dy = inp["dy"].to(dev)
    src = shifted(inp["relu_src"].to(dev), shift) if gated else None
    dres = shifted(inp["dres"].to(dev), shift) if gated else None
    fn = lib.ppo_conv3x3_backward_data_packed_f32 if packed else lib.ppo_conv3x3_backward_data_f32
    # the entry point's (cin, cout) = (cm, ck): it contracts over the forward's output channels
    return twice(lambda o: fn(_p(dy), _p(wdev), _p(src), _p(dres), _p(o), n, cm, ck, h, w, st), (n, cm, h, w), dev, shift)


@pytest.mark.parametrize("setup", SETUPS, ids=_sid)
@pytest.mark.parametrize("case", BWD_CASES, ids=_ids(BWD_CASES))
def test_backward_data_per_element(case, setup):
    lib, dev, st = _env()
    assert C.admitted(case)["backward_data"]
    n, data, packed = setup
    every = n == 3
    n = _resolve_n(n, "conv", case)
    ck, cm, h, w = case
    inp = C.backward_data_inputs(case, n, data)
    K = C.sum_length("backward_data", case, n)
    wdev = inp["w"].to(dev)
    if packed:
        wdev = pack(lib, st, wdev, cm, ck, 1)
    for gated in ((False, True) if every else (True,)):
        src, dres = (inp["relu_src"], inp["dres"]) if gated else (None, None)
        got = run_backward_data(lib, st, dev, case, n, inp, wdev, packed, gated)
        ref = C.backward_data_eval(inp["dy"], inp["w"], src, dres, "f64")
        A = C.backward_data_eval(inp["dy"], inp["w"], src, dres, "abs")
        f32 = C.backward_data_eval(inp["dy"], inp["w"], src, dres, "f32")
        judge(f"{C.case_id(case)} backward_data_{'gated_dres' if gated else 'plain'} {_sid(setup)} n={n}", got, ref, A, K, f32)
        if gated:  # where the gate is off the result is dres, bit for bit
            off = (inp["relu_src"] <= 0)
            assert bool(off.any()) and torch.equal(got.cpu()[off], inp["dres"][off])


def run_backward_weight(lib, st, dev, case, n, src, dy, mode):
    """accumulate 0 (twice, on workspaces filled differently), then accumulate 1 on the result, then dbias null.
    -> (dw, db) of the first launch."""
    ck, cm, h, w = case
    nbytes = int(lib.ppo_conv3x3_wgrad_workspace_bytes(ck, cm))
    fn = lib.ppo_conv3x3_backward_weight_f32
    results = []
    for fill in (float("nan"), 3.0):  # whatever the workspace held must not matter
        ws_buf, ws = guarded((nbytes // 4,), dev)
        ws.fill_(fill)
        wbuf, dw = guarded((cm, ck, 3, 3), dev)
        bbuf, db = guarded((cm,), dev)
        _lib.check(fn(_p(src), mode, _p(dy), _p(dw), _p(db), _p(ws), nbytes, n, ck, cm, h, w, 0, st), "backward_weight")
        assert guards_intact(ws_buf, ws) and guards_intact(wbuf, dw) and guards_intact(bbuf, db)
        results.append((dw.clone(), db.clone()))
    assert torch.equal(results[0][0], results[1][0]) and torch.equal(results[0][1], results[1][1]), \
        "two weight-gradient launches on the same inputs differ"
    # accumulate: the same sum added to what is there (x + x is exact in float32)
    _lib.check(fn(_p(src), mode, _p(dy), _p(dw), _p(db), _p(ws), nbytes, n, ck, cm, h, w, 1, st), "backward_weight accumulate")
    assert guards_intact(wbuf, dw) and guards_intact(bbuf, db)
    assert torch.equal(dw, 2.0 * results[0][0]) and torch.equal(db, 2.0 * results[0][1])
    # dbias is nullable: dw as before, db untouched
    _lib.check(fn(_p(src), mode, _p(dy), _p(dw), None, _p(ws), nbytes, n, ck, cm, h, w, 0, st), "backward_weight without dbias")
    assert guards_intact(wbuf, dw) and guards_intact(bbuf, db)
    assert torch.equal(dw, results[0][0]) and torch.equal(db, 2.0 * results[0][1])
    return results[0]


def assert_wgrad_wraps(lib, st, dev, case, n, src, dy, mode):
    """The slab launch of the same geometry reports its grid: more items than workgroups, so some took a second one."""
    ck, cm, h, w = case
    nbytes = int(lib.ppo_conv3x3_wgrad_workspace_bytes(ck, cm))
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
    n_slabs = ctypes.c_int(0)
    _lib.check(lib.ppo_conv3x3_backward_weight_slabs_f32(_p(src), mode, _p(dy), _p(ws), nbytes, n, ck, cm, h, w,
                                                         ctypes.addressof(n_slabs), st), "slabs")
    torch.cuda.synchronize()
    assert 0 < n_slabs.value < n * C.nbands("wgrad", h), (n_slabs.value, n * C.nbands("wgrad", h))


@pytest.mark.parametrize("setup", [(3, "plain"), (3, "ranged"), (1, "plain"), ("wrap", "plain")], ids=_sid)
@pytest.mark.parametrize("case", WG_CASES, ids=_ids(WG_CASES))
def test_backward_weight_per_element(case, setup):
    lib, dev, st = _env()
    n0, data = setup
    n = _resolve_n(n0, "wgrad", case)
    modes = C.admitted(case)["backward_weight"]
    if n0 != 3:  # one mode: ReLU on load where there is one, else the float input (the double-buffered loop)
        modes = (RELU,) if RELU in modes else (NONE,)
    inp = C.backward_weight_inputs(case, n, data)
    K = C.sum_length("backward_weight", case, n)
    dy = inp["dy"].to(dev)
    for mode in modes:
        src = (inp["xu"] if mode == U8 else inp["x"]).to(dev)
        dw, db = run_backward_weight(lib, st, dev, case, n, src, dy, mode)
        xin = C.loaded(inp, mode)
        (rw, rb), (Aw, Ab) = C.backward_weight_eval(xin, inp["dy"], "f64"), C.backward_weight_eval(xin, inp["dy"], "abs")
        fw, fb = C.backward_weight_eval(xin, inp["dy"], "f32")
        tag = f"{C.case_id(case)} backward_weight_{MODE_NAME[mode]} {_sid(setup)} n={n}"
        judge(tag + " dw", dw, rw, Aw, K, fw, aggregate=(C.case_id(case), n) in C.WGRAD_AGGREGATE)
        judge(tag + " db", db, rb, Ab, K, fb, aggregate=False)
        if n0 == "wrap":
            assert_wgrad_wraps(lib, st, dev, case, n, src, dy, mode)


def _integer_ops(case):
    a = C.admitted(case)
    return [op for op in ("forward", "backward_data", "backward_weight") if a[op]]


@pytest.mark.parametrize("n0", [3, "wrap"])
@pytest.mark.parametrize("case,op", [(c, op) for c in C.CASES for op in _integer_ops(c)],
                         ids=[f"{C.case_id(c)}-{op}" for c in C.CASES for op in _integer_ops(c)])
def test_integer_data_is_bit_equal_to_float64(case, op, n0):
    """Operands in [-2, 2] make every product and partial sum exact in float32 at every n used
    (test_integer_sets_are_exact_in_float32): a wrong operand map, and an item of the persistent loop dropped or taken
    twice, is a hard mismatch - in the weight gradient too, where no tolerance could show it.  Raw weights at n = 3,
    packed at the wrapping n."""
    lib, dev, st = _env()
    ck, cm, h, w = case
    n = _resolve_n(n0, "wgrad" if op == "backward_weight" else "conv", case)
    packed = n0 == "wrap"
    assert C.integer_bound(op, case, n) < 2 ** 24
    if op == "forward":
        inp = C.forward_inputs(case, n, "integers")
        mode = RELU if RELU in C.admitted(case)["forward"] else NONE
        wdev = inp["w"].to(dev)
        wdev = pack(lib, st, wdev, ck, cm, 0) if packed else wdev
        got = run_forward(lib, st, dev, case, n, inp, mode, wdev, packed, inp["b"], inp["res"])
        ref = C.forward_eval(C.loaded(inp, mode), inp["w"], inp["b"], inp["res"], "f64")
        assert torch.equal(got.cpu().double(), ref)
    elif op == "backward_data":
        inp = C.backward_data_inputs(case, n, "integers")
        wdev = inp["w"].to(dev)
        wdev = pack(lib, st, wdev, cm, ck, 1) if packed else wdev
        got = run_backward_data(lib, st, dev, case, n, inp, wdev, packed, True)
        ref = C.backward_data_eval(inp["dy"], inp["w"], inp["relu_src"], inp["dres"], "f64")
        assert torch.equal(got.cpu().double(), ref)
    else:
        inp = C.backward_weight_inputs(case, n, "integers")
        modes = C.admitted(case)["backward_weight"]
        mode = RELU if RELU in modes else NONE
        src, dy = inp["x"].to(dev), inp["dy"].to(dev)
        dw, db = run_backward_weight(lib, st, dev, case, n, src, dy, mode)
        rw, rb = C.backward_weight_eval(C.loaded(inp, mode), inp["dy"], "f64")
        assert torch.equal(dw.cpu().double(), rw) and torch.equal(db.cpu().double(), rb)
        if n0 == "wrap":
            assert_wgrad_wraps(lib, st, dev, case, n, src, dy, mode)


@pytest.mark.parametrize("packed", [False, True], ids=["raw", "packed"])
@pytest.mark.parametrize("setup", [(3, "plain"), (3, "ranged"), ("wrap", "plain")], ids=_sid)
@pytest.mark.parametrize("case", POOL_CASES, ids=_ids(POOL_CASES))
def test_fused_pool_against_float64(case, setup, packed):
    """ppo_conv3x3_pool_forward_f32 / _packed_f32.  With B = the per-element bound map of the convolution: every pooled
    value is within max-pool(B) of the float64 pooled value (|max a - max b| <= max |a - b|), and every argmax byte names
    a tap inside the image whose float64 value is within 2 max-pool(B) of the window's float64 maximum (the kernel's tap
    t beat the true winner s in float32: c_t >= k_t - B_t >= k_s - B_t >= c_s - B_s - B_t).  No window is excluded."""
    lib, dev, st = _env()
    n0, data = setup
    n = _resolve_n(n0, "pool", case)
    ck, cm, h, w = case
    ho, wo = (h + 1) // 2, (w + 1) // 2
    modes = C.admitted(case)["pool"] if n0 == 3 else (NONE,)
    inp = C.forward_inputs(case, n, data)
    K = C.sum_length("forward", case, n)
    wdev = inp["w"].to(dev)
    if packed:
        wdev = pack(lib, st, wdev, ck, cm, 0)
    fn = lib.ppo_conv3x3_pool_forward_packed_f32 if packed else lib.ppo_conv3x3_pool_forward_f32
    b = inp["b"].to(dev)
    for mode in modes:
        src = (inp["xu"] if mode == U8 else inp["x"]).to(dev)
        runs = []
        for _ in range(2):
            pbuf, p = guarded((n, cm, ho, wo), dev)
            abuf, amx = guarded((n, cm, ho, wo), dev, dtype=torch.uint8, sentinel=255)
            _lib.check(fn(_p(src), mode, _p(wdev), _p(b), _p(p), _p(amx), n, ck, cm, h, w, st), "pool forward")
            assert guards_intact(pbuf, p) and guards_intact(abuf, amx, 255)
            runs.append((p, amx))
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), "two launches differ"
        p, amx = runs[0][0].cpu().double(), runs[0][1].cpu()
        xin = C.loaded(inp, mode)
        c64 = C.forward_eval(xin, inp["w"], inp["b"], None, "f64")
        bound = C.bar_factor(K) * C.forward_eval(xin, inp["w"], inp["b"], None, "abs")
        p64, pbound = F.max_pool2d(c64, 3, 2, 1), F.max_pool2d(bound, 3, 2, 1)
        e = (p - p64).abs()
        bad = int((e > pbound).sum())
        print(f"CONV64_ERR {C.case_id(case)} pool_{MODE_NAME[mode]} {_sid(setup)}-{'packed' if packed else 'raw'} n={n} "
              f"max(e/bound)={float((e / pbound).max()):.3e}")
        assert bad == 0, f"{bad} pooled values outside the bound"
        assert int(amx.max()) <= 8, "an argmax byte is no tap"
        taps = F.unfold(F.pad(c64, (1, 1, 1, 1), value=float("-inf")).view(n * cm, 1, h + 2, w + 2), 3, stride=2)
        assert taps.shape == (n * cm, 9, ho * wo)
        chosen = torch.gather(taps, 1, amx.long().view(n * cm, 1, ho * wo)).view(n, cm, ho, wo)
        assert bool(torch.isfinite(chosen).all()), "an argmax byte names a tap in the padding"
        short = int((chosen < p64 - 2.0 * pbound).sum())
        assert short == 0, f"{short} windows whose argmax names a tap that is not the maximum within rounding"


@pytest.mark.parametrize("case", WIDE_CASES, ids=_ids(WIDE_CASES))
def test_narrow_epilogue_of_the_wide_geometries(case):
    """launch_conv takes the 16-byte epilogue only when out, residual and relu_src are 16-byte aligned; otherwise the
    scalar one, whose loads and stores are single floats (4-byte alignment is all it needs: buffer_f32 reads and plain
    float stores).  torch allocations are always aligned, so that instantiation is reached here by placing out / dx and
    residual / dres / relu_src one float past a 16-byte boundary (in, dy and the weights stay aligned: the band staging
    reads them 16 bytes at a time).  Same arithmetic, so the bits equal the aligned result's; the bar and the guards as
    everywhere."""
    lib, dev, st = _env()
    n, data = 3, "plain"
    ck, cm, h, w = case
    adm = C.admitted(case)
    if adm["forward"]:
        inp = C.forward_inputs(case, n, data)
        mode = RELU if RELU in adm["forward"] else NONE
        wdev = inp["w"].to(dev)
        wide = run_forward(lib, st, dev, case, n, inp, mode, wdev, False, inp["b"], inp["res"])
        narrow = run_forward(lib, st, dev, case, n, inp, mode, wdev, False, inp["b"], inp["res"], shift=1)
        assert wide.data_ptr() % 16 == 0 and narrow.data_ptr() % 16 == 4
        xin = C.loaded(inp, mode)
        ref, A = C.forward_eval(xin, inp["w"], inp["b"], inp["res"], "f64"), C.forward_eval(xin, inp["w"], inp["b"], inp["res"], "abs")
        judge(f"{C.case_id(case)} forward_narrow n={n}", narrow, ref, A, C.sum_length("forward", case, n),
              C.forward_eval(xin, inp["w"], inp["b"], inp["res"], "f32"))
        assert torch.equal(narrow, wide)
    if adm["backward_data"]:
        inp = C.backward_data_inputs(case, n, data)
        wdev = inp["w"].to(dev)
        wide = run_backward_data(lib, st, dev, case, n, inp, wdev, False, True)
        narrow = run_backward_data(lib, st, dev, case, n, inp, wdev, False, True, shift=1)
        assert wide.data_ptr() % 16 == 0 and narrow.data_ptr() % 16 == 4
        ref = C.backward_data_eval(inp["dy"], inp["w"], inp["relu_src"], inp["dres"], "f64")
        A = C.backward_data_eval(inp["dy"], inp["w"], inp["relu_src"], inp["dres"], "abs")
        judge(f"{C.case_id(case)} backward_data_narrow n={n}", narrow, ref, A, C.sum_length("backward_data", case, n),
              C.backward_data_eval(inp["dy"], inp["w"], inp["relu_src"], inp["dres"], "f32"))
        assert torch.equal(narrow, wide)
