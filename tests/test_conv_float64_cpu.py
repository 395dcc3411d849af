"""CPU: the conditions of tests/test_conv_float64_gpu.py, checked without a GPU on the float64 reference and the two
comparison evaluations of tests/conv_float64_torch.py - what has to hold for the GPU comparison to mean something: the
per-element bar is one plain float32 arithmetic meets at every element, a reduced-precision evaluation is an order of
magnitude worse in aggregate (so the aggregate bar can tell the two apart), the `integers` sets are exact in float32,
the wrapping batch sizes do wrap, and the table of admitted modes is what the library's probes say.

Prints CONV64_CPU lines: <case> <op> <what> <data> n, max(e/A) and rms(e/A) of float32 and of the split, their ratio."""
import pytest

torch = pytest.importorskip("torch")

import conv_float64_torch as C  # noqa: E402

NONE, RELU, U8 = C.NONE, C.RELU, C.U8
MODE_NAME = {NONE: "none", RELU: "relu", U8: "u8"}
FWD_CASES = [c for c in C.CASES if C.table(c)["forward"]]
BWD_CASES = [c for c in C.CASES if C.table(c)["backward_data"]]
WG_CASES = [c for c in C.CASES if C.table(c)["backward_weight"]]


def _ids(cases):
    return [C.case_id(c) for c in cases]


def _report(case, op, what, data, n, f32, split):
    ratio = split[1] / max(f32[1], 1e-300)
    print(f"CONV64_CPU {C.case_id(case)} {op} {what} {data} n={n} f32 max={f32[0]:.3e} rms={f32[1]:.3e} "
          f"split max={split[0]:.3e} rms={split[1]:.3e} ratio={ratio:.1f}")
    return ratio


def test_the_table_of_admitted_modes_is_what_the_probes_say():
    for case in C.CASES:
        t = C.table(case)
        assert t["forward"] or t["backward_data"], case  # every case of dispatch_conv is reached by something
    try:
        from ppo_amd import _lib
        lib = _lib.load()
    except Exception as e:  # not built on this host: the table is what the helper uses
        print(f"library not loaded ({type(e).__name__}): table only")
        return
    for case in C.CASES:
        assert C.probed(lib, case) == C.table(case), case
        assert C.admitted(case) == C.table(case)


def test_wrapping_batch_sizes_wrap():
    """Each entry satisfies its inequality and is the smallest that does; the conv values are the ones worked out by hand
    from today's TR / NW."""
    by_hand = {84: 110, 64: 193, 42: 110, 32: 193, 21: 385, 16: 769, 11: 1537, 8: 1537}
    for side, t in C.TILING.items():
        nb, n = C.nbands("conv", side), C.wrapping_n("conv", side)
        cap = 256 * (24 // t["conv"][1])
        assert n == by_hand[side]
        assert n * nb > cap and (n * nb) % 256 != 0
        assert all((m * nb <= cap) or (m * nb) % 256 == 0 for m in range(1, n))
        if t["pool"] is not None:
            nb, n = C.nbands("pool", side), C.wrapping_n("pool", side)
            assert n * nb > 256 * 3 and (n * nb) % 256 != 0
            assert all((m * nb <= 768) or (m * nb) % 256 == 0 for m in range(1, n))
        nb, n = C.nbands("wgrad", side), C.wrapping_n("wgrad", side)
        assert n * nb > 512 >= (n - 1) * nb
    # every tensor of the wrapping cases stays under 60 MB
    for case in C.CASES:
        ck, cm, h, w = case
        assert C.wrapping_n("conv", h) * max(ck, cm) * h * w * 4 < 60e6


def test_integer_sets_are_exact_in_float32():
    """Operands in [-2, 2]: every product and every partial sum, in any order, is an integer below 2^24."""
    for case in C.CASES:
        for n in (3, C.wrapping_n("conv", case[2])):
            assert C.integer_bound("forward", case, n) < 2 ** 24
            assert C.integer_bound("backward_data", case, n) < 2 ** 24
        for n in (3, C.wrapping_n("wgrad", case[2])):
            assert C.integer_bound("backward_weight", case, n) < 2 ** 24
    inp = C.forward_inputs((16, 16, 32, 32), 3, "integers")
    for t in (inp["x"], inp["w"], inp["res"]):
        assert float(t.abs().max()) == 2.0 and bool((t == t.round()).all())
    assert float(inp["b"].abs().max()) <= 5.0
    ref = C.forward_eval(C.loaded(inp, RELU), inp["w"], inp["b"], inp["res"], "f64")
    assert torch.equal(C.forward_eval(C.loaded(inp, RELU), inp["w"], inp["b"], inp["res"], "f32"), ref)


def test_ranged_sets_hold_what_they_claim():
    inp = C.forward_inputs((16, 16, 32, 32), 3, "ranged")
    x = inp["x"]
    zeros = float((x == 0).float().mean())
    assert 0.25 < zeros < 0.35
    assert bool(((x == 0) & torch.signbit(x)).any()) and bool(((x == 0) & ~torch.signbit(x)).any()) and bool((x < 0).any())
    per_channel = x.abs().amax((0, 2, 3))
    assert float(per_channel.max() / per_channel.min()) >= 2.0 ** 8  # channels of different scale
    src = C.backward_data_inputs((16, 16, 32, 32), 3, "ranged")["relu_src"]
    assert bool(((src == 0) & torch.signbit(src)).any()) and bool((src < 0).any()) and bool((src > 0).any())
    xu = C.forward_inputs((4, 16, 84, 84), 3, "ranged")["xu"]
    assert 0.25 < float((xu == 0).float().mean()) < 0.35


def _forward_variants(case):
    """(what, mode, bias?, residual?) of a forward case."""
    modes = C.table(case)["forward"]
    v = [("bias", NONE, True, False), ("nobias", NONE, False, False)]
    if RELU in modes:
        v.append(("relu_residual", RELU, True, True))
    if U8 in modes:
        v.append(("u8", U8, True, False))
    return v


@pytest.mark.parametrize("data", C.DATA_SETS)
@pytest.mark.parametrize("case", FWD_CASES, ids=_ids(FWD_CASES))
def test_forward_float32_meets_the_bar_and_the_split_is_10x_worse(case, data):
    n = 3
    inp = C.forward_inputs(case, n, data)
    K = C.sum_length("forward", case, n)
    for what, mode, bias, residual in _forward_variants(case):
        xin = C.loaded(inp, mode)
        b, res = (inp["b"] if bias else None), (inp["res"] if residual else None)
        ref, A = C.forward_eval(xin, inp["w"], b, res, "f64"), C.forward_eval(xin, inp["w"], b, res, "abs")
        f32 = C.err_stats(C.forward_eval(xin, inp["w"], b, res, "f32"), ref, A, K)
        split = C.err_stats(C.forward_eval(xin, inp["w"], b, res, "split"), ref, A, K)
        ratio = _report(case, "forward", what, data, n, f32, split)
        assert f32[2] == 0, f"{what}: {f32[2]} elements of plain float32 over the bar"
        assert ratio >= 10.0, what


@pytest.mark.parametrize("data", C.DATA_SETS)
@pytest.mark.parametrize("case", BWD_CASES, ids=_ids(BWD_CASES))
def test_backward_data_float32_meets_the_bar_and_the_split_is_10x_worse(case, data):
    n = 3
    inp = C.backward_data_inputs(case, n, data)
    K = C.sum_length("backward_data", case, n)
    for what, src, dres in (("plain", None, None), ("gated_dres", inp["relu_src"], inp["dres"])):
        ref = C.backward_data_eval(inp["dy"], inp["w"], src, dres, "f64")
        A = C.backward_data_eval(inp["dy"], inp["w"], src, dres, "abs")
        f32 = C.err_stats(C.backward_data_eval(inp["dy"], inp["w"], src, dres, "f32"), ref, A, K)
        split = C.err_stats(C.backward_data_eval(inp["dy"], inp["w"], src, dres, "split"), ref, A, K)
        ratio = _report(case, "backward_data", what, data, n, f32, split)
        assert f32[2] == 0, f"{what}: {f32[2]} elements of plain float32 over the bar"
        assert ratio >= 10.0, what


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("case", WG_CASES, ids=_ids(WG_CASES))
def test_backward_weight_float32_meets_the_bar_and_where_the_split_is_10x_worse(case, n):
    """The separation exists only for short sums: the ratios are printed for every case, and asserted (>= 10 on both data
    sets) exactly for the entries of WGRAD_AGGREGATE, which is what the GPU test reads."""
    K = C.sum_length("backward_weight", case, n)
    worst = float("inf")
    for data in C.DATA_SETS:
        inp = C.backward_weight_inputs(case, n, data)
        for mode in C.table(case)["backward_weight"]:
            xin = C.loaded(inp, mode)
            (dw, db), (Aw, Ab) = C.backward_weight_eval(xin, inp["dy"], "f64"), C.backward_weight_eval(xin, inp["dy"], "abs")
            g32, gsp = C.backward_weight_eval(xin, inp["dy"], "f32"), C.backward_weight_eval(xin, inp["dy"], "split")
            f32, split = C.err_stats(g32[0], dw, Aw, K), C.err_stats(gsp[0], dw, Aw, K)
            worst = min(worst, _report(case, "backward_weight", MODE_NAME[mode], data, n, f32, split))
            fb = C.err_stats(g32[1], db, Ab, K)
            assert f32[2] == 0 and fb[2] == 0, f"mode {mode}: plain float32 over the bar"
    print(f"CONV64_CPU {C.case_id(case)} backward_weight n={n} smallest ratio {worst:.1f}")
    if (C.case_id(case), n) in C.WGRAD_AGGREGATE:
        assert worst >= 10.0, worst


def test_long_weight_gradient_sums_have_no_separation():
    """At the sum lengths of the wrapping batches accumulation rounding swamps the split's truncation: no entry of
    WGRAD_AGGREGATE is at a wrapping n, and one long case shows why."""
    assert all(n in (1, 3) for _, n in C.WGRAD_AGGREGATE)
    case, n = (32, 32, 8, 8), C.wrapping_n("wgrad", 8)
    inp = C.backward_weight_inputs(case, n, "plain")
    xin = C.loaded(inp, RELU)
    dw, Aw = C.contract("backward_weight", xin, inp["dy"], "f64"), C.contract("backward_weight", xin, inp["dy"], "abs")
    K = C.sum_length("backward_weight", case, n)
    f32 = C.err_stats(C.contract("backward_weight", xin, inp["dy"], "f32"), dw, Aw, K)
    split = C.err_stats(C.contract("backward_weight", xin, inp["dy"], "split"), dw, Aw, K)
    assert f32[2] == 0
    assert _report(case, "backward_weight", "relu", "plain", n, f32, split) < 10.0
