"""GPU: the gradient-noise kernels (csrc/grad_noise.hip) against torch / NumPy.

acc must equal a torch float32 `acc += g` loop bit for bit.  Every sum of squares is compared with
np.sum(g.astype(np.float64) ** 2): float32 squares are exact in float64, so summation is the only rounding and any
summation order of n non-negative terms is within n * 2^-53 relative of the exact sum.  Sizes: 1 and 3 (scalar head / tail
only), 255 / 256 / 257 (around one workgroup's vectors), 65 541 (several workgroups, odd), 1 090 003 (the IMPALA net's order:
every workgroup, more than one unrolled trip)."""
import math

import numpy as np
import pytest
import torch

from ppo_amd import _lib

pytestmark = pytest.mark.gpu

SIZES = [1, 3, 255, 256, 257, 65541, 1090003]
U = 2.0 ** -53


@pytest.fixture(scope="module")
def lib():
    _lib.require_gpu()
    return _lib.load()


def run(lib, grads, acc, ws, out, max_passes=None):
    """grads: list of [n] device views; returns (acc, out) after the passes and the finish."""
    m, n = len(grads), grads[0].numel()
    max_passes = max_passes or m
    st = _lib.current_stream()
    for i, g in enumerate(grads):
        _lib.check(lib.ppo_grad_noise_pass_f32(g.data_ptr(), acc.data_ptr(), n, i, max_passes, ws.data_ptr(), st), "pass")
    _lib.check(lib.ppo_grad_noise_finish_f64(acc.data_ptr(), n, m, max_passes, ws.data_ptr(), out.data_ptr(), st), "finish")
    return acc, out[:m + 1].cpu().numpy()


def make(lib, n, passes, g_off, a_off, scale, seed):
    """passes gradients of n floats at base offset g_off floats, an acc at a_off floats; the last pass (of > 1) is zero."""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    store = torch.randn((passes, n + 4), generator=gen, device="cuda", dtype=torch.float32) * scale
    if passes > 1:
        store[-1].zero_()
    grads = [store[i, g_off:g_off + n] for i in range(passes)]
    acc_store = torch.full((n + 8,), float("nan"), device="cuda")
    ws = torch.full((lib.ppo_grad_noise_workspace_bytes(passes) // 8,), float("nan"), dtype=torch.float64, device="cuda")
    out = torch.full((passes + 1,), float("nan"), dtype=torch.float64, device="cuda")
    return grads, acc_store, acc_store[a_off:a_off + n], ws, out


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("passes,g_off,a_off,scale", [(1, 0, 0, 1.0), (2, 1, 0, 1e-4), (2, 0, 1, 1e3), (16, 1, 1, 1.0),
                                                      (2, 3, 2, 1.0)])
def test_accumulate_and_sums(lib, n, passes, g_off, a_off, scale):
    grads, acc_store, acc, ws, out = make(lib, n, passes, g_off, a_off, scale, seed=1000 * passes + n % 997)
    assert grads[0].data_ptr() % 16 == 4 * g_off % 16 and acc.data_ptr() % 16 == 4 * a_off % 16
    acc, sums = run(lib, grads, acc, ws, out)
    want = grads[0].clone()
    for g in grads[1:]:
        want += g
    assert torch.equal(acc, want)  # bit-identical float32 accumulation
    # nothing outside [a_off, a_off + n) was written
    assert torch.isnan(acc_store[:a_off]).all() and torch.isnan(acc_store[a_off + n:]).all()
    squares = [g.cpu().numpy().astype(np.float64) ** 2 for g in grads] + [want.cpu().numpy().astype(np.float64) ** 2]
    for i, (got, sq) in enumerate(zip(sums, squares)):
        # np.sum (pairwise, itself rounded) is the stated reference; math.fsum of the same exact squares is the correctly
        # rounded sum, against which the derived bound holds strictly: n - 1 additions of at most 2^-53 each, and the
        # reference's own half-ulp, stay below n * 2^-53
        for name, ref in (("np.sum", float(np.sum(sq))), ("fsum", math.fsum(sq))):
            err = abs(got - ref) / ref if ref > 0 else abs(got)
            print(f"n={n} passes={passes} out[{i}] vs {name} rel err {err:.3e} (bound {n * U:.3e})")
            assert err <= n * U, (i, name, got, ref)
    if passes > 1:
        assert sums[passes - 1] == 0.0  # the all-zero pass


@pytest.mark.parametrize("n", [257, 1090003])
def test_two_runs_are_bit_identical(lib, n):
    results = []
    for _ in range(2):
        grads, _store, acc, ws, out = make(lib, n, 3, 1, 0, 1.0, seed=7)
        acc, sums = run(lib, grads, acc, ws, out)
        results.append((acc.clone(), sums.copy()))
    assert torch.equal(results[0][0], results[1][0])
    assert results[0][1].tobytes() == results[1][1].tobytes()


def test_fewer_passes_than_the_workspace_holds(lib):
    grads, _store, acc, _ws, _out = make(lib, 1000, 3, 0, 0, 1.0, seed=3)
    ws = torch.zeros(lib.ppo_grad_noise_workspace_bytes(8) // 8, dtype=torch.float64, device="cuda")
    out = torch.zeros(9, dtype=torch.float64, device="cuda")
    _acc, sums = run(lib, grads, acc, ws, out, max_passes=8)
    refs = [np.sum(g.cpu().numpy().astype(np.float64) ** 2) for g in grads]
    assert all(abs(s - r) <= 1000 * U * r for s, r in zip(sums[:3], refs))
    assert (out[4:] == 0).all()  # untouched


def test_bad_arguments_are_refused(lib):
    g = torch.zeros(16, device="cuda")
    acc = torch.zeros(16, device="cuda")
    ws = torch.zeros(lib.ppo_grad_noise_workspace_bytes(2) // 8, dtype=torch.float64, device="cuda")
    out = torch.zeros(3, dtype=torch.float64, device="cuda")
    st = _lib.current_stream()
    ok = (g.data_ptr(), acc.data_ptr(), 16, 0, 2, ws.data_ptr(), st)
    for pos, bad in ((0, None), (1, None), (5, None), (2, 0), (2, -3), (3, -1), (3, 2), (4, 0)):
        a = list(ok)
        a[pos] = bad
        assert lib.ppo_grad_noise_pass_f32(*a) == -1
    assert lib.ppo_grad_noise_pass_f32(g.data_ptr() + 1, acc.data_ptr(), 8, 0, 2, ws.data_ptr(), st) == -3
    okf = (acc.data_ptr(), 16, 2, 2, ws.data_ptr(), out.data_ptr(), st)
    for pos, bad in ((0, None), (4, None), (5, None), (1, 0), (2, 0), (2, 3)):
        a = list(okf)
        a[pos] = bad
        assert lib.ppo_grad_noise_finish_f64(*a) == -1
    torch.cuda.synchronize()
    assert (acc == 0).all() and (out == 0).all()  # nothing was written on error
