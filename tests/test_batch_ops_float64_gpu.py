"""GPU: ppo_moments_f64, ppo_normalize_f32, ppo_accumulate_f32, ppo_axpy_f32, ppo_mask_mul_f32 and ppo_colsum_f32 called
directly (tests/policy_optim_float64.py: the references and how each bar is derived - from the arithmetic for the double
sums and the single float32 operations, measured on float32 torch for normalise and the column sums).  Outputs sit in
sentinel-filled buffers whose guards must survive; every launch runs twice and must give the same bits.

Prints POLOPT64_ERR <case> kernel max, float32 max, ratio, bar; profiles/policy_optim_float64.md records them."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import policy_optim_float64 as R  # noqa: E402
from ppo_amd import _lib  # noqa: E402

SENT64 = -7.25e300


def _p(t):
    return None if t is None else t.data_ptr()


def _env():
    return _lib.load(), torch.device("cuda"), _lib.current_stream()


def _bits(a, b):
    return R.same_bits(torch.as_tensor(a), torch.as_tensor(b))


def run_moments(lib, st, dev, xd):
    outs = []
    for fill in (0.0, float("nan")):  # whatever the workspace held must not matter
        mbuf, mom = R.guarded((3,), dev, dtype=torch.float64, sentinel=SENT64)
        wbuf, ws = R.guarded((lib.ppo_moments_workspace_bytes() // 8,), dev, dtype=torch.float64, sentinel=SENT64)
        ws.fill_(fill)
        _lib.check(lib.ppo_moments_f64(_p(xd), xd.numel(), _p(mom), _p(ws), st), "moments")
        torch.cuda.synchronize()
        assert R.guards_intact(mbuf, mom, SENT64) and R.guards_intact(wbuf, ws, SENT64)
        outs.append(mom.clone())
    assert R.same_bits(outs[0].cpu(), outs[1].cpu()), "two launches on the same inputs differ"
    return outs[0]


_MOMENT_DATA = {}


def _moment_data(n, data):
    """The array and its exact moments, computed once per case."""
    if (n, data) not in _MOMENT_DATA:
        rng = np.random.default_rng(n + (1 if data == "shifted" else 0))
        x = (rng.standard_normal(n) + (1e4 if data == "shifted" else 0.0)).astype(np.float32)
        _MOMENT_DATA[(n, data)] = (x, R.moments_ref(x))
    return _MOMENT_DATA[(n, data)]


@pytest.mark.parametrize("data", ["randn", "shifted"])
@pytest.mark.parametrize("n", [1, 255, 4096, 4097, 524289, 600001])
def test_moments_against_fsum(n, data):
    lib, dev, st = _env()
    x, (s, ss, cnt, sabs) = _moment_data(n, data)
    got = run_moments(lib, st, dev, torch.from_numpy(x).to(dev)).cpu().numpy()
    bar_s, bar_ss = n * 2.0 ** -52 * sabs, n * 2.0 ** -52 * ss  # the squares are their own absolute values
    print(f"POLOPT64_ERR moments n={n} {data} sum err={abs(got[0] - s):.3e} bar={bar_s:.3e} sumsq err={abs(got[1] - ss):.3e} "
          f"bar={bar_ss:.3e}")
    assert abs(got[0] - s) <= bar_s and abs(got[1] - ss) <= bar_ss
    assert got[2] == cnt


@pytest.mark.parametrize("n", [1, 256, 257])
def test_normalize_against_float64(n):
    lib, dev, st = _env()
    rng = np.random.default_rng(n)
    x = (rng.standard_normal(n) * 2.0 + 0.5).astype(np.float32)
    other = (rng.standard_normal(n) * 2.0 - 0.25).astype(np.float32)
    xd = torch.from_numpy(x).to(dev)
    eps = 1e-8
    # own: the moments of the array itself; pooled: of twice the data (this rank's and another's, the all-reduced case)
    for what, pool in (("own", x), ("pooled", np.concatenate([x, other]))):
        mom = run_moments(lib, st, dev, torch.from_numpy(pool).to(dev))
        outs = []
        for _ in range(2):
            obuf, out = R.guarded((n,), dev)
            sbuf, ms = R.guarded((2,), dev)
            _lib.check(lib.ppo_normalize_f32(_p(xd), n, _p(mom), eps, _p(out), _p(ms), st), "normalize")
            torch.cuda.synchronize()
            assert R.guards_intact(obuf, out) and R.guards_intact(sbuf, ms)
            outs.append((out.cpu(), ms.cpu()))
        assert R.same_bits(outs[0][0], outs[1][0]) and R.same_bits(outs[0][1], outs[1][1])
        s, ss, cnt, _ = R.moments_ref(pool)
        ref, mean, std, scale = R.normalize_ref(x, (s, ss, cnt), eps)
        if n == 1 and what == "own":  # variance 0: (x - mean) / eps with x - mean = 0
            assert float(outs[0][0][0]) == 0.0 and outs[0][1].tolist() == [float(x[0]), 0.0]
            continue
        e32 = R.rel_err(R.normalize_f32(x, pool, eps), ref, scale)
        e = R.rel_err(outs[0][0].double().numpy(), ref, scale)
        bar = R.report(f"normalize n={n} {what}", e, e32)
        assert e <= bar, f"{what}: {e:.3e} over the bar {bar:.3e}"
        # mean_std_out: the float64 mean and population std, each rounded once to float32 (a double sum's error is far below)
        assert abs(float(outs[0][1][0]) - mean) <= 2.0 ** -24 * abs(mean) + n * 2.0 ** -50 * (abs(mean) + 1)
        assert abs(float(outs[0][1][1]) - std) <= 2.0 ** -23 * std
    # nullable mean_std_out
    obuf, out = R.guarded((n,), dev)
    _lib.check(lib.ppo_normalize_f32(_p(xd), n, _p(mom), eps, _p(out), None, st), "normalize")
    assert R.guards_intact(obuf, out) and R.same_bits(out.cpu(), outs[0][0])


@pytest.mark.parametrize("n", [1, 256, 257])
def test_normalize_constant_array_gives_variance_zero_and_exact_zeros(n):
    """3.75 has a 4-bit mantissa: n c and n c^2 are exact doubles, so the variance is 0 exactly whatever the order."""
    lib, dev, st = _env()
    xd = torch.full((n,), 3.75, device=dev)
    mom = run_moments(lib, st, dev, xd)
    assert mom.cpu().tolist() == [3.75 * n, 3.75 * 3.75 * n, float(n)]
    obuf, out = R.guarded((n,), dev)
    sbuf, ms = R.guarded((2,), dev)
    _lib.check(lib.ppo_normalize_f32(_p(xd), n, _p(mom), 1e-8, _p(out), _p(ms), st), "normalize")
    torch.cuda.synchronize()
    assert R.guards_intact(obuf, out) and R.guards_intact(sbuf, ms)
    assert bool((out == 0).all()) and ms.cpu().tolist() == [3.75, 0.0]


@pytest.mark.parametrize("align", ["both", "dst_shifted", "src_shifted", "both_shifted"])
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 7, 1023, 1024, 1025, 1027])
def test_accumulate_is_one_float32_addition(n, align):
    """The 16-byte path (both aligned) ends in a scalar tail; any shifted pointer takes the scalar path."""
    lib, dev, st = _env()
    rng = np.random.default_rng(n)
    dst, src = rng.standard_normal(n).astype(np.float32), (rng.standard_normal(n) * 3).astype(np.float32)
    ds, ss = int(align in ("dst_shifted", "both_shifted")), int(align in ("src_shifted", "both_shifted"))
    outs = []
    for _ in range(2):
        dbuf, d = R.guarded((n,), dev, ds, init=torch.from_numpy(dst))
        sbuf, s = R.guarded((n,), dev, ss, init=torch.from_numpy(src))
        assert d.data_ptr() % 16 == 4 * ds and s.data_ptr() % 16 == 4 * ss
        _lib.check(lib.ppo_accumulate_f32(_p(d), _p(s), n, st), "accumulate")
        torch.cuda.synchronize()
        assert R.guards_intact(dbuf, d) and R.guards_intact(sbuf, s), "wrote outside dst"
        assert _bits(s.cpu(), torch.from_numpy(src)), "src changed"
        outs.append(d.cpu())
    assert R.same_bits(outs[0], outs[1])
    assert _bits(outs[0], torch.from_numpy(dst + src))


@pytest.mark.parametrize("n", [1, 255, 257])
def test_axpy_is_two_roundings(n):
    lib, dev, st = _env()
    dst, src, alpha = R.axpy_data(n)
    want = R.axpy_two_roundings(dst, src, alpha)
    if n > 200:  # the data tell a fused multiply-add apart (checked on the CPU as well)
        assert int((want.view(np.uint32) != R.axpy_fused(dst, src, alpha).view(np.uint32)).sum()) >= 10
    outs = []
    for _ in range(2):
        dbuf, d = R.guarded((n,), dev, init=torch.from_numpy(dst))
        s = torch.from_numpy(src).to(dev)
        _lib.check(lib.ppo_axpy_f32(_p(d), _p(s), float(alpha), n, st), "axpy")
        torch.cuda.synchronize()
        assert R.guards_intact(dbuf, d)
        outs.append(d.cpu())
    assert R.same_bits(outs[0], outs[1])
    assert _bits(outs[0], torch.from_numpy(want))


@pytest.mark.parametrize("n", [1, 255, 257])
def test_mask_mul_is_exact(n):
    lib, dev, st = _env()
    rng = np.random.default_rng(n)
    w = rng.standard_normal(n).astype(np.float32)
    mask = (rng.random(n) < 0.5).astype(np.uint8)
    mask[0] = n % 2
    for _ in range(2):
        wbuf, wd = R.guarded((n,), dev, init=torch.from_numpy(w))
        mbuf, md = R.guarded((n,), dev, dtype=torch.uint8, sentinel=255, init=torch.from_numpy(mask))
        _lib.check(lib.ppo_mask_mul_f32(_p(wd), _p(md), n, st), "mask_mul")
        torch.cuda.synchronize()
        assert R.guards_intact(wbuf, wd) and R.guards_intact(mbuf, md, 255)
        assert _bits(wd.cpu(), torch.from_numpy(w * mask.astype(np.float32)))


@pytest.mark.parametrize("cols", [1, 13, 256, 300])
@pytest.mark.parametrize("rows", [1, 255, 257, 1000])
def test_colsum_against_float64(rows, cols):
    lib, dev, st = _env()
    rng = np.random.default_rng(rows * 1000 + cols)
    for pad in (0, 5):
        ld = cols + pad
        full = np.full((rows, ld), 3.0e38, dtype=np.float32)  # the columns past `cols` must not be read into a sum
        full[:, :cols] = rng.standard_normal((rows, cols)).astype(np.float32)
        X = full[:, :cols]
        prev = rng.standard_normal(cols).astype(np.float32)
        xd = torch.from_numpy(full).to(dev)
        for accumulate in (0, 1):
            outs = []
            for _ in range(2):
                obuf, out = R.guarded((cols,), dev, init=torch.from_numpy(prev))
                _lib.check(lib.ppo_colsum_f32(_p(xd), rows, cols, ld, _p(out), accumulate, st), "colsum")
                torch.cuda.synchronize()
                assert R.guards_intact(obuf, out)
                outs.append(out.cpu())
            assert R.same_bits(outs[0], outs[1])
            ref, scale = R.colsum_ref(X, prev if accumulate else None)
            e32 = R.rel_err(R.colsum_f32(X.copy(), prev if accumulate else None), ref, scale)
            e = R.rel_err(outs[0].double().numpy(), ref, scale)
            bar = R.report(f"colsum rows={rows} cols={cols} ld={ld} accumulate={accumulate}", e, e32)
            assert e <= bar, f"{e:.3e} over the bar {bar:.3e}"
