"""GPU: ppo_sgd_step_f32 and ppo_sgd_step_presummed_f32 called directly, against float64 (tests/sgd_float64.py: sgd_ref;
tests/policy_optim_float64.py: the data regimes and how the bars are derived; tests/test_sgd_float64_cpu.py shows which
wrong variants the bars reject).  Consecutive steps; w is updated in place inside a sentinel-filled buffer, 16-byte
aligned and one float further (which forces the scalar path at n % 4 == 0); every sequence runs twice and must give the
same bits.

Prints POLOPT64_ERR sgd <case> kernel max, float32 max, ratio, bar; profiles/sgd_step.md records them."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import policy_optim_float64 as R  # noqa: E402
import sgd_float64 as S  # noqa: E402
from ppo_amd import _lib  # noqa: E402

LR = S.SGD_LR
HP = (R.ADAM_HP["lr"], R.ADAM_HP["beta1"], R.ADAM_HP["beta2"], R.ADAM_HP["eps"])


def _p(t):
    return None if t is None else t.data_ptr()


def _env():
    return _lib.load(), torch.device("cuda"), _lib.current_stream()


def _shifted(a, dev, shift):
    """The float32 array on the device, its first element `shift` floats past a 256-byte boundary."""
    buf = torch.empty(a.size + 8, dtype=torch.float32, device=dev)
    v = buf[shift:shift + a.size]
    v.copy_(torch.from_numpy(a))
    return v


def run_sgd(lib, st, dev, w, gs, max_norm, grad_div, shift, partials=None):
    """The steps in place in a guarded buffer -> per-step dicts of numpy arrays: w, norm and the workspace as the step left
    it.  partials: one float32 array per step -> the presummed entry point."""
    n = w.size
    wbuf, wv = R.guarded((n,), dev, shift, init=torch.from_numpy(w))
    nbuf, norm = R.guarded((1,), dev)
    wsbuf, ws = R.guarded((lib.ppo_adam_workspace_bytes() // 4,), dev)
    out = []
    for t, g in enumerate(gs):
        gd = _shifted(g, dev, shift)
        assert gd.data_ptr() % 16 == 4 * shift and wv.data_ptr() % 16 == 4 * shift
        args = (_p(wv), _p(gd), n, LR, float(max_norm), float(grad_div))
        if partials is None:
            rc = lib.ppo_sgd_step_f32(*args, _p(ws), _p(norm), st)
        else:
            pd = torch.from_numpy(partials[t]).to(dev)
            rc = lib.ppo_sgd_step_presummed_f32(*args, _p(pd), partials[t].size, _p(norm), st)
        _lib.check(rc, "sgd")
        torch.cuda.synchronize()
        assert R.guards_intact(wbuf, wv), "w: wrote outside its buffer"
        assert R.guards_intact(nbuf, norm) and R.guards_intact(wsbuf, ws)
        out.append({"w": wv.cpu().numpy().copy(), "norm": float(norm.item()), "ws": ws.cpu().numpy().copy()})
    return out


def twice(*a, **kw):
    r1, r2 = run_sgd(*a, **kw), run_sgd(*a, **kw)
    for a1, a2 in zip(r1, r2):
        assert np.array_equal(a1["w"].view(np.uint32), a2["w"].view(np.uint32)), "w: two runs on the same inputs differ"
        assert a1["norm"] == a2["norm"]
    return r1


def judge(tag, got, w, gs, max_norm, grad_div):
    ref = S.sgd_ref(w, gs, max_norm, grad_div)
    e = S.sgd_errs(got, ref)
    e32 = S.sgd_errs(S.sgd_f32(w, gs, max_norm, grad_div), ref)
    for k in ("w", "norm"):
        assert np.isfinite(e[k]), f"{tag}: {k} is not finite"
    return e, e32


@pytest.mark.parametrize("regime", R.ADAM_REGIMES)
def test_sgd_three_steps_against_float64(regime):
    """n = 260 on both paths, every max_norm kind, grad_div and both w modes (w = 0: the update itself is compared)."""
    lib, dev, st = _env()
    n = R.ADAM_N_SMALL
    for mn_kind in R.ADAM_MAX_NORM:
        for grad_div in R.ADAM_GRAD_DIV:
            for w_zero in (True, False):
                w, gs = S.sgd_inputs(n, regime, w_zero)
                mn = R.adam_max_norm(mn_kind, gs[0], grad_div)
                worst = {}
                for shift in (0, 1):
                    got = twice(lib, st, dev, w, gs, mn, grad_div, shift)
                    tag = f"sgd |g|={regime} max_norm={mn_kind} div={grad_div:g} w={'zero' if w_zero else 'randn'} shift={shift}"
                    e, e32 = judge(tag, got, w, gs, mn, grad_div)
                    for k in e:
                        worst[k] = max(worst.get(k, 0.0), e[k])
                        assert e[k] <= R.bar_from(e32[k]), f"{tag}: {k} {e[k]:.3e} over the bar {R.bar_from(e32[k]):.3e}"
                    if regime == "zero":  # norm 0, clip factor 1, nothing moves
                        for s in got:
                            assert s["norm"] == 0.0
                            assert np.array_equal(s["w"].view(np.uint32), w.view(np.uint32))
                tag = f"sgd |g|={regime} max_norm={mn_kind} div={grad_div:g} w={'zero' if w_zero else 'randn'}"
                for k in ("w", "norm"):
                    R.report(f"{tag} {k}", worst[k], e32[k])


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("n", R.ADAM_SIZES)
def test_sgd_sizes_and_alignments(n, shift):
    """The last two sizes wrap the scalar grid (1024 x 256 threads), the vector grid (n / 4 > 262144) and the 256-partial
    cap (n > 256 x 4096); n % 4 == 0 aligned takes the 16-byte path, everything else the scalar one."""
    lib, dev, st = _env()
    grad_div = 8.0
    for regime, mn_kind, w_zero in (("mix", "below", False), ("1e-3", "above", True)):
        w, gs = S.sgd_inputs(n, regime, w_zero, n_steps=2 if n > 100000 else 3)
        mn = R.adam_max_norm(mn_kind, gs[0], grad_div)
        got = twice(lib, st, dev, w, gs, mn, grad_div, shift)
        tag = f"sgd n={n} shift={shift} |g|={regime} max_norm={mn_kind}"
        e, e32 = judge(tag, got, w, gs, mn, grad_div)
        for k in e:
            bar = R.report(f"{tag} {k}", e[k], e32[k])
            assert e[k] <= bar, f"{tag}: {k} {e[k]:.3e} over the bar {bar:.3e}"


@pytest.mark.parametrize("n", [260, 4097, 1048580])
def test_sgd_reports_the_norm_bits_adam_reports(n):
    """The same sum-of-squares launch, partials and prologue: grad_norm_out of the two optimisers has the same bits."""
    lib, dev, st = _env()
    for mn_kind, grad_div in (("below", 8.0), ("off", 1.0)):
        w, m, v, gs = R.adam_inputs(n, "mix", False, n_steps=1)
        mn = R.adam_max_norm(mn_kind, gs[0], grad_div)
        g = torch.from_numpy(gs[0]).to(dev)
        ws = torch.zeros(lib.ppo_adam_workspace_bytes() // 4, device=dev)
        norms = torch.full((2,), -1.0, device=dev)
        wa, ma, va, wsg = (torch.from_numpy(a.copy()).to(dev) for a in (w, m, v, w))
        _lib.check(lib.ppo_adam_step_f32(_p(wa), _p(g), _p(ma), _p(va), n, 1, *HP, float(mn), grad_div, _p(ws), _p(norms[0:1]),
                                         st), "adam")
        _lib.check(lib.ppo_sgd_step_f32(_p(wsg), _p(g), n, LR, float(mn), grad_div, _p(ws), _p(norms[1:2]), st), "sgd")
        torch.cuda.synchronize()
        assert norms[0].item() > 0 and R.same_bits(norms[0:1], norms[1:2]), (n, mn_kind, norms.tolist())


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("n", [260, 4097, 1048580])
def test_sgd_presummed_on_the_workspace_partials_is_bit_identical(n, shift):
    lib, dev, st = _env()
    w, gs = S.sgd_inputs(n, "mix", False, n_steps=2)
    mn = R.adam_max_norm("below", gs[0], 8.0)
    plain = run_sgd(lib, st, dev, w, gs, mn, 8.0, shift)
    n_part = min((n + 4095) // 4096, 256)
    partials = [s["ws"][:n_part].copy() for s in plain]
    pre = run_sgd(lib, st, dev, w, gs, mn, 8.0, shift, partials=partials)
    for a, b in zip(plain, pre):
        assert np.array_equal(a["w"].view(np.uint32), b["w"].view(np.uint32))
        assert a["norm"] == b["norm"]
    assert not np.array_equal(plain[-1]["w"], w)


@pytest.mark.parametrize("n_partials", [1, 256])
def test_sgd_presummed_against_float64(n_partials):
    lib, dev, st = _env()
    n = R.ADAM_N_SMALL
    w, gs = S.sgd_inputs(n, "1e-3", True, n_steps=1)
    rng = np.random.default_rng(n_partials)
    total = float(np.sum(gs[0].astype(np.float64) ** 2))
    parts = rng.random(n_partials)
    parts = (parts / parts.sum() * total).astype(np.float32)
    sumsq = float(np.sum(parts.astype(np.float64)))
    mn = np.float32(np.sqrt(sumsq) * 0.7)
    for shift in (0, 1):
        got = twice(lib, st, dev, w, gs, mn, 1.0, shift, partials=[parts])
        e = S.sgd_errs(got, S.sgd_ref(w, gs, mn, 1.0, sumsq=sumsq))
        # float32's figure: the plain evaluation on the same gradient, clipped to the same norm (max_norm just below)
        mn32 = np.float32(np.sqrt(total) * 0.7)
        e32 = S.sgd_errs(S.sgd_f32(w, gs, mn32, 1.0), S.sgd_ref(w, gs, mn32, 1.0))
        for k in ("w", "norm"):
            bar = R.report(f"sgd presummed n_partials={n_partials} shift={shift} {k}", e[k], e32[k])
            assert e[k] <= bar, f"{k} {e[k]:.3e} over the bar {bar:.3e}"


def test_sgd_refuses_bad_arguments_before_anything_is_written():
    lib, dev, st = _env()
    w, g, parts = torch.ones(300, device=dev), torch.ones(300, device=dev), torch.ones(300, device=dev)
    ws = torch.zeros(lib.ppo_adam_workspace_bytes() // 4, device=dev)
    norm = torch.full((1,), -1.0, device=dev)
    for bad in (0, 257):
        assert lib.ppo_sgd_step_presummed_f32(_p(w), _p(g), 8, LR, 0.5, 1.0, _p(parts), bad, _p(norm), st) != 0
    assert lib.ppo_sgd_step_presummed_f32(_p(w), _p(g), 8, LR, 0.5, 0.0, _p(parts), 1, _p(norm), st) != 0
    assert lib.ppo_sgd_step_f32(_p(w), _p(g), 8, LR, 0.5, 0.0, _p(ws), _p(norm), st) != 0
    assert lib.ppo_sgd_step_f32(_p(w), _p(g), -1, LR, 0.5, 1.0, _p(ws), _p(norm), st) != 0
    assert lib.ppo_sgd_step_f32(None, _p(g), 8, LR, 0.5, 1.0, _p(ws), _p(norm), st) != 0
    assert lib.ppo_sgd_step_f32(_p(w), _p(g), 8, LR, 0.5, 1.0, None, _p(norm), st) != 0
    assert lib.ppo_sgd_step_f32(_p(w), _p(g), 0, LR, 0.5, 1.0, _p(ws), _p(norm), st) == 0  # nothing to do
    torch.cuda.synchronize()
    assert bool((w == 1).all()) and bool((ws == 0).all()) and norm.item() == -1.0
