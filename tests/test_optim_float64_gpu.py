"""GPU: ppo_adam_step_f32, ppo_adam_step_presummed_f32 and ppo_adam_step_scatter_f32 called directly, against float64
(tests/policy_optim_float64.py: adam_ref, the data regimes and how the bars are derived;
tests/test_policy_optim_float64_cpu.py shows which wrong variants the bars reject).  Three consecutive steps from given m
and v; w, m and v are updated in place inside sentinel-filled buffers, 16-byte aligned and one float further (which
forces the scalar path at n % 4 == 0); every sequence runs twice and must give the same bits.

Prints POLOPT64_ERR <case> kernel max, float32 max, ratio, bar; profiles/policy_optim_float64.md records them."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import policy_optim_float64 as R  # noqa: E402
from ppo_amd import _lib  # noqa: E402

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


def run_adam(lib, st, dev, w, m, v, gs, step0, max_norm, grad_div, shift, entry="plain", scatter=None, n_scatter=0, n_packed=0,
             partials=None):
    """The steps in place in guarded buffers -> (per-step dicts of numpy arrays: w, m, v, norm and the workspace as the step
    left it; packed or None).  entry:
    'plain', 'scatter' (table [n, 2] int32) or 'presummed' (partials: one float32 array per step)."""
    n = w.size
    state = {k: R.guarded((n,), dev, shift, init=torch.from_numpy(a)) for k, a in (("w", w), ("m", m), ("v", v))}
    nbuf, norm = R.guarded((1,), dev)
    wsbuf, ws = R.guarded((lib.ppo_adam_workspace_bytes() // 4,), dev)
    pbuf, packed = R.guarded((n_packed,), dev) if entry == "scatter" else (None, None)
    table = None if scatter is None else torch.from_numpy(scatter).to(dev)
    out = []
    for t, g in enumerate(gs):
        gd = _shifted(g, dev, shift)
        assert gd.data_ptr() % 16 == 4 * shift and state["w"][1].data_ptr() % 16 == 4 * shift
        args = (_p(state["w"][1]), _p(gd), _p(state["m"][1]), _p(state["v"][1]), n, step0 + t, *HP, float(max_norm), float(grad_div))
        if entry == "plain":
            rc = lib.ppo_adam_step_f32(*args, _p(ws), _p(norm), st)
        elif entry == "scatter":
            rc = lib.ppo_adam_step_scatter_f32(*args, _p(ws), _p(norm), _p(table), n_scatter, _p(packed), st)
        else:
            pd = torch.from_numpy(partials[t]).to(dev)
            rc = lib.ppo_adam_step_presummed_f32(*args, _p(pd), partials[t].size, _p(norm), st)
        _lib.check(rc, "adam")
        torch.cuda.synchronize()
        for k, (buf, view) in state.items():
            assert R.guards_intact(buf, view), f"{k}: wrote outside its buffer"
        assert R.guards_intact(nbuf, norm) and R.guards_intact(wsbuf, ws)
        assert pbuf is None or R.guards_intact(pbuf, packed)
        out.append({**{k: s[1].cpu().numpy().copy() for k, s in state.items()}, "norm": float(norm.item()),
                    "ws": ws.cpu().numpy().copy()})
    return out, None if packed is None else packed.cpu().numpy().copy()


def twice(*a, **kw):
    r1, p1 = run_adam(*a, **kw)
    r2, p2 = run_adam(*a, **kw)
    for a1, a2 in zip(r1, r2):
        for k in ("w", "m", "v"):
            assert np.array_equal(a1[k].view(np.uint32), a2[k].view(np.uint32)), f"{k}: two runs on the same inputs differ"
        assert a1["norm"] == a2["norm"]
    assert p1 is None or np.array_equal(p1.view(np.uint32), p2.view(np.uint32))
    return r1, p1


def judge(tag, got, w, m, v, gs, step0, max_norm, grad_div, sumsq=None):
    ref = R.adam_ref(w, m, v, gs, step0, max_norm, grad_div, sumsq=sumsq)
    e = R.adam_errs(got, ref)
    e32 = R.adam_errs(R.adam_f32(w, m, v, gs, step0, max_norm, grad_div), ref) if sumsq is None else None
    for k in ("w", "m", "v", "norm"):
        assert np.isfinite(e[k]), f"{tag}: {k} is not finite"
    return e, e32


@pytest.mark.parametrize("regime", R.ADAM_REGIMES)
@pytest.mark.parametrize("step", R.ADAM_STEPS)
def test_adam_three_steps_against_float64(step, regime):
    """n = 260 on both paths, every max_norm kind, grad_div and both w modes (w = 0: the update itself is compared)."""
    lib, dev, st = _env()
    n = R.ADAM_N_SMALL
    for mn_kind in R.ADAM_MAX_NORM:
        for grad_div in R.ADAM_GRAD_DIV:
            for w_zero in (True, False):
                w, m, v, gs = R.adam_inputs(n, regime, w_zero)
                mn = R.adam_max_norm(mn_kind, gs[0], grad_div)
                worst = {}
                for shift in (0, 1):
                    got, _ = twice(lib, st, dev, w, m, v, gs, step, mn, grad_div, shift)
                    tag = f"adam step={step} |g|={regime} max_norm={mn_kind} div={grad_div:g} w={'zero' if w_zero else 'randn'} shift={shift}"
                    e, e32 = judge(tag, got, w, m, v, gs, step, mn, grad_div)
                    for k in e:
                        worst[k] = max(worst.get(k, 0.0), e[k])
                        assert e[k] <= R.bar_from(e32[k]), f"{tag}: {k} {e[k]:.3e} over the bar {R.bar_from(e32[k]):.3e}"
                    if regime == "zero":  # norm 0, clip factor 1, w moves only by what m carries
                        assert got[0]["norm"] == 0.0
                        assert not w_zero or np.all(np.sign(got[0]["w"]) == -np.sign(m))
                tag = f"adam step={step} |g|={regime} max_norm={mn_kind} div={grad_div:g} w={'zero' if w_zero else 'randn'}"
                for k in ("w", "m", "v", "norm"):
                    R.report(f"{tag} {k}", worst[k], e32[k])


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("n", R.ADAM_SIZES)
def test_adam_sizes_and_alignments(n, shift):
    """The last two sizes wrap the scalar grid (1024 x 256 threads), the vector grid (n / 4 > 262144) and the 256-partial
    cap (n > 256 x 4096); n % 4 == 0 aligned takes the 16-byte path, everything else the scalar one."""
    lib, dev, st = _env()
    step, grad_div = 10, 8.0
    for regime, mn_kind, w_zero in (("mix", "below", False), ("1e-3", "above", True)):
        w, m, v, gs = R.adam_inputs(n, regime, w_zero, n_steps=2 if n > 100000 else 3)
        mn = R.adam_max_norm(mn_kind, gs[0], grad_div)
        got, _ = twice(lib, st, dev, w, m, v, gs, step, mn, grad_div, shift)
        tag = f"adam n={n} shift={shift} |g|={regime} max_norm={mn_kind}"
        e, e32 = judge(tag, got, w, m, v, gs, step, mn, grad_div)
        for k in e:
            bar = R.report(f"{tag} {k}", e[k], e32[k])
            assert e[k] <= bar, f"{tag}: {k} {e[k]:.3e} over the bar {bar:.3e}"


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("n", [260, 4097, 1048580])
def test_adam_presummed_on_the_workspace_partials_is_bit_identical(n, shift):
    lib, dev, st = _env()
    w, m, v, gs = R.adam_inputs(n, "mix", False, n_steps=2)
    mn = R.adam_max_norm("below", gs[0], 8.0)
    plain, _ = run_adam(lib, st, dev, w, m, v, gs, 10, mn, 8.0, shift)
    n_part = min((n + 4095) // 4096, 256)
    partials = [s["ws"][:n_part].copy() for s in plain]
    pre, _ = run_adam(lib, st, dev, w, m, v, gs, 10, mn, 8.0, shift, entry="presummed", partials=partials)
    for a, b in zip(plain, pre):
        for k in ("w", "m", "v"):
            assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k
        assert a["norm"] == b["norm"]


@pytest.mark.parametrize("n_partials", [1, 256])
def test_adam_presummed_against_float64(n_partials):
    lib, dev, st = _env()
    n = R.ADAM_N_SMALL
    w, m, v, gs = R.adam_inputs(n, "1e-3", True, n_steps=1)
    rng = np.random.default_rng(n_partials)
    total = float(np.sum(gs[0].astype(np.float64) ** 2))
    parts = rng.random(n_partials)
    parts = (parts / parts.sum() * total).astype(np.float32)
    sumsq = float(np.sum(parts.astype(np.float64)))
    mn = np.float32(np.sqrt(sumsq) * 0.7)
    for shift in (0, 1):
        got, _ = twice(lib, st, dev, w, m, v, gs, 2, mn, 1.0, shift, entry="presummed", partials=[parts])
        ref = R.adam_ref(w, m, v, gs, 2, mn, 1.0, sumsq=sumsq)
        e = R.adam_errs(got, ref)
        # float32's figure: the plain evaluation on the same gradient, clipped to the same norm (max_norm just below)
        e32 = R.adam_errs(R.adam_f32(w, m, v, gs, 2, np.float32(np.sqrt(total) * 0.7), 1.0),
                          R.adam_ref(w, m, v, gs, 2, np.float32(np.sqrt(total) * 0.7), 1.0))
        for k in ("w", "m", "v", "norm"):
            bar = R.report(f"adam presummed n_partials={n_partials} shift={shift} {k}", e[k], e32[k])
            assert e[k] <= bar, f"{k} {e[k]:.3e} over the bar {bar:.3e}"


def test_adam_presummed_refuses_partial_counts_outside_1_to_256():
    lib, dev, st = _env()
    w, m, v, g, parts = (torch.zeros(300, device=dev) for _ in range(5))
    for bad in (0, 257):
        assert lib.ppo_adam_step_presummed_f32(_p(w), _p(g), _p(m), _p(v), 8, 1, *HP, 0.5, 1.0, _p(parts), bad, None, st) != 0
    assert bool((w == 0).all())


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("n_scatter", [0, 1, 6, 40])
def test_adam_scatter_table_with_a_ragged_end(n_scatter, shift):
    """A table with -1 entries and rows with two targets: packed holds the new w at every target and the sentinel
    elsewhere; w, m, v bit-equal to the call without a table.  n = 40: the 16-byte path when aligned (n_scatter = 6 ends
    inside a float4), the scalar path one float further."""
    lib, dev, st = _env()
    n, n_packed = 40, 97
    w, m, v, gs = R.adam_inputs(n, "1e-3", False, n_steps=1)
    rng = np.random.default_rng(11)
    table = np.full((n, 2), -1, dtype=np.int32)
    targets = rng.permutation(n_packed)
    for i in range(n):
        kind = i % 4  # both targets, first only, second only, none
        if kind in (0, 1):
            table[i, 0] = targets[2 * i]
        if kind in (0, 2):
            table[i, 1] = targets[2 * i + 1]
    plain, _ = run_adam(lib, st, dev, w, m, v, gs, 3, 0.5, 1.0, shift)
    got, packed = twice(lib, st, dev, w, m, v, gs, 3, 0.5, 1.0, shift, entry="scatter", scatter=table, n_scatter=n_scatter,
                        n_packed=n_packed)
    for k in ("w", "m", "v"):
        assert np.array_equal(got[0][k].view(np.uint32), plain[0][k].view(np.uint32)), k
    want = np.full(n_packed, np.float32(R.SENTINEL))
    for i in range(n_scatter):
        for d in table[i]:
            if d >= 0:
                want[d] = got[0]["w"][i]
    assert np.array_equal(packed.view(np.uint32), want.view(np.uint32))
    assert n_scatter == 0 or int((want != np.float32(R.SENTINEL)).sum()) > 0


def test_adam_scatter_refuses_a_table_longer_than_the_buffer():
    lib, dev, st = _env()
    w, m, v, g, packed = (torch.zeros(64, device=dev) for _ in range(5))
    table = torch.full((64, 2), -1, dtype=torch.int32, device=dev)
    ws = torch.empty(lib.ppo_adam_workspace_bytes() // 4, device=dev)
    assert lib.ppo_adam_step_scatter_f32(_p(w), _p(g), _p(m), _p(v), 40, 1, *HP, 0.5, 1.0, _p(ws), None, _p(table), 41,
                                         _p(packed), st) != 0
