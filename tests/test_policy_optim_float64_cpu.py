"""CPU: what has to hold for tests/test_policy_float64_gpu.py, test_optim_float64_gpu.py and
test_batch_ops_float64_gpu.py to mean something, checked without a GPU on the references, data sets and float32
evaluations of tests/policy_optim_float64.py: every measured bar accepts plain float32 torch on the data of the GPU tests
and rejects a wrong variant of the same operation (written here in float32 torch / numpy, never in a kernel); the uniform
the sampler is to produce lies strictly inside (0, 1) for all 2^24 values of k while the formula without the clamp
reaches 1.0; the counters the GPU test uses for that draw have that k; the action comparison leaves out at most 2 % of the
rows for the seeds in use.

Prints POLOPT64_CPU lines: case, float32's error, the variant's error, the bar."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import policy_optim_float64 as R  # noqa: E402


def _line(tag, f32, variant, bar):
    print(f"POLOPT64_CPU {tag} f32={f32:.3e} variant={variant:.3e} bar={bar:.3e}")


# --------------------------------------------------------------------------------------------- the generator
def test_uniform_is_strictly_inside_the_unit_interval_for_every_k():
    k = np.arange(2 ** 24, dtype=np.uint32)
    u = R.u_from_k(k)
    assert u.dtype == np.float32
    assert float(u.min()) > 0.0 and float(u.max()) < 1.0
    assert u[0] == np.float32(2.0 ** -25) and u[-1] == R.U_MAX
    # -log(-log u) is finite at both ends in float32
    with np.errstate(all="raise"):
        g = -np.log(-np.log(u[[0, -1]]))
    assert np.isfinite(g).all()
    # the formula without the clamp: k + 0.5 rounds to even above 2^23 and reaches 2^24 at the last k
    old = R.u_unclamped(k)
    assert old[-1] == np.float32(1.0) and int((old >= 1.0).sum()) == 1
    # every other draw keeps its bits
    assert np.array_equal(old[:-1].view(np.uint32), u[:-1].view(np.uint32))
    assert np.all(np.diff(u.astype(np.float64)) >= 0)


def test_the_bad_counters_draw_the_last_k():
    k, u = R.uniform01_ref(R.BAD_SEED, np.array(R.BAD_COUNTERS, dtype=np.uint64))
    assert (k == 2 ** 24 - 1).all() and (u == R.U_MAX).all()
    assert (R.u_unclamped(k) == np.float32(1.0)).all()
    # found by search, not only written down: the first of them is the first such counter of the seed
    kk = R.uniform01_ref(R.BAD_SEED, np.arange(R.BAD_COUNTERS[0] + 1, dtype=np.uint64))[0]
    assert int(np.flatnonzero(kk == 2 ** 24 - 1)[0]) == R.BAD_COUNTERS[0]


def test_uniform01_ref_known_values_and_wraparound():
    """splitmix64's first outputs from state 0 are public: uniform01_ref(seed, c) mixes seed + golden * (c + 1), so
    (seed 0, counter 0) is the generator's first output, 0xE220A8397B1DCDAF; its top 24 bits are k."""
    k, u = R.uniform01_ref(0, 0)
    assert int(k[0]) == 0xE220A8397B1DCDAF >> 40
    assert u[0] == np.float32((int(k[0]) + 0.5) * 2.0 ** -24)
    # a seed above 2^32 and counters near 2^64 wrap without error
    k2, _ = R.uniform01_ref(0xFEDCBA9876543210, np.array([2 ** 64 - 1, 0], dtype=np.uint64))
    assert int(k2[0]) == int(R.uniform01_ref(0xFEDCBA9876543210 - 0x9E3779B97F4A7C15, 0)[0][0])


# --------------------------------------------------------------------------------------------- discrete action step
@pytest.mark.parametrize("data", R.ACT_DATA)
def test_log_policy_bar_accepts_float32_and_rejects_wrong_softmax(data):
    for nA in R.ACT_NA:
        z = R.act_logits(nA, data)
        for T in R.ACT_T:
            ref = R.policy_act_ref(z, T)
            f32 = R.lp_err(R.policy_act_f32(z, T)["lp"], ref)
            bar = R.bar_from(f32)
            assert f32 <= bar
            if T != 1.0 and nA > 1:
                bad = R.lp_err(R.policy_act_f32(z, T, variant="temp_multiplied")["lp"], ref)
                _line(f"act nA={nA} {data} T={T} temp_multiplied", f32, bad, bar)
                assert bad > bar
            # exp overflows without the max subtraction: e^1e4 always, e^80 = 5.5e34 not yet, e^160 (T = 0.5) does
            if (data == "shift1e4" or (data == "pm80" and T == 0.5)) and nA > 1:
                bad = R.lp_err(R.policy_act_f32(z, T, variant="no_max")["lp"], ref)
                _line(f"act nA={nA} {data} T={T} no_max", f32, bad, bar)
                assert bad > bar


@pytest.mark.parametrize("data", R.ACT_DATA)
def test_action_margin_leaves_out_at_most_two_percent_for_the_seeds_in_use(data):
    for nA in R.ACT_NA:
        z, u = R.act_logits(nA, data), R.act_uniforms(nA, data)
        for T in R.ACT_T:
            ref = R.policy_act_ref(z, T, u)
            f32 = R.policy_act_f32(z, T, u)
            clear = R.clear_rows(ref, R.bar_from(R.lp_err(f32["lp"], ref)))
            for B in R.ACT_B:
                out = int((~clear[:B]).sum())
                assert out <= int(R.EXCLUDED_CAP * B), (nA, data, T, B, out)
            assert torch.equal(f32["action"][clear], ref["action"][clear]), (nA, data, T)


def test_internal_generator_cases_meet_the_cap():
    """The (seed, offset) pairs of the internal-generator GPU tests."""
    for nA, seed, offset in R.GEN_CASES:
        z = R.act_logits(nA, "plain")
        B = z.shape[0]
        u = R.uniform01_ref(seed, np.uint64(offset) + np.arange(B * nA, dtype=np.uint64))[1].reshape(B, nA)
        ref = R.policy_act_ref(z, 1.0, u)
        f32 = R.policy_act_f32(z, 1.0, torch.from_numpy(u))
        clear = R.clear_rows(ref, R.bar_from(R.lp_err(f32["lp"], ref)))
        assert int((~clear).sum()) <= int(R.EXCLUDED_CAP * B)
        assert torch.equal(f32["action"][clear], ref["action"][clear])
        assert len(set(ref["action"].tolist())) > 1


def test_u_equal_one_takes_the_improbable_action_and_the_clamped_u_does_not():
    """The GPU test's case on the CPU: the bad counter on action a*, logit -40 there, zeros elsewhere."""
    for counter in R.BAD_COUNTERS[:2]:
        for a_star in (0, 5):
            z, u, offset = R.bad_draw_case(counter, a_star)
            assert R.uniform01_ref(R.BAD_SEED, offset + a_star)[0][0] == 2 ** 24 - 1
            ref = R.policy_act_ref(z, 1.0, u)
            assert int(ref["action"][0]) != a_star and ref["gap"][0] > 1e-3
            u_old = u.copy()
            u_old[0, a_star] = 1.0
            with np.errstate(divide="ignore"):
                s_old = R.policy_act_f32(z, 1.0, torch.from_numpy(u_old))
            assert int(s_old["action"][0]) == a_star and float(s_old["scores"][0, a_star]) == float("inf")


# --------------------------------------------------------------------------------------------- discrete PPO loss
@pytest.mark.parametrize("nA", R.LOSS_NA)
def test_loss_bars_accept_float32_and_reject_clamps_gradient(nA):
    for vh in R.LOSS_VH:
        inp = R.loss_inputs(nA, vh)
        for with_old in (False, True):
            B = max(R.LOSS_B)
            ref = R.ppo_loss_ref(inp, B, with_old, **R.LOSS_COEF)
            f32 = R.ppo_loss_f32(inp, B, with_old, **R.LOSS_COEF)
            d32, s32 = R.loss_errs(f32["dheads"], f32["stats"], ref)
            bar = R.bar_from(d32)
            assert d32 <= bar and all(v <= R.bar_from(v) for v in s32.values())
            bad = R.ppo_loss_f32(inp, B, with_old, variant="clamp_grad", **R.LOSS_COEF)
            dbad, _ = R.loss_errs(bad["dheads"], bad["stats"], ref)
            _line(f"loss nA={nA} vh={vh} old={int(with_old)} clamp_grad", d32, dbad, bar)
            assert dbad > bar
            # what the per-row scale adds: an entropy gradient 1 % off on one quiet row stays under 1e-5 of the tensor's
            # max-norm (the bar of test_ppo_loss_matches_reference_formula_autograd) and is over this one
            quiet = f32["dheads"].clone()
            quiet[5, :nA] *= 1.01  # the advantage-0 row: its policy gradient is the entropy term alone, 1 % off
            dq, _ = R.loss_errs(quiet, f32["stats"], ref)
            whole = float((quiet.double() - ref["dheads"]).abs().max() / ref["dheads"].abs().max())
            _line(f"loss nA={nA} vh={vh} old={int(with_old)} quiet_row_1pct (whole-tensor max-norm {whole:.1e})", d32, dq, bar)
            assert dq > bar and whole < 1e-5
            # the clipped column: no planted row is left out, at most 2 % of the random ones
            decided = R.clip_decided(ref, R.bar_from(s32["ratio"]))
            assert bool(decided[:R.N_PLANTED].all())
            for Bs in R.LOSS_B:
                assert int((~decided[:Bs]).sum()) <= int(R.EXCLUDED_CAP * max(Bs - R.N_PLANTED, 0))
            assert torch.equal(f32["stats"][:, 3][decided].double(), ref["stats"][:, 3][decided])
            # both branches of the planted rows are what their names say
            r = ref["ratio"]
            assert r[0] > 1.2 and r[1] > 1.2 and r[2] < 0.8 and r[3] < 0.8 and abs(float(r[4]) - 1.0) < 1e-6
            assert ref["stats"][:4, 3].tolist() == [1.0] * 4 and ref["stats"][4, 3] == 0.0
            assert float(ref["dheads"][0, :nA].abs().max()) < 0.02 * float(ref["dheads"][1, :nA].abs().max())


# --------------------------------------------------------------------------------------------- Adam
def _adam_case(step, regime, mn_kind, grad_div, w_zero, variant):
    w, m, v, gs = R.adam_inputs(R.ADAM_N_SMALL, regime, w_zero)
    mn = R.adam_max_norm(mn_kind, gs[0], grad_div)
    ref = R.adam_ref(w, m, v, gs, step, mn, grad_div)
    f32 = R.adam_errs(R.adam_f32(w, m, v, gs, step, mn, grad_div), ref)
    bad = R.adam_errs(R.adam_f32(w, m, v, gs, step, mn, grad_div, variant=variant), ref)
    return f32, bad


# (variant, the case of the GPU test where it shows: step, regime, max_norm, grad_div, w = 0)
ADAM_VARIANTS = [
    ("eps_in_root", 1, "1e-8", "off", 1.0, True), ("eps_in_root", 10, "1e-3", "off", 8.0, True),
    ("eps_before_bc", 1, "1e-8", "off", 1.0, True), ("eps_before_bc", 2, "1e-3", "above", 1.0, True),
    ("eps_before_bc", 10, "1e-3", "off", 1.0, True),
    ("bc_float", 1000, "1", "off", 1.0, True), ("bc_float", 1000, "1e-3", "below", 8.0, True),
    ("clip_no_1e-6", 10, "1e-8", "below", 1.0, True), ("clip_no_1e-6", 1000, "1e-3", "below", 1.0, True),
]


@pytest.mark.parametrize("variant,step,regime,mn_kind,grad_div,w_zero", ADAM_VARIANTS)
def test_adam_bar_rejects_the_wrong_variant(variant, step, regime, mn_kind, grad_div, w_zero):
    f32, bad = _adam_case(step, regime, mn_kind, grad_div, w_zero, variant)
    bar = R.bar_from(f32["w"])
    _line(f"adam {variant} step={step} |g|={regime} max_norm={mn_kind} div={grad_div} w={'zero' if w_zero else 'randn'}", f32["w"], bad["w"], bar)
    assert f32["w"] <= bar and bad["w"] > bar


@pytest.mark.parametrize("step", R.ADAM_STEPS)
def test_adam_float32_meets_its_bars_on_every_small_case_and_nothing_is_nan(step):
    for regime in R.ADAM_REGIMES:
        for mn_kind in R.ADAM_MAX_NORM:
            for grad_div in R.ADAM_GRAD_DIV:
                for w_zero in (True, False):
                    w, m, v, gs = R.adam_inputs(R.ADAM_N_SMALL, regime, w_zero)
                    mn = R.adam_max_norm(mn_kind, gs[0], grad_div)
                    ref = R.adam_ref(w, m, v, gs, step, mn, grad_div)
                    assert all(np.isfinite(r[k]).all() for r in ref for k in ("w", "m", "v"))
                    e = R.adam_errs(R.adam_f32(w, m, v, gs, step, mn, grad_div), ref)
                    assert all(np.isfinite(x) for x in e.values()), (regime, mn_kind, grad_div, w_zero, e)
                    if regime == "zero":  # w moves only by what m carries: the update is -step_size m' / denom with g = 0
                        assert ref[0]["norm"] == 0.0 and np.all(np.sign(ref[0]["dw"]) == -np.sign(m))


def test_adam_f32_is_torch_optim_adam():
    """The float32 comparison evaluation is torch.optim.Adam + clip_grad_norm_ themselves, to rounding of the update."""
    w, m, v, gs = R.adam_inputs(R.ADAM_N_SMALL, "1e-3", False)
    p = torch.nn.Parameter(torch.from_numpy(w.copy()))
    opt = torch.optim.Adam([p], lr=2.5e-4, eps=1e-5, betas=(0.9, 0.999))
    mine = R.adam_f32(w, np.zeros_like(m), np.zeros_like(v), gs, 1, np.float32(0.01), 1.0)
    for t, g in enumerate(gs):
        p.grad = torch.from_numpy(g.copy())
        torch.nn.utils.clip_grad_norm_([p], 0.01)
        opt.step()
        assert np.abs(p.detach().numpy() - mine[t]["w"]).max() <= 2.0 ** -22 * 2.5e-4 * (t + 1) + 2.0 ** -24 * np.abs(w).max()


# --------------------------------------------------------------------------------------------- batch operations
@pytest.mark.parametrize("n", [256, 257])
def test_normalize_bar_rejects_the_sample_variance(n):
    rng = np.random.default_rng(n)
    x = rng.standard_normal(n).astype(np.float32)
    for pool in (x, np.concatenate([x, rng.standard_normal(n).astype(np.float32) + 0.5])):
        s, ss, cnt, _ = R.moments_ref(pool)
        ref, _, _, scale = R.normalize_ref(x, (s, ss, cnt), 1e-8)
        f32 = R.rel_err(R.normalize_f32(x, pool, 1e-8), ref, scale)
        bad = R.rel_err(R.normalize_f32(x, pool, 1e-8, variant="sample_var"), ref, scale)
        _line(f"normalize n={n} pool={pool.size} sample_var", f32, bad, R.bar_from(f32))
        assert f32 <= R.bar_from(f32) < bad


def test_axpy_data_tell_a_fused_multiply_add_from_two_roundings():
    dst, src, alpha = R.axpy_data(257)
    differ = int((R.axpy_two_roundings(dst, src, alpha).view(np.uint32) != R.axpy_fused(dst, src, alpha).view(np.uint32)).sum())
    print(f"POLOPT64_CPU axpy: {differ} of 257 elements differ between two roundings and a fused multiply-add")
    assert differ >= 10


def test_moments_bar_is_above_a_pairwise_double_sum_and_below_a_float32_sum():
    """n 2^-52 sum |x| admits any double summation order and refuses a float32 accumulator."""
    rng = np.random.default_rng(3)
    x = (1e4 + rng.standard_normal(600001)).astype(np.float32)
    s, ss, cnt, sabs = R.moments_ref(x)
    bar = x.size * 2.0 ** -52 * sabs
    assert abs(float(np.sum(x.astype(np.float64))) - s) <= bar
    assert abs(float(np.cumsum(x.astype(np.float64))[-1]) - s) <= bar  # the sequential order
    assert abs(float(np.sum(x, dtype=np.float32)) - s) > bar
