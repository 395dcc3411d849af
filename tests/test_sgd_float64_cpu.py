"""No GPU: that the bars tests/test_sgd_float64_gpu.py holds the SGD kernels to reject something (tests/sgd_float64.py's
wrong variants are over them in the cases named here), that the floor never exceeds the scale, the --*_opt_optimizer and
--*_opt_adam_beta1=-1 handling of ppo_amd/config.py, and the SGD checkpoint layout against torch.optim.SGD's own."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import policy_optim_float64 as R  # noqa: E402
import sgd_float64 as S  # noqa: E402

N = R.ADAM_N_SMALL
CASES = [(regime, mn, gd) for regime in R.ADAM_REGIMES for mn in R.ADAM_MAX_NORM for gd in R.ADAM_GRAD_DIV]


def _case(regime, mn_kind, grad_div, w_zero=False):
    w, gs = S.sgd_inputs(N, regime, w_zero)
    mn = R.adam_max_norm(mn_kind, gs[0], grad_div)
    return w, gs, mn, S.sgd_ref(w, gs, mn, grad_div)


def _over(variant, regime, mn_kind, grad_div, w_zero=False):
    """Is the variant over the bar for w or the norm in this case?"""
    w, gs, mn, ref = _case(regime, mn_kind, grad_div, w_zero)
    e32 = S.sgd_errs(S.sgd_f32(w, gs, mn, grad_div), ref)
    e = S.sgd_errs(S.sgd_f32(w, gs, mn, grad_div, variant=variant), ref)
    return any(not (e[k] <= R.bar_from(e32[k])) for k in ("w", "norm"))


@pytest.mark.parametrize("regime,mn_kind,grad_div", CASES)
@pytest.mark.parametrize("w_zero", [True, False])
def test_sgd_float32_meets_its_own_bars_and_the_floor_is_below_the_scale(regime, mn_kind, grad_div, w_zero):
    w, gs, mn, ref = _case(regime, mn_kind, grad_div, w_zero)
    e32 = S.sgd_errs(S.sgd_f32(w, gs, mn, grad_div), ref)
    for k in ("w", "norm"):
        assert np.isfinite(e32[k]) and e32[k] <= R.bar_from(e32[k])
    # w's scale is ulp(w) + |dw| of the step: the error is counted in ulps of w where the update is below w's rounding
    # (an earlier step's rounding is carried along and meets a later, smaller scale), as for Adam's w
    assert R.bar_from(e32["norm"]) < 1e-5, e32["norm"]
    for r in ref:
        assert np.all(r["w_scale"] > 0) and np.all(np.isfinite(r["w_scale"]))


def test_clip_without_1e_6_is_over_the_bar_where_the_norm_is_tiny():
    # w = 0, so that an update of 1e-12 is not lost in w's own rounding
    assert _over("clip_no_1e-6", "1e-8", "below", 1.0, w_zero=True)
    assert _over("clip_no_1e-6", "1e-8", "below", 8.0, w_zero=True)


@pytest.mark.parametrize("variant", ["no_grad_div", "norm_undivided"])
@pytest.mark.parametrize("regime", [r for r in R.ADAM_REGIMES if r != "zero"])
def test_a_lost_grad_div_is_over_the_bar_at_grad_div_8(variant, regime):
    # 'norm_undivided' changes the clip only: it shows where the clip acts
    assert _over(variant, regime, "below", 8.0, w_zero=True)
    if variant == "no_grad_div":
        assert all(_over(variant, regime, mn, 8.0, w_zero=True) for mn in R.ADAM_MAX_NORM)


@pytest.mark.parametrize("regime,mn_kind,grad_div", [c for c in CASES if c[0] != "zero"])
def test_the_wrong_sign_is_over_the_bar_everywhere_but_zero(regime, mn_kind, grad_div):
    assert _over("plus", regime, mn_kind, grad_div, w_zero=True)
    if regime in ("1", "1e4", "mix"):  # updates that a randn w's rounding does not swallow
        assert _over("plus", regime, mn_kind, grad_div, w_zero=False)


def test_the_wrong_sign_moves_nothing_when_the_gradient_is_zero():
    assert not _over("plus", "zero", "off", 1.0)


@pytest.mark.parametrize("regime", [r for r in R.ADAM_REGIMES if r != "zero"])
def test_lr_in_the_reported_norm_is_over_the_bar(regime):
    assert _over("lr_in_norm", regime, "off", 1.0)


def test_sgd_f32_is_clip_grad_norm_and_torch_optim_sgd():
    """The comparison evaluation is what the reference runs, clip_grad_norm_ then torch.optim.SGD.step: the norm bit for
    bit, w within one rounding of w and of the update per step (torch's add_(grad, alpha=-lr) may fuse the multiply-add)."""
    for regime, mn_kind in (("1", "below"), ("mix", "above"), ("1e-3", "off")):
        w, gs = S.sgd_inputs(N, regime, False)
        mn = R.adam_max_norm(mn_kind, gs[0], 1.0)
        p = torch.nn.Parameter(torch.from_numpy(w.copy()))
        opt = torch.optim.SGD([p], lr=S.SGD_LR)
        got = S.sgd_f32(w, gs, mn, 1.0)
        for t, (g, step) in enumerate(zip(gs, got)):  # both run free: a step's difference is carried into the next
            p.grad = torch.from_numpy(g.copy())
            norm = torch.nn.utils.clip_grad_norm_([p], float(mn)) if mn > 0 else torch.linalg.vector_norm(p.grad)
            opt.step()
            assert float(norm) == step["norm"]
            tol = (t + 1) * 2.0 ** -23 * (np.abs(step["w"]).astype(np.float64) + S.SGD_LR * np.abs(g))
            assert np.all(np.abs(p.detach().numpy().astype(np.float64) - step["w"]) <= tol)


# --------------------------------------------------------------------------------------------- config
BASE = ["--env_type=synthetic", "--model_encoder=mlp", "--disable_logging=True"]


def _fresh_args():
    from ppo_amd.config import Config
    return Config()


def test_optimizer_flag_holds_sgd_and_refuses_anything_else():
    a = _fresh_args().setup(BASE + ["--policy_opt_optimizer=sgd"])
    assert a.policy_opt.optimizer == "sgd" and a.value_opt.optimizer == "adam"
    for flag in ("policy_opt", "value_opt", "distil_opt", "rnd_opt"):
        with pytest.raises(ValueError, match="Invalid Optimizer foo"):
            _fresh_args().setup(BASE + [f"--{flag}_optimizer=foo"])


def test_adam_beta1_minus_one_resolves_to_one_minus_one_over_the_update_count(capsys, monkeypatch):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    line = BASE + ["--policy_opt_adam_beta1=-1", "--n_steps=128", "--agents=16", "--policy_opt_mini_batch_size=256"]
    a = _fresh_args().setup(line + ["--policy_opt_epochs=2"])
    assert a.policy_opt.adam_beta1 == 1 - 1 / 16
    assert a.value_opt.adam_beta1 == 0.9
    assert f"Set policy_opt beta1 to {1 - 1 / 16}" in capsys.readouterr().out
    with pytest.raises(ValueError, match="policy_opt_adam_beta1"):
        _fresh_args().setup(line + ["--policy_opt_epochs=0"])
    # every group, and the rollout is what all ranks see together
    monkeypatch.setenv("WORLD_SIZE", "2")
    a = _fresh_args().setup(BASE + ["--rnd_opt_adam_beta1=-1", "--n_steps=128", "--agents=16", "--rnd_opt_mini_batch_size=256",
                                    "--rnd_opt_epochs=1", "--policy_opt_optimizer=sgd", "--policy_opt_adam_beta1=-1"])
    assert a.rnd_opt.adam_beta1 == 1 - 1 / 16
    assert a.policy_opt.optimizer == "sgd"  # the Adam flags of an SGD group are accepted


# --------------------------------------------------------------------------------------------- checkpoint layout
@pytest.mark.parametrize("n_parameters,lr", [(1, 2.5e-4), (7, 0.01)])
def test_sgd_state_dict_is_torch_optim_sgds_key_for_key(n_parameters, lr):
    from ppo_amd.models import sgd_state_dict
    want = torch.optim.SGD([torch.nn.Parameter(torch.zeros(3, 2)) for _ in range(n_parameters)], lr=lr).state_dict()
    got = sgd_state_dict(n_parameters, lr)
    assert got == want
    assert got["state"] == {} and len(got["param_groups"]) == 1
    group = got["param_groups"][0]
    assert list(group.keys()) == list(want["param_groups"][0].keys())
    assert group["lr"] == lr and group["params"] == list(range(n_parameters)) and group["momentum"] == 0


def test_a_state_dict_of_the_other_kind_is_refused():
    from ppo_amd.models import check_optimizer_layout, optimizer_layout_kind, sgd_state_dict
    p = [torch.nn.Parameter(torch.zeros(2))]
    adam, sgd = torch.optim.Adam(p).state_dict(), sgd_state_dict(1, 0.1)
    assert optimizer_layout_kind(adam) == "adam" and optimizer_layout_kind(sgd) == "sgd"
    assert optimizer_layout_kind({"flat": {}, "step": 3}) == "adam"
    check_optimizer_layout(adam, "adam")
    check_optimizer_layout(sgd, "sgd")
    with pytest.raises(ValueError, match="adam.*sgd"):
        check_optimizer_layout(adam, "sgd")
    with pytest.raises(ValueError, match="sgd.*adam"):
        check_optimizer_layout(sgd, "adam")
    with pytest.raises(ValueError, match="adam.*sgd"):
        check_optimizer_layout({"flat": {}, "step": 3}, "sgd")
