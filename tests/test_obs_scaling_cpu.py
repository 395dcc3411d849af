"""No GPU: --observation_scaling=scaled|centered|unit.

The two signed preparations written out in torch for all 256 bytes, with the number of bytes at which every tempting
shortcut differs from them: what makes the exhaustive table test of tests/test_obs_scaling_gpu.py tell the right form of
a kernel's load from the wrong ones.  Then the flag's way from the command line into the model: config parsing, the
reference's ValueError, train.py's forwarding, and the library's argument checks for the new mode values."""
import pytest

torch = pytest.importorskip("torch")

import obs_scaling_torch as O  # noqa: E402
from ppo_amd import _lib  # noqa: E402
from ppo_amd.config import Config  # noqa: E402


def test_the_subtraction_is_inexact_for_63_bytes():
    q = O.all_bytes().float() / 255.0
    assert int(((q - 0.5).double() != q.double() - 0.5).sum()) == 63


def test_the_reference_expressions_and_their_end_points():
    c, u = O.table("centered"), O.table("unit")
    assert c.dtype == u.dtype == torch.float32
    assert (float(c[0]), float(c[255]), float(u[0]), float(u[255])) == (-0.5, 0.5, -3.0, 3.0)
    assert torch.equal(O.table("scaled"), O.all_bytes().float() / 255.0)
    assert torch.equal(c, O.all_bytes().float() / 255.0 - 0.5)  # the `* 1` changes nothing
    assert torch.equal(u, c * 6)
    for s in O.SIGNED:  # strictly increasing: a byte is recognisable from its value
        assert bool((O.table(s)[1:] > O.table(s)[:-1]).all())
    with pytest.raises(ValueError, match="Invalid observation_scaling mode half"):
        O.prep(O.all_bytes(), "half")


def test_every_shortcut_is_wrong_somewhere():
    """A fused multiply-add, a folded scale and a single rounding of the exact value each miss the reference's bits at
    many bytes, so a kernel that takes one of them cannot pass a comparison over all 256."""
    unit, centered = O.shortcuts("unit"), O.shortcuts("centered")
    assert O.differing(unit["fma"], O.table("unit")) == 31
    assert O.differing(unit["folded_scale"], O.table("unit")) == 149
    assert O.differing(centered["single_rounding"], O.table("centered")) == 128
    assert O.differing(unit["single_rounding"], O.table("unit")) == 180
    # (the helper's single rounding is the nearest float32 indeed)
    for s in O.SIGNED:
        got, want = O.shortcuts(s)["single_rounding"].double(), torch.tensor([float(v) for v in O.exact(s)], dtype=torch.float64)
        assert float((got - want).abs().max()) <= 2.0 ** -24 * 3.0


def test_constants_match_the_header():
    import os
    import re
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "ppo_amd.h")).read()
    defines = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (PPO_\w+) (\d+)\b", header)}
    for name in ("PPO_IN_U8", "PPO_IN_U8_CENTERED", "PPO_IN_U8_UNIT", "PPO_OBS_F32", "PPO_OBS_U8", "PPO_OBS_U8_CENTERED",
                 "PPO_OBS_U8_UNIT", "PPO_HASH_NORMED_CENTERED", "PPO_HASH_NORMED_OFFSET_CENTERED", "PPO_HASH_NORMED_UNIT",
                 "PPO_HASH_NORMED_OFFSET_UNIT"):
        assert defines[name] == getattr(_lib, name), name
    assert [O.IN_MODE[s] for s in O.SCALINGS] == [_lib.PPO_IN_U8, _lib.PPO_IN_U8_CENTERED, _lib.PPO_IN_U8_UNIT]
    assert [O.OBS_PREP[s] for s in O.SCALINGS] == [_lib.PPO_OBS_U8, _lib.PPO_OBS_U8_CENTERED, _lib.PPO_OBS_U8_UNIT]
    from ppo_amd import hashing, models
    assert {s: v[0] for s, v in models.OBSERVATION_SCALINGS.items()} == O.IN_MODE
    assert {s: v[1] for s, v in models.OBSERVATION_SCALINGS.items()} == O.OBS_PREP
    assert hashing.NORMED_MODES == O.HASH_MODE


@pytest.mark.parametrize("scaling", O.SCALINGS)
def test_config_accepts_the_three_values(scaling):
    c = Config()
    c.setup([f"--observation_scaling={scaling}"])
    assert c.observation_scaling == scaling


def test_config_default_and_refusal():
    c = Config()
    c.setup([])
    assert c.observation_scaling == "scaled"
    with pytest.raises(ValueError, match="Invalid observation_scaling mode halved"):
        Config().setup(["--observation_scaling=halved"])


def test_the_model_layer_refuses_other_values_with_the_reference_message():
    from ppo_amd import models
    assert models.check_observation_scaling("unit") == "unit"
    with pytest.raises(ValueError, match="^Invalid observation_scaling mode None$"):
        models.check_observation_scaling(None)
    # before anything touches a GPU: TVFModel, DualHeadNet and ObsNormalizer check their argument first
    with pytest.raises(ValueError, match="Invalid observation_scaling mode x"):
        models.TVFModel("impala", observation_scaling="x")
    with pytest.raises(ValueError, match="Invalid observation_scaling mode x"):
        models.DualHeadNet("impala", (4, 84, 84), 6, observation_scaling="x")
    with pytest.raises(ValueError, match="Invalid observation_scaling mode x"):
        models.ObsNormalizer((4, 84, 84), "cpu", observation_scaling="x")


@pytest.mark.parametrize("scaling", O.SCALINGS)
def test_train_py_forwards_the_flag(monkeypatch, scaling):
    import train
    from ppo_amd import envs, models
    seen = {}

    def fake_model(**kw):
        seen.update(kw)
        return "model"

    monkeypatch.setattr(models, "TVFModel", fake_model)
    monkeypatch.setattr(envs, "get_env_spec", lambda: ((4, 84, 84), 6))
    train.args.setup([f"--observation_scaling={scaling}"])
    try:
        assert train.make_model(None) == "model"
    finally:
        train.args.setup([])
    assert seen["observation_scaling"] == scaling


def test_new_mode_values_pass_the_argument_checks_and_the_gaps_stay_refused(hip_lib):
    """Host-side checks only (no launch: n = 0, a probe, or a refusal that comes first)."""
    lib, P = hip_lib, 1 << 12
    for mode in (_lib.PPO_IN_U8_CENTERED, _lib.PPO_IN_U8_UNIT):
        for cin, side in ((4, 84), (5, 84), (3, 64), (4, 64)):
            assert lib.ppo_conv3x3_forward_supported(mode, cin, 16, side, side)
            assert lib.ppo_conv3x3_pool_forward_supported(mode, cin, 16, side, side)
            assert lib.ppo_conv3x3_backward_weight_supported(mode, cin, 16, side, side)
        assert not lib.ppo_conv3x3_forward_supported(mode, 16, 32, 42, 42)   # float maps only
        assert not lib.ppo_conv3x3_forward_supported(mode, 4, 16, 80, 80)
        assert lib.ppo_conv3x3_forward_f32(P, mode, P, P, None, P, 0, 4, 16, 84, 84, None) == 0
        # a geometry without a kernel is refused as such, not as an unknown mode
        assert lib.ppo_conv3x3_forward_f32(P, mode, P, P, None, P, 1, 7, 16, 30, 30, None) == -1
        assert b"unsupported geometry" in lib.ppo_last_error()
        # the generic and the strided families: refused for the null pointer, not for the mode
        assert lib.ppo_conv3x3_any_forward_f32(None, mode, P, P, None, P, 1, 3, 5, 7, 9, None) == -1
        assert b"in_mode" not in lib.ppo_last_error()
        assert lib.ppo_conv2d_strided_forward_f32(None, mode, P, P, P, 1, 1, 4, 36, 36, 32, 8, 8, 4, None) == -1
        assert b"in_mode" not in lib.ppo_last_error()
    # 3 stays no mode
    assert not lib.ppo_conv3x3_forward_supported(3, 4, 16, 84, 84)
    assert lib.ppo_conv3x3_any_forward_f32(P, 3, P, P, None, P, 1, 3, 5, 7, 9, None) == -1 and b"in_mode" in lib.ppo_last_error()
    assert lib.ppo_conv2d_strided_forward_f32(P, 3, P, P, P, 1, 1, 4, 36, 36, 32, 8, 8, 4, None) == -1
    assert b"in_mode" in lib.ppo_last_error()
    # observation preparations 0..3, hash modes 0..3 and 8..11
    assert lib.ppo_obs_normalize_f32(P, 3, P, P, 0.0, P, 0, 16, None) == 0
    assert lib.ppo_obs_normalize_f32(P, 4, P, P, 0.0, P, 1, 16, None) == -1 and b"is_u8" in lib.ppo_last_error()
    assert lib.ppo_obs_moments_f64(P, -1, 1, 16, P, None) == -1 and b"is_u8" in lib.ppo_last_error()
    assert lib.ppo_obs_normalize_channel_f32(P, 4, None, P, P, 0.0, P, 1, 2, 4, 4, 1, None) == -1 and b"is_u8" in lib.ppo_last_error()
    for mode in (8, 9, 10, 11):  # normed: mu / std are required
        assert lib.ppo_state_hash_i32(P, 2, 4, 8, 8, 1, 0, mode, None, None, 0.0, P, P, 16, P, None) == -1
        assert b"null" in lib.ppo_last_error()
        assert lib.ppo_state_hash_i32(P, 0, 4, 8, 8, 1, 0, mode, P, P, 0.0, P, P, 16, P, None) == 0
    for mode in (4, 5, 6, 7, 12, -1):
        assert lib.ppo_state_hash_i32(P, 2, 4, 8, 8, 1, 0, mode, P, P, 0.0, P, P, 16, P, None) == -1
        assert b"mode" in lib.ppo_last_error()
