"""CPU: the flags of Random Network Distillation and the host half of the intrinsic returns.

tests/golden/rnd_runner_golden.npz part (g) (tests/golden/make_rnd_golden.py --runner) scripts two consecutive rollouts of
intrinsic rewards [6, 5] (one of them 7.0, clipped to 5 as generate_rollout does) through the reference's
calculate_intrinsic_returns, with --ir_propagation on and off.  Everything the host computes - the forward EMS filter, the
running moments of its output and the normalisation scale - is float64 arithmetic written expression for expression as the
reference's, so it must carry the same bits."""
import json
import os

import numpy as np
import pytest

from ppo_amd import checkpoint
from ppo_amd.config import Config
from ppo_amd.rollout import intrinsic_return_scale
from ppo_amd.running_stats import RunningMeanStd


@pytest.fixture(scope="module")
def gold(golden_dir):
    return (np.load(os.path.join(golden_dir, "rnd_runner_golden.npz")),
            json.load(open(os.path.join(golden_dir, "rnd_runner_golden.json"))))


def test_flags_parse_to_the_references_defaults():
    c = Config().setup([])
    assert c.rnd.enabled is False and c.rnd.experience_proportion == 0.25          # rl/config.py:402-403
    assert (c.ir.propagation, c.ir.scale, c.ir.center, c.ir.normalize) == (True, 0.3, False, True)  # :449-452
    assert c.gamma_int == 0.99                                                      # :770
    o = c.rnd_opt                                                                   # :267-285
    assert (o.optimizer, o.epochs, o.mini_batch_size, o.lr, o.lr_anneal) == ("adam", 1, 256, 2.5e-4, False)
    assert (o.adam_epsilon, o.adam_beta1, o.adam_beta2) == (1e-5, 0.9, 0.999)
    assert c.use_intrinsic_rewards is False and c.flatten()["use_intrinsic_rewards"] is False
    on = Config().setup(["--rnd_enabled=True", "--observation_normalization=True", "--rnd_experience_proportion=0.5",
                         "--rnd_opt_lr=1e-3", "--rnd_opt_epochs=2", "--ir_scale=0.5", "--ir_center=True",
                         "--ir_normalize=False", "--ir_propagation=False", "--gamma_int=0.9"])
    assert on.rnd.enabled is True and on.use_intrinsic_rewards is True and on._ignored == []
    assert (on.rnd.experience_proportion, on.rnd_opt.lr, on.rnd_opt.epochs) == (0.5, 1e-3, 2)
    assert (on.ir.scale, on.ir.center, on.ir.normalize, on.ir.propagation, on.gamma_int) == (0.5, True, False, False, 0.9)
    flat = on.flatten()
    assert flat["rnd_enabled"] is True and flat["rnd_opt_lr"] == 1e-3 and flat["ir_scale"] == 0.5


def test_rnd_needs_observation_normalization():
    with pytest.raises(AssertionError, match="RND requires observation normalization"):
        Config().setup(["--rnd_enabled=True"])
    with pytest.raises(AssertionError, match="RND requires observation normalization"):
        Config().setup(["--rnd_enabled=True", "--observation_normalization=False"])


def test_with_rnd_off_nothing_else_is_parsed_differently():
    # flags of subsystems that are still not built are ignored with a note, as before; the RND flags no longer are
    c = Config().setup(["--hash_bonus=0.1", "--replay_size=4", "--agents=8"])
    assert c._ignored == ["--hash_bonus=0.1", "--replay_size=4"] and c.agents == 8
    assert Config().setup(["--use_intrinsic_rewards=True"])._ignored == []  # still accepted; follows --rnd_enabled
    assert Config().setup(["--use_intrinsic_rewards=True"]).use_intrinsic_rewards is False
    assert Config().setup([])._ignored == []
    # the groups of the other optimisers keep their epoch defaults
    c = Config().setup([])
    assert (c.policy_opt.epochs, c.value_opt.epochs, c.distil_opt.epochs) == (2, 1, 2)


@pytest.mark.parametrize("prop", [1, 0])
def test_host_half_of_the_intrinsic_returns_is_bit_exact(gold, prop):
    g, meta = gold
    assert meta["g_dtypes"][f"g_prop{prop}_center0_r0_rewards"] == "float64"  # NumPy >= 2 wrote the fixture
    rewards, terminals = g["g_int_rewards"], g["g_terminals"]
    assert rewards[0, 2, 3] == 7.0 and rewards.dtype == np.float32 and terminals.dtype == bool and terminals.any()
    ems, rms = np.zeros([rewards.shape[2]]), RunningMeanStd(shape=())
    for r in range(2):
        ems, scale = intrinsic_return_scale(ems, rms, np.clip(rewards[r], -5, 5), terminals[r], meta["gamma_int"], bool(prop))
        for center in (0, 1):  # centring happens after the host half: both cases recorded the same host state
            key = f"g_prop{prop}_center{center}_r{r}_"
            assert ems.dtype == np.float64 and ems.tobytes() == g[key + "ems_norm"].tobytes()
            got = np.asarray([rms.mean, rms.var, rms.count], np.float64)
            assert got.tobytes() == g[key + "rms"].tobytes(), (got, g[key + "rms"])
            assert np.float64(scale).tobytes() == g[key + "scale"].tobytes()
    # the two settings differ: a terminal cuts the filter only without propagation
    assert not np.array_equal(g["g_prop1_center0_r1_ems_norm"], g["g_prop0_center0_r1_ems_norm"])


def test_rnd_checkpoint_entries_survive_the_plain_container(tmp_path):
    rms = RunningMeanStd(shape=())
    ems, _scale = intrinsic_return_scale(np.zeros([3]), rms, np.arange(6, dtype=np.float32).reshape(2, 3) / 7,
                                         np.zeros((2, 3), bool), 0.99, True)
    data = {"ems_norm": ems, "intrinsic_returns_rms": {"mean": np.float64(rms.mean), "var": np.float64(rms.var),
                                                       "count": float(rms.count)}}
    path = checkpoint.save(data, str(tmp_path / "c.pt"), False)
    back = checkpoint.load(path)
    assert back["ems_norm"].dtype == np.float64 and back["ems_norm"].tobytes() == ems.tobytes()
    for k in ("mean", "var"):
        assert np.float64(back["intrinsic_returns_rms"][k]).tobytes() == np.float64(getattr(rms, k)).tobytes()
    assert back["intrinsic_returns_rms"]["count"] == rms.count
