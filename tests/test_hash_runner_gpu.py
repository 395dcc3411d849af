"""GPU: state hashing in the Runner - the hashes written during the pipelined and the generic rollout, the count tables and
the bonus after it, the intrinsic path without RND, the sum with RND, the normed inputs against the normaliser's statistics,
checkpoint and reset.  The set-up is that of tests/test_rnd_runner_gpu.py: nature encoder, synthetic env 4 x 36 x 36 (all
4 * 36 * 36 elements are hashed: the env type is not atari), 8 agents, 4 - 6 steps, 8 hash bits so that bins collide.

Everything is compared exactly: hashes with the float64 NumPy projection (tests/hash_numpy.py; each test asserts that no
projection of its inputs lies inside the float64 rounding bound), tables with the reference's float64 loop byte for byte,
rewards with float32(float64(r) + bonus * g) byte for byte."""
import os

import numpy as np
import pytest

import hash_numpy as HN

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from ppo_amd import checkpoint, logger, models, rollout  # noqa: E402
from ppo_amd.config import args  # noqa: E402
from ppo_amd.vec_env import SplitVecEnv, SyntheticVecEnv  # noqa: E402

DIMS, N_ACTIONS, BITS = (4, 36, 36), 6, 8
FLAGS = ["--model_encoder=nature", "--env_type=synthetic", "--env_embed_time=False", "--env_synthetic_shape=4,36,36",
         "--seed=5", "--disable_logging=True", "--device=cuda", "--model_architecture=single",
         "--policy_opt_mini_batch_size=16", "--policy_opt_epochs=1", "--value_opt_mini_batch_size=16", "--value_opt_epochs=1",
         "--distil_opt_mini_batch_size=16", "--rnd_opt_mini_batch_size=8"]
HASH = ["--hash_enabled=True", f"--hash_bits={BITS}"]


@pytest.fixture(scope="module")
def norm_state(golden_dir):
    g = np.load(os.path.join(golden_dir, "rnd_runner_golden.npz"))  # an observation normaliser that has seen data
    return {"mean": g["f_obs_mean"], "var": g["f_obs_var"], "count": float(g["f_obs_count"])}


def make_runner(extra=(), agents=8, n_steps=4, parts=2, norm=None, frozen=False, generic=False, seed=5):
    flags = [*FLAGS, f"--agents={agents}", f"--n_steps={n_steps}", *extra]
    if norm is not None:
        flags += ["--observation_normalization=True"] + (["--freeze_observation_normalization=True"] if frozen else [])
    args.setup(flags)
    np.random.seed(11)
    torch.manual_seed(seed)
    model = models.TVFModel(encoder="nature", input_dims=DIMS, actions=N_ACTIONS, device="cuda", architecture="single",
                            hidden_units=64, use_rnd=bool(args.rnd.enabled), observation_normalization=norm is not None,
                            head_scale=0.1, head_bias=True, freeze_observation_normalization=frozen,
                            value_head_names=("ext", "int") if args.use_intrinsic_rewards else ("ext",))
    if norm is not None:
        model.obs_norm.load_state_dict(norm)
    r = rollout.Runner(model, logger.Logger(quiet=True))
    per = agents // parts
    envs_ = [SyntheticVecEnv(per, obs_shape=DIMS, n_actions=N_ACTIONS, seed=3, p_done=0.1, env_offset=i * per, threads=2)
             for i in range(parts)]
    r.vec_env = envs_[0] if parts == 1 else SplitVecEnv(envs_)
    r.reset()
    r.force_generic_rollout = generic
    return r


def numpy_hashes(r, mode="raw", quantize=1, mu=None, std=None, eps=0.0):
    """Hashes of all_obs[1:] by the float64 projection, [N, A]; asserts that no bit of them is in doubt."""
    obs = r.all_obs[1:].cpu().numpy().reshape(r.N * r.A, *DIMS)
    h = r.hash.hasher
    want, p, bound = HN.project(HN.hash_input(obs, DIMS[0], mode, quantize, mu, std, eps), h.weight.cpu().numpy(),
                                h.bias.cpu().numpy())
    assert not (np.abs(p) <= bound).any(), "an observation of this run lies inside the rounding bound"
    return want.reshape(r.N, r.A)


def tables(r):
    torch.cuda.synchronize()
    return r.hash.global_counts.cpu().numpy(), r.hash.recent_counts.cpu().numpy()


BONUS = [*HASH, "--hash_bonus=0.25"]


def test_pipelined_and_generic_rollouts_agree_and_match_numpy():
    a = make_runner(BONUS, n_steps=5)
    b = make_runner(BONUS, n_steps=5, generic=True)
    assert a.hash.n_bins == 256 and a.hash.hasher.in_d == 4 * 36 * 36 and a.hash.obs_hashes.dtype == torch.int32
    want_g, want_r = np.zeros(256), np.zeros(256)
    for rollouts in (1, 2):
        a.generate_rollout()
        b.generate_rollout()
        ga, ra = tables(a)
        gb, rb = tables(b)
        assert torch.equal(a.all_obs, b.all_obs)
        assert torch.equal(a.hash.obs_hashes, b.hash.obs_hashes)
        assert ga.tobytes() == gb.tobytes() and ra.tobytes() == rb.tobytes()
        assert torch.equal(a.int_rewards, b.int_rewards)
        hashes = a.hash.obs_hashes.cpu().numpy()
        assert np.array_equal(hashes, numpy_hashes(a))
        HN.count_loop(hashes, args.hash.decay, want_g, want_r)
        assert ga.tobytes() == want_g.tobytes() and ra.tobytes() == want_r.tobytes()
        assert ga.sum() == a.N * a.A * rollouts
        assert len(np.unique(hashes)) > 4 and (np.bincount(hashes.reshape(-1)) > 1).any()  # spread out, and colliding
        # the bonus of the hash-only intrinsic path: 0 + bonus / recent[h], from the final recent counts
        assert a.int_rewards.cpu().numpy().tobytes() == HN.bonus(np.zeros((a.N, a.A), np.float32), hashes, ra, "hyperbolic",
                                                                 0.25).tobytes()
        assert a.hash.stats() == (int(np.count_nonzero(ga)), int(np.count_nonzero(ra.astype(int))))


def test_tracking_only_changes_nothing_else():
    on = make_runner(HASH)
    off = make_runner()
    assert on.VH == 1 and on.value_heads == ["ext"] and not on.intrinsic and not hasattr(on, "int_rewards")
    assert off.hash is None and on.hash is not None and args.use_intrinsic_rewards is False
    for r in (on, off):
        np.random.seed(11)  # the minibatch permutations of train()
        r.generate_rollout()
        r.calculate_returns()
        r.train()
    torch.cuda.synchronize()
    for name in ("all_obs", "actions", "value", "ext_rewards", "log_pac", "advantage", "returns"):
        assert torch.equal(getattr(on, name), getattr(off, name)), name
    assert torch.equal(on.policy_net.flat, off.policy_net.flat)
    g, _r = tables(on)
    assert g.sum() == on.N * on.A


@pytest.mark.parametrize("method", ["hyperbolic", "quadratic", "binary"])
def test_bonus_without_rnd_trains_the_int_head(method):
    r = make_runner([*BONUS, f"--hash_bonus_method={method}"], n_steps=6)
    assert r.VH == 2 and r.value_heads == ["ext", "int"] and r.rnd is None and r.rnd_optimizer is None and r.intrinsic
    r.int_rewards.fill_(3.0)  # a rollout starts from zero intrinsic rewards
    r.generate_rollout()
    _g, recent = tables(r)
    hashes = r.hash.obs_hashes.cpu().numpy()
    threshold = r.hash.last_threshold if method == "binary" else None
    if method == "binary":
        assert np.float64(threshold).tobytes() == np.float64(r.hash.threshold(recent)).tobytes()
    want = HN.bonus(np.zeros((r.N, r.A), np.float32), hashes, recent, method, 0.25, threshold)
    assert r.int_rewards.cpu().numpy().tobytes() == want.tobytes()
    if method == "hyperbolic":
        assert want.tobytes() == np.float32(0.25 / recent[hashes]).tobytes()
    before = r.policy_net.flat.clone()
    r.calculate_returns()
    assert r.int_returns.abs().max() > 0 and torch.isfinite(r.advantage).all()
    r.train()
    torch.cuda.synchronize()
    stats = r.fetch_stats()
    assert np.isfinite([float(v) for v in stats.values()]).all() and "loss_rnd" not in stats, stats
    assert torch.isfinite(r.policy_net.flat).all() and not torch.equal(r.policy_net.flat, before)
    assert r.policy_net.grads["value_head.weight"].abs().amax(1).min() > 0  # both heads' rows learn, the int head's too


def test_bonus_with_rnd_is_added_to_the_prediction_error(norm_state):
    rnd = ["--rnd_enabled=True"]
    a = make_runner(rnd, norm=norm_state)
    b = make_runner([*rnd, *BONUS], norm=norm_state)
    a.generate_rollout()
    b.generate_rollout()
    _g, recent = tables(b)
    assert torch.equal(a.all_obs, b.all_obs) and torch.equal(a.actions, b.actions)
    raw = a.int_rewards.cpu().numpy()
    assert raw.min() > 0
    want = HN.bonus(raw, b.hash.obs_hashes.cpu().numpy(), recent, "hyperbolic", 0.25)
    assert b.int_rewards.cpu().numpy().tobytes() == want.tobytes()
    b.calculate_returns()
    b.train()
    torch.cuda.synchronize()
    assert b.rnd.adam_steps == 1 and torch.isfinite(b.policy_net.flat).all()


@pytest.mark.parametrize("mode", ["normed", "normed_offset"])
def test_normed_input_with_a_frozen_normaliser_matches_numpy(norm_state, mode):
    r = make_runner([*HASH, f"--hash_input={mode}", "--hash_quantize=8"], norm=norm_state, frozen=True, n_steps=5)
    r.generate_rollout()
    torch.cuda.synchronize()
    n = r.model.obs_norm
    want = numpy_hashes(r, mode, 8, n.mu.cpu().numpy(), n.std.cpu().numpy(), n.norm_eps)
    assert np.array_equal(r.hash.obs_hashes.cpu().numpy(), want)
    assert len(np.unique(want)) > 1


def test_normed_input_with_a_live_normaliser_agrees_between_the_rollout_forms(norm_state):
    a = make_runner([*HASH, "--hash_input=normed"], norm=norm_state, n_steps=5)
    b = make_runner([*HASH, "--hash_input=normed"], norm=norm_state, n_steps=5, generic=True)
    for _ in range(2):
        a.generate_rollout()
        b.generate_rollout()
        torch.cuda.synchronize()
        assert torch.equal(a.all_obs, b.all_obs) and torch.equal(a.model.obs_norm.mu, b.model.obs_norm.mu)
        assert torch.equal(a.hash.obs_hashes, b.hash.obs_hashes)
    # the statistics moved during the rollout, and the last row was hashed with the last constants
    n = a.model.obs_norm
    last = HN.project(HN.hash_input(a.all_obs[a.N].cpu().numpy(), 4, "normed", 1, n.mu.cpu().numpy(), n.std.cpu().numpy(),
                                    n.norm_eps), a.hash.hasher.weight.cpu().numpy(), a.hash.hasher.bias.cpu().numpy())
    assert not (np.abs(last[1]) <= last[2]).any()
    assert np.array_equal(a.hash.obs_hashes[a.N - 1].cpu().numpy(), last[0])
    assert tables(a)[0].tobytes() == tables(b)[0].tobytes() and tables(a)[1].tobytes() == tables(b)[1].tobytes()


def test_checkpoint_round_trip_and_reset(tmp_path):
    a = make_runner(BONUS)
    a.generate_rollout()
    a.calculate_returns()
    a.train()
    ga, ra = tables(a)
    assert ga.sum() == 32 and ra.any()
    path = a.save_checkpoint(str(tmp_path / "checkpoint-000M-params.pt"), a.step)
    cp = checkpoint.load(path)
    for key, table in (("hash_global_counts", ga), ("hash_recent_counts", ra)):  # rl/rollout.py:409-411
        assert isinstance(cp[key], np.ndarray) and cp[key].dtype == np.float64 and cp[key].shape == (256,)
        assert cp[key].tobytes() == table.tobytes()
    assert "ems_norm" in cp and "intrinsic_returns_rms" in cp and "rnd_optimizer_state_dict" not in cp
    b = make_runner(BONUS, seed=6)
    assert not tables(b)[0].any()
    assert b.load_checkpoint(path) == 32
    gb, rb = tables(b)
    assert gb.tobytes() == ga.tobytes() and rb.tobytes() == ra.tobytes()
    assert b.ems_norm.tobytes() == a.ems_norm.tobytes()
    # the resumed run counts on from the restored tables
    a.generate_rollout()
    b.generate_rollout()
    assert torch.equal(a.all_obs, b.all_obs)
    assert tables(a)[0].tobytes() == tables(b)[0].tobytes() and tables(a)[1].tobytes() == tables(b)[1].tobytes()
    assert tables(a)[0].sum() == 64
    a.reset()
    assert not tables(a)[0].any() and not tables(a)[1].any()
    # without hashing a checkpoint has neither key
    off = make_runner()
    cp = checkpoint.load(off.save_checkpoint(str(tmp_path / "off.pt"), 0))
    assert "hash_global_counts" not in cp and "hash_recent_counts" not in cp and "ems_norm" not in cp


def test_the_three_log_lines():
    r = make_runner([*BONUS, "--disable_logging=False", "--disable_ev=True"])
    seen = 0
    for _ in range(2):
        r.generate_rollout()
        r.calculate_returns()
        g, rec = tables(r)
        states = int(np.count_nonzero(g))
        assert r.log["hash_states"] == states and r.log["*hash_delta"] == states - seen  # rl/rollout.py:1243-1250
        assert r.log["*hash_recent"] == int(np.count_nonzero(rec.astype(int)))
        seen = states
    assert seen > 4


def test_train_main_with_a_hash_bonus_runs_and_logs_hash_states(monkeypatch, tmp_path):
    import sys
    import train
    batch = 32 * 16
    monkeypatch.setattr(sys, "argv", [
        "train.py", "--agents=32", "--n_steps=16", "--model_architecture=single", "--model_encoder=nature",
        "--env_type=synthetic", "--env_embed_time=False", "--seed=4", "--policy_opt_mini_batch_size=128",
        "--policy_opt_epochs=1", "--env_warmup_period=5", "--experiment_name=exp", "--run_name=hash_test",
        f"--output_folder={tmp_path}", f"--epochs={(2 * batch - 1) / 1e6}", "--hash_enabled=True", "--hash_bonus=0.01"])
    r = train.main()
    assert r.step == 2 * batch and r.hash is not None and r.VH == 2 and r.rnd is None and args._ignored == []
    assert r.model.policy_net.value_head_names == ["ext", "int"]
    g, _rec = tables(r)
    assert g.sum() == 2 * batch and r.log["hash_states"] == np.count_nonzero(g) > 0
    assert "hash_states" in open(os.path.join(args.log_folder, "training_log.csv")).readline()
    assert torch.isfinite(r.net.flat).all()


def test_hashing_refuses_what_it_cannot_do(norm_state):
    with pytest.raises(ValueError, match="observation_normalization"):
        make_runner([*HASH, "--hash_input=normed"])
    args.setup([*FLAGS, "--agents=8", "--n_steps=4", *BONUS])
    torch.manual_seed(5)
    one_head = models.TVFModel(encoder="nature", input_dims=DIMS, actions=N_ACTIONS, device="cuda", architecture="single",
                               hidden_units=64, head_scale=0.1, head_bias=True, value_head_names=("ext",))
    with pytest.raises(NotImplementedError, match="value heads"):
        rollout.Runner(one_head, logger.Logger(quiet=True))
