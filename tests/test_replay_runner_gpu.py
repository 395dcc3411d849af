"""GPU: the replay buffer in the Runner - what an iteration adds, the distil batch drawn from it, the distil phase trained
on that batch, checkpoints, and that nothing moves with replay off.  The set-up is that of tests/test_hash_runner_gpu.py
(nature encoder, synthetic env 4 x 36 x 36, 8 agents, 4 steps) with the dual architecture, whose distil phase is what reads
the buffer.

Everything is compared exactly: buffers with the NumPy restatement of the reference's buffer (tests/replay_numpy.py, itself
checked against the reference's recorded results in tests/test_replay_cpu.py) driven from the same np.random seed, sampled
rows with torch indexing, targets with the networks' own forwards, trained parameters bit for bit."""
import numpy as np
import pytest

import replay_numpy as RN

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from ppo_amd import checkpoint, logger, models, rollout  # noqa: E402
from ppo_amd.config import args  # noqa: E402
from ppo_amd.replay import ExperienceReplayBuffer as Buffer  # noqa: E402
from ppo_amd.vec_env import SplitVecEnv, SyntheticVecEnv  # noqa: E402

DIMS, N_ACTIONS, AGENTS, STEPS = (4, 36, 36), 6, 8, 4
BATCH = AGENTS * STEPS
FLAGS = ["--model_encoder=nature", "--env_type=synthetic", "--env_embed_time=False", "--env_synthetic_shape=4,36,36",
         "--seed=5", "--disable_logging=True", "--device=cuda", "--model_architecture=dual", f"--agents={AGENTS}",
         f"--n_steps={STEPS}", "--policy_opt_mini_batch_size=16", "--policy_opt_epochs=1", "--value_opt_mini_batch_size=16",
         "--value_opt_epochs=1", "--distil_opt_mini_batch_size=16", "--distil_opt_epochs=2", "--max_micro_batch_size=24"]
REPLAY = ["--replay_mode=uniform", "--replay_size=64", "--distil_batch_size=48"]


@pytest.fixture(autouse=True)
def restore_micro_batch_size():
    """--max_micro_batch_size=24 (two forward chunks per distil batch) is a top-level flag: a later args.setup() without it
    would keep the value, so it is put back for the files that run after this one."""
    before = args.max_micro_batch_size
    yield
    args.max_micro_batch_size = before


IMPALA_DIMS = (4, 84, 84)  # where the IMPALA nets read uint8 rows through the minibatch index in their first convolution


def make_runner(extra=(), seed=5, parts=2, encoder="nature"):
    dims = DIMS if encoder == "nature" else IMPALA_DIMS
    args.setup([*FLAGS, *extra, f"--model_encoder={encoder}", "--env_synthetic_shape=" + ",".join(map(str, dims))])
    np.random.seed(11)
    torch.manual_seed(seed)
    model = models.TVFModel(encoder=encoder, input_dims=dims, actions=N_ACTIONS, device="cuda", architecture="dual",
                            hidden_units=64, head_scale=0.1, head_bias=True, value_head_names=("ext",))
    r = rollout.Runner(model, logger.Logger(quiet=True))
    per = AGENTS // parts
    envs_ = [SyntheticVecEnv(per, obs_shape=dims, n_actions=N_ACTIONS, seed=3, p_done=0.1, env_offset=i * per, threads=2)
             for i in range(parts)]
    r.vec_env = SplitVecEnv(envs_)
    r.reset()
    return r


def iteration(r, seed):
    """One rollout + returns + training with the host RNG seeded, so that two Runners (and NumPy) draw alike."""
    r.generate_rollout()
    np.random.seed(seed)
    r.calculate_returns()
    r.train()
    torch.cuda.synchronize()


def rollout_rows(r):
    """What the reference hands to add_experience (rl/rollout.py:957-969) for the rollout that stands in r's buffers."""
    torch.cuda.synchronize()
    rows = r.prev_obs.reshape(BATCH, *DIMS).cpu().numpy()
    steps = np.arange(BATCH) + (r.step - BATCH)
    aux = Buffer.create_aux_buffer((BATCH,), reward=r.ext_rewards.cpu().numpy().reshape(-1), time=r.all_time[:STEPS].reshape(-1),
                                   action=r.actions.cpu().numpy().reshape(-1), step=steps)
    return rows, aux


def state_of(buf):
    return (buf.current_size, buf.experience_seen, buf.ring_buffer_location, buf.stats_last_entries_added,
            buf.stats_last_entries_submitted)


@pytest.mark.parametrize("mode,thinning", [("uniform", 1.0), ("sequential", 1.0), ("overwrite", 0.5)])
def test_buffer_after_three_iterations_equals_the_numpy_restatement(mode, thinning):
    r = make_runner([f"--replay_mode={mode}", "--replay_size=40", f"--replay_thinning={thinning}", "--replay_mixing=True",
                     "--distil_batch_size=48"])
    buf = r.replay_buffer
    assert buf is not None and buf.max_size == 40 and buf.mode == mode and buf.data.is_cuda and buf.current_size == 0
    assert tuple(buf._data.shape) == (40, *DIMS) and buf._data.dtype == torch.uint8 and args._ignored == []
    want = RN.NumpyReplay(40, DIMS, np.uint8, mode, thinning)
    for i in range(3):
        r.generate_rollout()
        rows, aux = rollout_rows(r)
        assert aux[:, Buffer.AUX_STEP].max() == (i + 1) * BATCH - 1
        np.random.seed(100 + i)
        want.add(rows, aux)
        after = np.random.rand()
        np.random.seed(100 + i)
        r.calculate_returns()
        assert np.random.rand() == after  # the add drew what the reference draws, and nothing else did
        torch.cuda.synchronize()
        assert state_of(buf) == (len(want.data), want.seen, want.ring, want.added, BATCH)
        assert buf.data.cpu().numpy().tobytes() == want.data.tobytes()
        assert buf.aux.cpu().numpy().tobytes() == want.aux.tobytes()
        r.train()
    assert buf.current_size == 40 and r.batch_counter == 3 and torch.isfinite(r.policy_net.flat).all()
    assert len(np.unique(want.data.reshape(40, -1), axis=0)) > 8  # rows that differ: a misplaced row would show


def torch_sample(r, wanted, mixing):
    """The rows get_replay_sample must return, by torch indexing, drawing as rl/rollout.py:2043-2046 draws."""
    buf = r.replay_buffer
    obs = buf.data
    if mixing or buf.current_size == 0:
        obs = torch.cat([obs, r.prev_obs.reshape(BATCH, *r.state_shape)])
    if wanted < len(obs):
        sample = np.random.choice(len(obs), wanted, replace=False)
        obs = obs[torch.from_numpy(sample).cuda()]
    return obs.contiguous()


def forwards(r, obs, chunk=24):
    """Targets from value_net and the old policy from policy_net, chunk by chunk."""
    targets, old = [], []
    for i in range(0, len(obs), chunk):
        targets.append(r.value_net.forward(obs[i:i + chunk], exclude_policy=True)["value"][:, 0].clone())
        old.append(r.policy_net.forward(obs[i:i + chunk], exclude_value=True)["log_policy"].clone())
    return torch.cat(targets), torch.cat(old)


@pytest.mark.parametrize("mixing", [False, True])
def test_distil_batch_rows_targets_and_old_policy(mixing):
    r = make_runner([*REPLAY, f"--replay_mixing={mixing}"])
    for i, (size, rows) in enumerate([(BATCH, 48 if mixing else 32), (64, 48)]):
        r.generate_rollout()
        np.random.seed(30 + i)
        r.calculate_returns()
        assert r.replay_buffer.current_size == size
        np.random.seed(50 + i)
        want_obs = torch_sample(r, 48, mixing)
        after = np.random.rand()
        np.random.seed(50 + i)
        batch = r.get_distil_batch(48)
        assert np.random.rand() == after
        torch.cuda.synchronize()
        assert tuple(batch["prev_state"].shape) == (rows, *DIMS) and batch["prev_state"].is_contiguous()
        assert torch.equal(batch["prev_state"], want_obs)
        want_targets, want_old = forwards(r, want_obs)
        assert tuple(batch["distil_targets"].shape) == (rows,) and tuple(batch["old_policy"].shape) == (rows, N_ACTIONS)
        assert torch.equal(batch["distil_targets"], want_targets) and torch.equal(batch["old_policy"], want_old)
        assert batch["use_tvf"] is False and want_targets.abs().max() > 0
        # the aux records travel with the rows when asked for
        np.random.seed(50 + i)
        obs, aux = r.get_replay_sample(48, with_aux=True)
        torch.cuda.synchronize()
        assert torch.equal(obs, want_obs) and tuple(aux.shape) == (rows, 16)
        if not mixing and size == 64:
            np.random.seed(50 + i)
            sample = np.random.choice(64, 48, replace=False)
            assert torch.equal(aux, r.replay_buffer.aux[torch.from_numpy(sample).cuda()])
        r.train()
    torch.cuda.synchronize()
    assert torch.isfinite(r.policy_net.flat).all()


@pytest.mark.parametrize("encoder", ["nature", "impala"])
def test_train_distil_equals_driving_distil_minibatch_by_hand(encoder):
    """nature: a minibatch's rows are gathered out of the distil batch; impala: the first convolution reads them out of
    it through the index (the distil batch, not the rollout, is then the array the index points into)."""
    a = make_runner([*REPLAY, "--replay_mixing=True"], encoder=encoder)
    b = make_runner([*REPLAY, "--replay_mixing=True"], encoder=encoder)
    for r in (a, b):
        iteration(r, 7)
        r.generate_rollout()
        np.random.seed(8)
        r.calculate_returns()
        r.train_policy()
        r.train_value()
    torch.cuda.synchronize()
    assert torch.equal(a.policy_net.flat, b.policy_net.flat) and torch.equal(a.replay_buffer.data, b.replay_buffer.data)
    assert a.replay_buffer.current_size == 64
    before = a.policy_net.flat.clone()
    np.random.seed(9)
    a.train_distil()
    # b: the same draws, the rows gathered by torch indexing, the minibatches driven here
    np.random.seed(9)
    obs = torch_sample(b, 48, True)
    targets, old = forwards(b, obs)
    net = b.policy_net
    indexed = net.takes_obs_index(obs)
    assert indexed == (encoder == "impala")
    net.zero_untouched_grads()
    opt = rollout.Optimizer(net, args.distil_opt, b.distil_optimizer.state)
    for _epoch in range(2):
        ordering = np.arange(48, dtype=np.int32)
        np.random.shuffle(ordering)
        for j in range(3):
            idx = torch.from_numpy(ordering[16 * j:16 * (j + 1)]).cuda()
            net.distil_minibatch(obs if indexed else obs[idx.long()].contiguous(), targets, old, beta=args.distil.beta,
                                 use_tvf=False, weights=None, gaussian=False, loss_scale=1.0, index=idx, obs_indexed=indexed)
            b.optimizer_step(opt, "distil")
    torch.cuda.synchronize()
    assert not torch.equal(a.policy_net.flat, before)
    assert torch.equal(a.policy_net.flat, b.policy_net.flat)
    assert torch.equal(a.distil_optimizer.state.exp_avg, b.distil_optimizer.state.exp_avg)
    assert a.distil_optimizer.state.step == b.distil_optimizer.state.step == 2 * 2 * 3  # two distil phases of two epochs over 48 rows in minibatches of 16
    stats = a.fetch_stats()
    assert np.isfinite(stats["loss_distil"]) and stats["loss_distil_value"] > 0


def test_checkpoint_resumes_the_buffer_and_the_run(tmp_path):
    flags = [*REPLAY, "--replay_mode=sequential", "--replay_size=40", "--replay_mixing=True"]
    a = make_runner(flags)
    iteration(a, 1)
    iteration(a, 2)
    assert a.replay_buffer.current_size == 40 and a.replay_buffer.ring_buffer_location == 64
    path = a.save_checkpoint(str(tmp_path / "checkpoint-000M-params.pt"), a.step)
    saved = checkpoint.load(path)["replay_buffer"]  # rl/replay.py:65-74
    assert set(saved) == {"max_size", "experience_seen", "ring_buffer_location", "data", "aux", "name", "thinning"}
    assert isinstance(saved["data"], np.ndarray) and saved["data"].shape == (40, *DIMS) and saved["data"].dtype == np.uint8
    assert saved["data"].tobytes() == a.replay_buffer.data.cpu().numpy().tobytes()
    assert saved["aux"].dtype == np.float32 and saved["aux"].tobytes() == a.replay_buffer.aux.cpu().numpy().tobytes()
    assert (saved["max_size"], saved["experience_seen"], saved["ring_buffer_location"]) == (40, 64, 64)
    b = make_runner(flags, seed=6)
    assert b.replay_buffer.current_size == 0
    assert b.load_checkpoint(path) == 2 * BATCH
    assert state_of(b.replay_buffer)[:3] == (40, 64, 64)
    assert torch.equal(b.replay_buffer.data, a.replay_buffer.data) and torch.equal(b.replay_buffer.aux, a.replay_buffer.aux)
    iteration(a, 3)
    iteration(b, 3)
    assert torch.equal(a.all_obs, b.all_obs)
    assert torch.equal(b.replay_buffer.data, a.replay_buffer.data) and torch.equal(b.replay_buffer.aux, a.replay_buffer.aux)
    assert state_of(a.replay_buffer) == state_of(b.replay_buffer) == (40, 96, 96, 32, 32)
    assert torch.equal(a.policy_net.flat, b.policy_net.flat) and torch.equal(a.value_net.flat, b.value_net.flat)
    # disable_replay leaves the entry out; another --replay_size is refused on load
    bare = checkpoint.load(a.save_checkpoint(str(tmp_path / "bare.pt"), a.step, disable_replay=True))
    assert "replay_buffer" not in bare
    c = make_runner([*REPLAY, "--replay_mode=sequential", "--replay_size=48"])
    with pytest.raises(ValueError, match="--replay_size"):
        c.load_checkpoint(path)
    off = make_runner()
    assert "replay_buffer" not in checkpoint.load(off.save_checkpoint(str(tmp_path / "off.pt"), 0))


def test_replay_off_changes_nothing():
    plain = make_runner()
    assert args._ignored == [] and plain.replay_buffer is None
    ignored = make_runner(["--replay_size=64"])
    assert args._ignored == ["--replay_size=64"] and ignored.replay_buffer is None and not args.replay.enabled
    for r in (plain, ignored):
        iteration(r, 21)
        iteration(r, 22)
    assert torch.equal(plain.all_obs, ignored.all_obs)
    assert plain.policy_net.flat.cpu().numpy().tobytes() == ignored.policy_net.flat.cpu().numpy().tobytes()
    assert plain.value_net.flat.cpu().numpy().tobytes() == ignored.value_net.flat.cpu().numpy().tobytes()
    # and without a buffer a distil batch other than the rollout is still refused
    with pytest.raises(NotImplementedError, match="distil_batch_size"):
        plain.get_distil_batch(16)


def test_what_the_replay_path_refuses(monkeypatch):
    r = make_runner([*REPLAY, "--distil_batch_size=24"])
    r.generate_rollout()
    r.calculate_returns()
    with pytest.raises(ValueError, match="multiple"):  # 24 rows in minibatches of 16, as the other phases
        r.train_distil()
    r = make_runner([*REPLAY, "--distil_target=return"])
    r.generate_rollout()
    r.calculate_returns()
    with pytest.raises(AssertionError, match="value targets"):  # rl/rollout.py:2115
        r.get_distil_batch(16)
    monkeypatch.setattr(rollout.parallel, "world_size", lambda: 2)
    with pytest.raises(NotImplementedError, match="data parallelism"):
        make_runner(REPLAY)


def test_replay_stats_are_logged_every_fourth_batch():
    r = make_runner([*REPLAY, "--disable_logging=False", "--disable_ev=True"])
    r.generate_rollout()
    r.calculate_returns()  # batch 0
    assert r.log["replay_size"] == BATCH and r.log["replay_last_entries_added"] == BATCH and 0 <= r.log["rp_ks"] <= 1
    assert r.log["replay_diversity"] > 0 and r.log["replay_density"] == r.log["replay_diversity_k1"] > 0
    r.train()
    r.generate_rollout()
    r.calculate_returns()  # batch 1: not logged
    assert r.log["replay_size"] == BATCH and r.replay_buffer.current_size == 64


def test_train_main_with_a_replay_buffer(monkeypatch, tmp_path):
    import sys
    import train
    batch = 32 * 16
    monkeypatch.setattr(sys, "argv", [
        "train.py", "--agents=32", "--n_steps=16", "--model_architecture=dual", "--model_encoder=nature",
        "--env_type=synthetic", "--env_embed_time=False", "--seed=4", "--policy_opt_mini_batch_size=128",
        "--policy_opt_epochs=1", "--value_opt_mini_batch_size=128", "--distil_opt_mini_batch_size=128", "--env_warmup_period=5",
        "--experiment_name=exp", "--run_name=replay_test", f"--output_folder={tmp_path}", f"--epochs={(2 * batch - 1) / 1e6}",
        "--replay_mode=uniform", "--replay_size=256", "--distil_batch_size=256", "--replay_mixing=True"])
    r = train.main()
    buf = r.replay_buffer
    assert r.step == 2 * batch and args._ignored == [] and buf is not None and buf.mode == "uniform"
    assert (buf.current_size, buf.experience_seen, buf.stats_last_entries_submitted) == (256, 2 * batch, batch)
    assert buf.stats_last_entries_added == 128  # ceil(512 / 1024 * 256)
    assert r.distil_optimizer.state.step == 2 * 2 * 2  # two iterations, two epochs, 256 rows in minibatches of 128
    assert "replay_size" in open(__import__("os").path.join(args.log_folder, "training_log.csv")).readline()
    assert torch.isfinite(r.policy_net.flat).all() and torch.isfinite(r.value_net.flat).all()
