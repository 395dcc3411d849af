"""GPU: the Runner with a batch-norm IMPALA model (--model_encoder_args="{'batch_norm': True}"), built from flags on the
synthetic env.  The rollout runs in train mode (rl/rollout.py:712): every one of its N + 1 forwards - all A envs at once, or
chunks of --max_micro_batch_size in row order - normalises with its own batch's statistics and updates the running ones;
everything behind it (returns, minibatch updates) runs in eval mode on the running statistics, which it leaves alone.

The buffers after a rollout are compared with a float64 replay (tests/impala_batchnorm_torch.py) of rows 0..N of all_obs
from the initial state, at the forward bar of tests/test_impala_batchnorm_gpu.py - 1e-4 of each tensor's maximum: the maps
that feed the statistics carry float32 convolution error - and the counter exactly."""
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import impala_batchnorm_torch as BN  # noqa: E402

COMMON = ["--n_steps=4", "--model_encoder=impala", "--model_encoder_args={'batch_norm': True}", "--model_hidden_units=64",
          "--env_type=synthetic", "--env_embed_time=False", "--env_synthetic_shape=4,20,20", "--seed=4",
          "--policy_opt_mini_batch_size=16", "--policy_opt_epochs=1", "--value_opt_mini_batch_size=16", "--value_opt_epochs=1",
          "--distil_opt_mini_batch_size=16", "--distil_opt_epochs=1", "--disable_logging=True"]
CASES = {
    "single_8": ["--agents=8", "--model_architecture=single"],
    "single_16_chunks_of_8": ["--agents=16", "--model_architecture=single", "--max_micro_batch_size=8"],
    "dual_8": ["--agents=8", "--model_architecture=dual"],
}


@pytest.fixture(autouse=True)
def restore_micro_batch_size():
    """--max_micro_batch_size is a top-level flag: a later args.setup() without it would keep the value."""
    from ppo_amd.config import args
    before = args.max_micro_batch_size
    yield
    args.max_micro_batch_size = before


def make_runner(flags, seed=1, tmp=None):
    from ppo_amd import envs, logger, models, rollout
    from ppo_amd.config import args
    args.setup([*COMMON, *flags, *([f"--output_folder={tmp}"] if tmp else [])])
    torch.manual_seed(seed)
    np.random.seed(seed)
    shape, nA = envs.get_env_spec()
    model = models.TVFModel("impala", encoder_args=args.model.encoder_args, input_dims=shape, actions=nA, device="cuda",
                            architecture=args.model.architecture, hidden_units=args.model.hidden_units, head_scale=0.1,
                            head_bias=True)
    assert model.batch_norm and model.policy_net.training
    r = rollout.Runner(model, logger.Logger(quiet=True))
    r.vec_env = envs.create_envs_classic()
    r.reset()
    return r


def double_sd(net):
    return {k: (v.detach().cpu().double() if v.is_floating_point() else v.detach().cpu().clone()) for k, v in net.state_dict().items()}


def rel_err(got, ref):
    got, ref = torch.as_tensor(got).detach().cpu().double(), torch.as_tensor(ref).detach().cpu().double()
    return (got - ref.reshape(got.shape)).abs().max().item() / max(ref.abs().max().item(), 1e-30)


def nets_of(r):
    return [r.policy_net] + ([r.value_net] if r.dual else [])


@pytest.mark.parametrize("name", list(CASES))
def test_rollout_updates_the_buffers_as_a_float64_replay_does(name):
    from ppo_amd.config import args
    r = make_runner(CASES[name])
    N, A = r.N, r.A
    micro = min(int(args.max_micro_batch_size), A)
    chunks = -(-A // micro)
    start = [double_sd(n) for n in nets_of(r)]
    r.generate_rollout()
    torch.cuda.synchronize()
    assert all(not n.training for n in nets_of(r)), "generate_rollout leaves the model in eval mode (rl/rollout.py:927)"
    obs = r.all_obs.cpu().double() / 255.0
    for net, sd in zip(nets_of(r), start):
        geom = dict(n_stacks=len(net.spec.channels), n_block=net.spec.n_block, down_sample=net.spec.down_sample)
        for t in range(N + 1):
            for lo in range(0, A, micro):
                with torch.no_grad():
                    out, new = BN.forward_train(sd, obs[t, lo:lo + micro], **geom)
                sd.update(new)
                if net is r.value_net:
                    e = rel_err(r.value[t, lo:lo + micro], out["value"])
                    assert e < 1e-4, (name, t, lo, "value", e)
                if net is r.policy_net and t < N:
                    e = rel_err(r.log_policy[t, lo:lo + micro], out["log_policy"])
                    assert e < 1e-4, (name, t, lo, "log_policy", e)
        for bname, t_ in net.buffers.items():
            if bname.endswith("num_batches_tracked"):
                assert int(t_) == (N + 1) * chunks == int(sd[bname]), bname
            else:
                e = rel_err(t_, sd[bname])
                print(f"IMPALA_BN rollout {name} {bname} rel_err={e:.3e}")
                assert e < 1e-4, (name, bname, e)
    # everything behind the rollout runs on the running statistics and leaves them alone; gamma and beta train
    kept = [{k: v.clone() for k, v in n.buffers.items()} for n in nets_of(r)]
    affine = [{k: v.clone() for k, v in n.params.items() if ".bn" in k} for n in nets_of(r)]
    r.calculate_returns()
    r.train()
    torch.cuda.synchronize()
    for net, b0, p0 in zip(nets_of(r), kept, affine):
        assert not net.training
        assert all(torch.equal(b0[k], v) for k, v in net.buffers.items()), "train() changed a batch-norm buffer"
        assert all(not torch.equal(p0[k], net.params[k]) for k in p0), "a gamma or beta did not move"
        assert torch.isfinite(net.flat).all()


def iteration(r):
    r.generate_rollout()
    r.calculate_returns()
    r.train()


def same_state(a, b):
    for na, nb in zip(nets_of(a), nets_of(b)):
        assert torch.equal(na.flat, nb.flat)
        for k in na.buffers:
            assert torch.equal(na.buffers[k], nb.buffers[k]), k
    assert torch.equal(a.all_obs, b.all_obs) and torch.equal(a.actions, b.actions) and torch.equal(a.value, b.value)
    assert torch.equal(a.log_policy, b.log_policy)


def test_two_runs_from_one_seed_are_bit_identical():
    runs = []
    for _ in range(2):
        r = make_runner(CASES["single_16_chunks_of_8"], seed=3)
        for _it in range(2):  # the second rollout replays the recorded train-mode plans
            iteration(r)
        torch.cuda.synchronize()
        runs.append(r)
    same_state(*runs)


def test_checkpoint_holds_the_buffers_and_resumes_bit_identically(tmp_path):
    from ppo_amd import checkpoint
    a = make_runner(CASES["single_8"], seed=1, tmp=str(tmp_path))
    iteration(a)
    path = a.save_checkpoint(str(tmp_path / "checkpoint-000M-params.pt"), a.step)
    keys = list(checkpoint.load(path)["model_state_dict"])
    base = "policy_net.encoder.stacks.0.blocks.0.bn0."
    i = keys.index(base + "weight")
    assert keys[i:i + 5] == [base + k for k in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")]
    iteration(a)
    torch.cuda.synchronize()
    b = make_runner(CASES["single_8"], seed=2, tmp=str(tmp_path))
    assert not torch.equal(a.policy_net.flat, b.policy_net.flat)
    b.load_checkpoint(path)
    assert int(b.policy_net.buffers[base[len("policy_net."):] + "num_batches_tracked"]) == a.N + 1
    iteration(b)
    torch.cuda.synchronize()
    same_state(a, b)


def test_train_py_launch_line_completes(monkeypatch, tmp_path):
    import train
    batch = 8 * 4
    monkeypatch.setattr(sys, "argv", ["train.py", *[f for f in COMMON if f != "--disable_logging=True"], *CASES["single_8"],
                                      f"--output_folder={tmp_path}", "--env_warmup_period=5", "--experiment_name=exp",
                                      "--run_name=bn", f"--epochs={(3 * batch - 1) / 1e6}"])
    r = train.main()
    assert r.step == 3 * batch and r.model.batch_norm and torch.isfinite(r.policy_net.flat).all()
    nbt = next(v for k, v in r.policy_net.buffers.items() if k.endswith("num_batches_tracked"))
    assert int(nbt) == 3 * (r.N + 1)  # the warm-up draws random actions and runs no forward: 3 rollouts, nothing else


def test_data_parallelism_is_refused(monkeypatch):
    from ppo_amd import envs, logger, models, rollout
    from ppo_amd.config import args
    args.setup([*COMMON, *CASES["single_8"]])
    shape, nA = envs.get_env_spec()
    model = models.TVFModel("impala", encoder_args=args.model.encoder_args, input_dims=shape, actions=nA, device="cuda",
                            architecture="single", hidden_units=64, head_scale=0.1, head_bias=True)
    monkeypatch.setattr(rollout.parallel, "world_size", lambda: 2)
    with pytest.raises(NotImplementedError, match="data parallelism"):
        rollout.Runner(model, logger.Logger(quiet=True))
