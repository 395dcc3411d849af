"""GPU: a Runner on the synthetic env with 4 x 84 x 84 observations and the IMPALA encoder under
--model_encoder_args="{'down_sample': 'stride'}" - the stack-first convolutions on the generic stride-2 kernels, no
max-pool, the minibatches through the gathered path, the flag read by args.setup and handed to TVFModel as train.py does -
trains: finite losses, every convolution parameter moves, the run is reproducible bit for bit from its seed, and a
checkpoint restores into a run that continues bit-identically (the pattern of tests/test_impala_any_train_gpu.py)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FLAGS = ["--agents=8", "--n_steps=8", "--model_architecture=single", "--model_encoder=impala",
         "--model_encoder_args={'down_sample': 'stride'}", "--env_type=synthetic", "--env_synthetic_shape=4,84,84",
         "--env_embed_time=False", "--seed=4", "--policy_opt_mini_batch_size=32", "--policy_opt_epochs=1",
         "--env_warmup_period=5", "--experiment_name=exp", "--run_name=impala_stride"]
BATCH = 8 * 8


def make_runner(seed, tmp):
    from ppo_amd import envs, logger, models, rollout
    from ppo_amd.config import args
    args.setup([*FLAGS, f"--output_folder={tmp}"])
    assert args.model.encoder_args == "{'down_sample': 'stride'}"
    torch.manual_seed(seed)
    shape, nA = envs.get_env_spec()
    assert tuple(shape) == (4, 84, 84)
    model = models.TVFModel(args.model.encoder, encoder_args=args.model.encoder_args, input_dims=shape, actions=nA,
                            device="cuda", architecture="single", hidden_units=64, head_scale=0.1, head_bias=True)
    r = rollout.Runner(model, logger.Logger(quiet=True))
    r.vec_env = envs.create_envs_classic()
    r.reset()
    return r


def iteration(r):
    r.generate_rollout()
    r.calculate_returns()
    r.train()


def test_runner_trains_reproducibly_and_resumes_bit_identically(tmp_path):
    np.random.seed(9)
    a = make_runner(1, str(tmp_path))
    net = a.net
    assert net.spec.down_sample == "stride" and net.spec.out_shape == (32, 11, 11)
    assert net.generic_convs == [f"encoder.stacks.{si}.firstconv" for si in range(3)] and not net.takes_obs_index(a.all_obs)
    start = net.flat.clone()
    iteration(a)
    path = a.save_checkpoint(str(tmp_path / "checkpoint-000M-params.pt"), a.step)
    assert os.path.exists(path)
    iteration(a)
    torch.cuda.synchronize()
    assert a.step == 2 * BATCH and net._adam_step == 2 * (BATCH // 32)
    assert torch.isfinite(net.flat).all() and torch.isfinite(net.grad).all()
    stat_rows = [t for (bname, _shape, _dt), t in net._bufs.items() if bname.startswith("stat_rows_")]
    assert stat_rows and all(torch.isfinite(t).all() for t in stat_rows), "a minibatch's loss statistics are not finite"
    assert not any(bname.startswith("tidx") for (bname, _shape, _dt) in net._bufs), "an argmax buffer without a max-pool"
    for name, (o, shape) in net._offsets.items():
        if name.startswith("encoder.stacks."):
            n = int(np.prod(shape))
            assert not torch.equal(net.flat[o:o + n], start[o:o + n]), f"{name} did not move"

    # the same seeds again: the same bits
    np.random.seed(9)
    b = make_runner(1, str(tmp_path))
    assert torch.equal(b.net.flat, start)
    for _ in range(2):
        iteration(b)
    torch.cuda.synchronize()
    assert torch.equal(a.net.flat, b.net.flat), "two runs from one seed differ"
    assert torch.equal(a.net.exp_avg, b.net.exp_avg) and torch.equal(a.net.exp_avg_sq, b.net.exp_avg_sq)

    # other seeds, then the checkpoint taken after iteration 1: continues to the same bits
    np.random.seed(12345)
    c = make_runner(2, str(tmp_path))
    assert not torch.equal(c.net.flat, start)
    assert c.load_checkpoint(str(tmp_path / "checkpoint-000M-params.pt")) == BATCH
    iteration(c)
    torch.cuda.synchronize()
    assert torch.equal(a.all_obs, c.all_obs) and torch.equal(a.actions, c.actions)
    assert torch.equal(a.net.flat, c.net.flat), "parameters diverged after resume"
    assert torch.equal(a.net.exp_avg, c.net.exp_avg) and torch.equal(a.net.exp_avg_sq, c.net.exp_avg_sq)
    assert a.step == c.step and a.net._adam_step == c.net._adam_step
