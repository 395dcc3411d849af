"""GPU: the Nature-CNN encoder end to end (DualHeadNet / TVFModel / Runner / train.py with encoder="nature").

Against tests/golden/nature_golden.npz (the reference's TVFModel(encoder="nature") on CPU, make_nature_golden.py):
forward head outputs within 1e-4 of the tensor's max at (4, 36, 36) / hidden 64 and at (4, 84, 84) / hidden 512; at the
small geometry the loss of one policy minibatch within 1e-4 and every parameter gradient within the bars
tests/test_model_gpu.py holds IMPALA's to (1e-4 of the tensor's max for the convolutions, 1e-5 for the linear layer and
the heads).  The fixture's seed leaves every ReLU pre-activation at least 1e-5 from zero, so nothing is excluded.
At full size the same gradient bars against a float64 network written here with torch.nn.functional.conv2d."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
import torch.nn.functional as F  # noqa: E402

from ppo_amd import models  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "nature_golden.npz")), json.load(open(os.path.join(golden_dir, "nature_golden.json")))


def rel_err(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-30)


def make_net(meta, tag):
    torch.manual_seed(meta[tag]["seed"])
    return models.DualHeadNet("nature", tuple(meta[tag]["input_dims"]), meta["n_actions"], hidden_units=meta[tag]["hidden_units"],
                              head_scale=meta["head_scale"], head_bias=meta["head_bias"], device="cuda")


def bar(name):
    return 1e-4 if name.startswith("encoder.conv") else 1e-5


@pytest.mark.parametrize("tag", ["small", "full"])
def test_forward_matches_reference(gold, tag):
    g, meta = gold
    net = make_net(meta, tag)
    assert list(net.state_dict().keys()) == meta[tag]["param_names"]
    assert net.n_parameters() == sum(int(np.prod(v["shape"])) for v in meta[tag]["params"].values())
    assert not net.takes_obs_index(torch.zeros((1, *meta[tag]["input_dims"]), dtype=torch.uint8, device="cuda"))
    x = torch.from_numpy(g[f"{tag}_fwd_x"]).cuda()
    for _ in range(2):  # the second forward replays the recorded launch plan
        out = net.forward(x, policy_temperature=1.0)
        torch.cuda.synchronize()
        for k in ("raw_policy", "log_policy", "value", "advantage"):
            assert rel_err(out[k].cpu().numpy(), g[f"{tag}_fwd_{k}"]) < 1e-4, k


def test_policy_minibatch_matches_reference_runner(gold):
    g, meta = gold
    assert meta["small"]["relu_margin"] >= 1e-5
    net = make_net(meta, "small")
    d = {k: g[f"small_mb_{k}"] for k in ("prev_state", "actions", "log_policy", "log_pac", "advantages", "returns")}
    stats = net.ppo_minibatch(
        torch.from_numpy(d["prev_state"]).cuda(), torch.from_numpy(d["actions"].astype(np.int32)).cuda(),
        torch.from_numpy(d["log_pac"]).cuda(), torch.from_numpy(d["log_policy"]).cuda(),
        torch.from_numpy(d["advantages"]).cuda(), torch.from_numpy(d["returns"]).cuda(),
        eps_clip=meta["ppo_epsilon"], ent_coef=meta["entropy_bonus"], vf_coef=meta["ppo_vf_coef"], loss_scale=1.0)
    torch.cuda.synchronize()
    s = stats.cpu().numpy().astype(np.float64)
    loss, kl_approx, kl_true, clip_frac = g["small_mb_result"]
    assert abs(-s[:, 6].mean() - loss) < 1e-4 * max(1.0, abs(loss))
    assert abs(s[:, 4].mean() - kl_approx) < 1e-5 + 1e-4 * abs(kl_approx)
    assert abs(s[:, 5].mean() - kl_true) < 1e-5 + 1e-4 * abs(kl_true)
    assert abs(s[:, 3].mean() - clip_frac) < 1e-9
    worst = {}
    for name in meta["small"]["param_names"]:
        if name in meta["small"]["grad_none"]:
            assert float(net.grads[name].abs().max()) == 0.0, name
            continue
        worst[name] = rel_err(net.grads[name].cpu().numpy(), g["small_grad_" + name])
        print(f"NATURE_GRAD small {name} rel_err={worst[name]:.3e} bar={bar(name):.0e}")
    for name, e in worst.items():
        assert e < bar(name), (name, e)


def float64_network(sd, x, n_actions):
    """NatureCNN + heads (rl/models.py:130-145, 467-506) in float64: fused head row [policy | value | advantage]."""
    h = x
    for name, stride in (("conv1", 4), ("conv2", 2), ("conv3", 1)):
        h = F.relu(F.conv2d(h, sd[f"encoder.{name}.weight"], sd[f"encoder.{name}.bias"], stride=stride))
    feat = F.relu(F.linear(h.reshape(h.shape[0], -1), sd["encoder.fc.weight"], sd["encoder.fc.bias"]))
    heads = [F.linear(feat, sd[f"{n}.weight"], sd.get(f"{n}.bias")) for n in ("policy_head", "value_head", "advantage_head")]
    return torch.cat(heads, dim=1)


def test_full_size_gradients_match_float64():
    """(4, 84, 84), hidden 512, minibatch 8: PPO loss gradients of all eight encoder tensors and the heads against
    float64 autograd of the same function (loss: rl/rollout.py:1640-1660, 1744-1753, as oracle/model_torch.ppo_loss)."""
    from oracle import model_torch as R
    B, nA = 8, 6
    torch.manual_seed(3)
    net = models.DualHeadNet("nature", (4, 84, 84), nA, hidden_units=512, head_scale=0.1, head_bias=True, device="cuda")
    rng = np.random.default_rng(5)
    x = torch.from_numpy(rng.integers(0, 256, size=(B, 4, 84, 84), dtype=np.uint8)).cuda()
    actions = torch.from_numpy(rng.integers(0, nA, size=(B,)).astype(np.int64)).cuda()
    old_lp = torch.log_softmax(torch.from_numpy(rng.normal(size=(B, nA)).astype(np.float32)), dim=1).cuda()
    old_log_pac = old_lp[torch.arange(B), actions].contiguous()
    adv = torch.from_numpy(rng.normal(size=(B,)).astype(np.float32)).cuda()
    ret = torch.from_numpy(rng.normal(size=(B, 1)).astype(np.float32)).cuda()
    net.ppo_minibatch(x, actions.int(), old_log_pac, old_lp, adv, ret, eps_clip=0.2, ent_coef=0.01, vf_coef=0.5, loss_scale=1.0)
    torch.cuda.synchronize()
    sd = {k: v.detach().double().requires_grad_(True) for k, v in net.params.items()}
    o = float64_network(sd, x.double() / 255.0, nA)
    # no ReLU decision of this sample may be a near-tie, or float32 and float64 could differ by a whole branch
    out = {"raw_policy": o[:, :nA], "log_policy": torch.log_softmax(o[:, :nA], dim=1), "value": o[:, nA:nA + 1]}
    loss = R.ppo_loss(out, actions, old_log_pac.double(), adv.double(), ret.double())
    loss.backward()
    assert rel_err(net.heads(net.encode(x, train=True), "t").cpu().numpy(), o.detach().cpu().numpy()) < 1e-4
    for name, p in sd.items():
        if p.grad is None:
            assert float(net.grads[name].abs().max()) == 0.0, name
            continue
        e = rel_err(net.grads[name].cpu().numpy(), p.grad.cpu().numpy())
        print(f"NATURE_GRAD full {name} rel_err={e:.3e} bar={bar(name):.0e}")
        assert e < bar(name), (name, e)


FLAGS = ["--agents=8", "--n_steps=16", "--model_encoder=nature", "--env_type=synthetic", "--env_embed_time=False", "--seed=4",
         "--policy_opt_mini_batch_size=64", "--policy_opt_epochs=1", "--value_opt_mini_batch_size=64", "--value_opt_epochs=1", "--distil_opt_mini_batch_size=64",
         "--env_warmup_period=5"]


def make_runner(seed, tmp, architecture):
    from ppo_amd import envs, logger, rollout
    from ppo_amd.config import args
    args.setup([*FLAGS, f"--model_architecture={architecture}", f"--output_folder={tmp}"])
    torch.manual_seed(seed)
    shape, nA = envs.get_env_spec()
    model = models.TVFModel("nature", encoder_args={"base_channels": 32}, input_dims=shape, actions=nA, device="cuda",
                            architecture=architecture, hidden_units=512, head_scale=0.1, head_bias=True)
    r = rollout.Runner(model, logger.Logger(quiet=True))
    r.vec_env = envs.create_envs_classic()
    r.reset()
    return r


def iteration(r):
    r.generate_rollout()
    r.calculate_returns()
    r.train()


@pytest.mark.parametrize("architecture", ["single", "dual"])
def test_runner_trains_and_resumes_bit_identically(tmp_path, architecture):
    np.random.seed(9)
    a = make_runner(1, str(tmp_path), architecture)
    assert a.all_obs.dtype == torch.uint8
    nets = [a.policy_net] if architecture == "single" else [a.policy_net, a.value_net]
    before = [n.flat.clone() for n in nets]
    for _ in range(2):
        iteration(a)
    torch.cuda.synchronize()
    for n, b0 in zip(nets, before):
        assert torch.isfinite(n.flat).all() and torch.isfinite(n.grad).all() and not torch.equal(n.flat, b0)
    assert torch.isfinite(a.advantage).all() and torch.isfinite(a.value).all()
    path = a.save_checkpoint(str(tmp_path / "checkpoint-000M-params.pt"), a.step)
    iteration(a)
    torch.cuda.synchronize()
    np.random.seed(12345)
    b = make_runner(2, str(tmp_path), architecture)
    assert b.load_checkpoint(str(tmp_path / "checkpoint-000M-params.pt")) == 2 * 8 * 16 and os.path.exists(path)
    iteration(b)
    torch.cuda.synchronize()
    assert torch.equal(a.all_obs, b.all_obs) and torch.equal(a.actions, b.actions)
    for na, nb in zip(nets, [b.policy_net] if architecture == "single" else [b.policy_net, b.value_net]):
        assert torch.equal(na.flat, nb.flat) and torch.equal(na.exp_avg, nb.exp_avg) and torch.equal(na.exp_avg_sq, nb.exp_avg_sq)


def test_train_py_runs_with_the_default_encoder(tmp_path):
    """`python train.py` with no --model_encoder: the default (nature, as the reference's) now has a HIP path."""
    from ppo_amd.config import args
    args.setup(["--env_type=synthetic"])
    assert args.model.encoder == "nature"
    cmd = [sys.executable, os.path.join(ROOT, "train.py"), "--env_type=synthetic", "--device=cuda:0", "--agents=8", "--n_steps=16",
           f"--epochs={(2 * 8 * 16 - 1) / 1e6}", "--policy_opt_mini_batch_size=64", "--value_opt_mini_batch_size=64",
           "--distil_opt_mini_batch_size=64", "--env_warmup_period=5", f"--output_folder={tmp_path}", "--restore=never"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
