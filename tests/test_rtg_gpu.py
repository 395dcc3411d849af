"""GPU: the RTG encoder end to end (DualHeadNet / TVFModel / Runner / train.py with encoder="rtg").

Against tests/golden/rtg_golden.npz (the reference's TVFModel(encoder="rtg") on CPU, make_rtg_golden.py): forward head
outputs within 1e-4 of the tensor's max at (4, 36, 46) / hidden 64 - an odd height at the first pool, odd widths at the
second and third - and at (4, 84, 84) / hidden 512; at the small geometry the loss of one policy minibatch within 1e-4 and
every parameter gradient within the bars tests/test_nature_gpu.py holds the nature encoder's to (1e-4 of the tensor's max
for the convolutions, 1e-5 for the linear layer and the heads).  This network has two kinds of kink - ReLU zeros and pool
ties; the fixture's seeds leave every pooled value and encoder output at least 1e-5 from zero and every open window's
maximum at least 1e-5 above its runner-up, so nothing is excluded.  At full size the same gradient bars against a float64
network written here with torch.nn.functional, at the minibatch of 2 the fixture found such a seed for."""
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
    return np.load(os.path.join(golden_dir, "rtg_golden.npz")), json.load(open(os.path.join(golden_dir, "rtg_golden.json")))


def rel_err(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-30)


def make_net(meta, tag, **kw):
    torch.manual_seed(meta[tag]["seed"])
    return models.DualHeadNet("rtg", tuple(meta[tag]["input_dims"]), meta["n_actions"], hidden_units=meta[tag]["hidden_units"],
                              head_scale=meta["head_scale"], head_bias=meta["head_bias"], device="cuda", **kw)


def bar(name):
    return 1e-4 if name.startswith("encoder.conv") else 1e-5


@pytest.mark.parametrize("tag", ["small", "full"])
def test_forward_matches_reference(gold, tag):
    g, meta = gold
    net = make_net(meta, tag, base_channels=48)  # **ignore_args (rl/models.py:177): accepted and ignored
    assert list(net.state_dict().keys()) == meta[tag]["param_names"]
    assert net.n_parameters() == sum(int(np.prod(v["shape"])) for v in meta[tag]["params"].values())
    assert not net.takes_obs_index(torch.zeros((1, *meta[tag]["input_dims"]), dtype=torch.uint8, device="cuda"))
    assert net.early_grad_offset == 0 and net.generic_convs == [] and not net.split_bf16
    x = torch.from_numpy(g[f"{tag}_fwd_x"]).cuda()
    for _ in range(2):  # the second forward replays the recorded launch plan
        out = net.forward(x, policy_temperature=1.0)
        torch.cuda.synchronize()
        for k in ("raw_policy", "log_policy", "value", "advantage"):
            assert rel_err(out[k].cpu().numpy(), g[f"{tag}_fwd_{k}"]) < 1e-4, k
    (calls, *_rest), = net._plans.values()
    assert [n for _f, n, _a in calls] == [
        "ppo_conv2d_strided_forward_f32", "ppo_maxpool2x2_relu_forward_f32", "ppo_conv3x3_any_forward_f32",
        "ppo_maxpool2x2_relu_forward_f32", "ppo_conv3x3_any_forward_f32", "ppo_maxpool2x2_relu_forward_f32",
        "ppo_dense_heads_forward_f32"]


def test_policy_minibatch_matches_reference_runner(gold):
    g, meta = gold
    assert meta["small"]["kink_margin"] >= 1e-5
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
        print(f"RTG_GRAD small {name} rel_err={worst[name]:.3e} bar={bar(name):.0e}")
    for name, e in worst.items():
        assert e < bar(name), (name, e)


def pool_margin(y):
    """Of one pre-pool map [B, C, H, W]: min(|pooled value|, maximum - runner-up over the windows pooled > 0)."""
    b, c, h, w = y.shape
    ho, wo = h // 2, w // 2
    win = y[:, :, :2 * ho, :2 * wo].reshape(b, c, ho, 2, wo, 2).permute(0, 1, 2, 4, 3, 5).reshape(b, c, ho, wo, 4)
    top = win.sort(dim=-1, descending=True).values
    pooled, gap = top[..., 0], top[..., 0] - top[..., 1]
    return min(float(pooled.abs().min()), float(gap[pooled > 0].min()))


def float64_network(sd, x, margins=None):
    """RTG_LSTM + heads (rl/models.py:198-213, 467-506) in float64: fused head row [policy | value | advantage].
    `margins`: a list that receives the kink margin of every pre-pool map and of the encoder output."""
    h = x
    for name, stride, padding in (("conv1", 2, 0), ("conv2", 1, 1), ("conv3", 1, 1)):
        y = F.conv2d(h, sd[f"encoder.{name}.weight"], sd[f"encoder.{name}.bias"], stride=stride, padding=padding)
        if margins is not None:
            margins.append(pool_margin(y.detach()))
        h = F.relu(F.max_pool2d(y, 2, 2))
    z = F.linear(h.reshape(h.shape[0], -1), sd["encoder.fc.weight"], sd["encoder.fc.bias"])
    if margins is not None:
        margins.append(float(z.detach().abs().min()))
    feat = F.relu(z)
    heads = [F.linear(feat, sd[f"{n}.weight"], sd.get(f"{n}.bias")) for n in ("policy_head", "value_head", "advantage_head")]
    return torch.cat(heads, dim=1)


def test_full_size_gradients_match_float64(gold):
    """(4, 84, 84), hidden 512, minibatch 2 from the fixture's `full_b2` seed: PPO loss gradients of all eight encoder
    tensors and the heads against float64 autograd of the same function (loss: rl/rollout.py:1640-1660, 1744-1753, as
    oracle/model_torch.ppo_loss).  The kink margin is recomputed in float64 first and must be at least 5e-6, half the
    generator's 1e-5 (float32 against float64 forward): a changed initialisation fails here, loudly, not through a
    flipped window."""
    from oracle import model_torch as R
    _g, meta = gold
    m2 = meta["full_b2"]
    assert m2["kink_margin"] >= 1e-5
    B, nA, seed = m2["minibatch"], meta["n_actions"], m2["seed"]
    torch.manual_seed(seed)
    net = models.DualHeadNet("rtg", tuple(m2["input_dims"]), nA, hidden_units=m2["hidden_units"], head_scale=meta["head_scale"],
                             head_bias=meta["head_bias"], device="cuda")
    rng = np.random.default_rng(seed)
    x = torch.from_numpy(rng.integers(0, 256, size=(B, *m2["input_dims"]), dtype=np.uint8)).cuda()  # the first draw
    actions = torch.from_numpy(rng.integers(0, nA, size=(B,)).astype(np.int64)).cuda()
    old_lp = torch.log_softmax(torch.from_numpy(rng.normal(size=(B, nA)).astype(np.float32)), dim=1).cuda()
    old_log_pac = old_lp[torch.arange(B), actions].contiguous()
    adv = torch.from_numpy(rng.normal(size=(B,)).astype(np.float32)).cuda()
    ret = torch.from_numpy(rng.normal(size=(B, 1)).astype(np.float32)).cuda()
    net.ppo_minibatch(x, actions.int(), old_log_pac, old_lp, adv, ret, eps_clip=0.2, ent_coef=0.01, vf_coef=0.5, loss_scale=1.0)
    torch.cuda.synchronize()
    sd = {k: v.detach().double().requires_grad_(True) for k, v in net.params.items()}
    margins = []
    o = float64_network(sd, x.double() / 255.0, margins)
    print(f"RTG_MARGIN full_b2 float64 {min(margins):.3e} (fixture, float32: {m2['kink_margin']:.3e})")
    assert len(margins) == 4 and min(margins) >= 5e-6, margins
    out = {"raw_policy": o[:, :nA], "log_policy": torch.log_softmax(o[:, :nA], dim=1), "value": o[:, nA:nA + 1]}
    loss = R.ppo_loss(out, actions, old_log_pac.double(), adv.double(), ret.double())
    loss.backward()
    assert rel_err(net.heads(net.encode(x, train=True), "t").cpu().numpy(), o.detach().cpu().numpy()) < 1e-4
    worst = {}
    for name, p in sd.items():
        if p.grad is None:
            assert float(net.grads[name].abs().max()) == 0.0, name
            continue
        worst[name] = rel_err(net.grads[name].cpu().numpy(), p.grad.cpu().numpy())
        print(f"RTG_GRAD full_b2 {name} rel_err={worst[name]:.3e} bar={bar(name):.0e}")
    for name, e in worst.items():
        assert e < bar(name), (name, e)


def test_float_observations_with_normalisation_match_float64():
    """Float observations through observation normalisation - the convolution reads PPO_IN_NONE - against the float64
    network on clamp((x - mu) / (std + eps), -5, 5) (rl/models.py:783-784), twice (the second forward replays the plan)."""
    dims, nA, B = (4, 36, 46), 6, 4
    torch.manual_seed(23)
    model = models.TVFModel("rtg", input_dims=dims, actions=nA, device="cuda", architecture="single", hidden_units=64,
                            head_scale=0.1, head_bias=True, observation_normalization=True)
    net = model.policy_net
    g = torch.Generator(device="cuda").manual_seed(1)
    for _ in range(3):
        model.obs_norm.update(3.0 * torch.randn((64, *dims), device="cuda", generator=g) + 1.0)
    x = 3.0 * torch.randn((B, *dims), device="cuda", generator=g) + 1.0
    mu, std = model.obs_norm.mu.double().view(dims), model.obs_norm.std.double().view(dims)
    xn = torch.clamp((x.double() - mu) / (std + model.obs_norm.norm_eps), -5, 5)
    assert float(xn.std()) > 0.5 and float((x - xn.float()).abs().max()) > 1.0  # really normalised
    sd = {k: v.detach().double() for k, v in net.params.items()}
    want = float64_network(sd, xn).cpu().numpy()
    for _ in range(2):
        got = net.forward(x)["_heads"]
        torch.cuda.synchronize()
        assert rel_err(got.cpu().numpy(), want) < 1e-4
    (calls, *_rest), = net._plans.values()
    assert calls[0][1] == "ppo_obs_normalize_f32" and calls[1][1] == "ppo_conv2d_strided_forward_f32"
    assert calls[1][2][1] == models.IN_NONE


FLAGS = ["--agents=8", "--n_steps=16", "--model_encoder=rtg", "--env_type=synthetic", "--env_embed_time=False", "--seed=4",
         "--policy_opt_mini_batch_size=64", "--policy_opt_epochs=1", "--value_opt_mini_batch_size=64", "--value_opt_epochs=1", "--distil_opt_mini_batch_size=64",
         "--env_warmup_period=5"]


def make_runner(seed, tmp, architecture):
    from ppo_amd import envs, logger, rollout
    from ppo_amd.config import args
    args.setup([*FLAGS, f"--model_architecture={architecture}", f"--output_folder={tmp}"])
    assert args.model.encoder == "rtg"
    torch.manual_seed(seed)
    shape, nA = envs.get_env_spec()
    model = models.TVFModel(args.model.encoder, encoder_args=None, input_dims=shape, actions=nA, device="cuda",
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
    assert a.all_obs.dtype == torch.uint8 and a.policy_net.encoder_kind == "rtg"
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


def test_train_py_runs_with_the_rtg_encoder(tmp_path):
    """`python train.py --model_encoder=rtg`, in a fresh child process."""
    cmd = [sys.executable, os.path.join(ROOT, "train.py"), "--model_encoder=rtg", "--env_type=synthetic", "--device=cuda:0",
           "--agents=8", "--n_steps=16", f"--epochs={(2 * 8 * 16 - 1) / 1e6}", "--policy_opt_mini_batch_size=64",
           "--value_opt_mini_batch_size=64", "--distil_opt_mini_batch_size=64", "--env_warmup_period=5",
           f"--output_folder={tmp_path}", "--restore=never"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
