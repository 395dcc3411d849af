"""GPU: the Nature-CNN encoder under --precision=medium (DualHeadNet(precision=...)): the convolution passes listed in
models.NATURE_SPLIT run as split-bf16 launches (csrc/conv_strided_bf16x3.hip), `high` calls exactly what it called.

Forward: head outputs at both geometries of tests/golden/nature_golden.npz within 1e-4 of each tensor's largest entry
(the project's forward bar for the split mode), and not the bits of `high`.

Gradients: one policy minibatch at the small geometry against a float64 restatement whose ReLU gates are taken from
the net under test (acts[name] > 0) - the exact gradient of the function the net computed, so a ReLU that the split
forward flipped cannot fail the test.  Bar: 1e-4 of each tensor's largest entry, the bar() tests/test_nature_gpu.py holds
convolution gradients to (the linear layer and the heads run in exact float32 but on activations that carry the
convolutions' split error, so they share it).  Measured (MI355X), medium / high:

    encoder.conv1.weight 8.714e-06 / 2.222e-07    encoder.conv1.bias 9.449e-06 / 1.992e-07
    encoder.conv2.weight 7.507e-06 / 2.657e-07    encoder.conv2.bias 6.774e-06 / 1.510e-07
    encoder.conv3.weight 6.621e-06 / 1.860e-07    encoder.conv3.bias 5.244e-07 / 1.280e-07
    encoder.fc.weight    7.004e-06 / 1.478e-07    encoder.fc.bias    6.553e-07 / 8.246e-08
    policy_head.weight   7.913e-06 / 2.999e-07    policy_head.bias   8.643e-07 / 7.524e-08
    value_head.weight    7.436e-06 / 1.824e-07    value_head.bias    2.895e-08 / 9.642e-08
    advantage_head.*     0 / 0 (no gradient reaches it from the policy loss)

(with the six listed passes split; with the weight gradients of conv2 and conv3 split as well the worst was conv2.weight
at 1.105e-05).  Forward, medium / high: small 3.8e-07 - 1.2e-05 / 1.9e-07 - 1.8e-06, full 5.2e-07 -
1.6e-05 / 1.9e-07 - 1.5e-06.  Nothing is over the bar.

A two-iteration Runner under medium resumes bit-identically from its checkpoint, whose key tree is a `high` run's, and
train.py --model_encoder=nature --precision=medium exits 0."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
import torch.nn.functional as F  # noqa: E402

from ppo_amd import models  # noqa: E402
from test_nature_gpu import FLAGS, ROOT, gold, iteration, rel_err  # noqa: E402,F401  (gold: a fixture)

LAYERS = ("conv1", "conv2", "conv3")
GRAD_BAR = 1e-4  # of each tensor's largest entry


def build(meta, tag, precision):
    torch.manual_seed(meta[tag]["seed"])
    net = models.DualHeadNet("nature", tuple(meta[tag]["input_dims"]), meta["n_actions"], hidden_units=meta[tag]["hidden_units"],
                             head_scale=meta["head_scale"], head_bias=meta["head_bias"], device="cuda", precision=precision)
    calls = []
    orig = net._call
    net._call = lambda fn, *a: (calls.append(fn), orig(fn, *a))[1]
    return net, calls


def entry(layer, conv_pass, split):
    return f"ppo_conv2d_strided_{conv_pass}_" + ("bf16x3" if split and (layer, conv_pass) in models.NATURE_SPLIT else "f32")


def expected_calls(split):
    """The strided-convolution launches of one training forward + backward, in order."""
    fwd = [entry(layer, "forward", split) for layer in LAYERS]
    bwd = []
    for layer in reversed(LAYERS):
        bwd.append(entry(layer, "backward_weight", split))
        if layer != "conv1":
            bwd.append(entry(layer, "backward_data", split))
    return fwd + bwd


def minibatch(net, g, meta):
    d = {k: g[f"small_mb_{k}"] for k in ("prev_state", "actions", "log_policy", "log_pac", "advantages", "returns")}
    net.grad.zero_()
    net.ppo_minibatch(
        torch.from_numpy(d["prev_state"]).cuda(), torch.from_numpy(d["actions"].astype(np.int32)).cuda(),
        torch.from_numpy(d["log_pac"]).cuda(), torch.from_numpy(d["log_policy"]).cuda(),
        torch.from_numpy(d["advantages"]).cuda(), torch.from_numpy(d["returns"]).cuda(),
        eps_clip=meta["ppo_epsilon"], ent_coef=meta["entropy_bonus"], vf_coef=meta["ppo_vf_coef"], loss_scale=1.0)
    torch.cuda.synchronize()
    return d


def float64_gradients(net, d, meta):
    """d loss / d parameter in float64 of NatureCNN + heads with every ReLU replaced by the gate the net itself took."""
    from oracle import model_torch as R
    x = torch.from_numpy(d["prev_state"]).cuda()
    acts = net.encode(x, train=True)
    torch.cuda.synchronize()
    gates = {k: (acts[k] > 0).double().cpu() for k in (*LAYERS, "h")}
    sd = {k: v.detach().double().cpu().requires_grad_(True) for k, v in net.params.items()}
    h = torch.from_numpy(d["prev_state"]).double() / 255.0 if d["prev_state"].dtype == np.uint8 \
        else torch.from_numpy(d["prev_state"]).double()
    for name, stride in zip(LAYERS, (4, 2, 1)):
        h = F.conv2d(h, sd[f"encoder.{name}.weight"], sd[f"encoder.{name}.bias"], stride=stride) * gates[name]
    feat = F.linear(h.reshape(h.shape[0], -1), sd["encoder.fc.weight"], sd["encoder.fc.bias"]) * gates["h"]
    nA = meta["n_actions"]
    o = torch.cat([F.linear(feat, sd[f"{n}.weight"], sd.get(f"{n}.bias")) for n in ("policy_head", "value_head", "advantage_head")], 1)
    out = {"log_policy": torch.log_softmax(o[:, :nA], dim=1), "value": o[:, nA:nA + 1]}
    loss = R.ppo_loss(out, torch.from_numpy(d["actions"]).long(), torch.from_numpy(d["log_pac"]).double(),
                      torch.from_numpy(d["advantages"]).double(), torch.from_numpy(d["returns"]).double(),
                      eps=meta["ppo_epsilon"], ent_coef=meta["entropy_bonus"], vf_coef=meta["ppo_vf_coef"])
    loss.backward()
    return {k: (None if p.grad is None else p.grad.numpy()) for k, p in sd.items()}


def test_medium_takes_the_listed_split_launches_and_high_none(gold):
    g, meta = gold
    hi, calls_hi = build(meta, "small", "high")
    md, calls_md = build(meta, "small", "medium")
    assert torch.equal(hi.flat, md.flat)
    assert md.split_bf16 == bool(models.NATURE_SPLIT) and not hi.split_bf16 and md.precision == "medium"
    for net in (hi, md):
        minibatch(net, g, meta)

    def strided(calls):
        return [c for c in calls if c.startswith("ppo_conv2d_strided_")]
    assert strided(calls_hi) == expected_calls(False) and not any("bf16x3" in c for c in calls_hi)
    assert strided(calls_md) == expected_calls(True)
    assert sum("bf16x3" in c for c in calls_md) == len(models.NATURE_SPLIT)
    assert [c for c in calls_md if "strided" not in c] == [c for c in calls_hi if "strided" not in c]
    assert set(md._bufs) == set(hi._bufs), "the split mode added a buffer"
    assert list(md.state_dict().keys()) == list(hi.state_dict().keys())


@pytest.mark.parametrize("tag", ["small", "full"])
def test_forward_is_inside_the_split_bar(gold, tag):
    g, meta = gold
    hi, _ = build(meta, tag, "high")
    md, _ = build(meta, tag, "medium")
    x = torch.from_numpy(g[f"{tag}_fwd_x"]).cuda()
    o_hi = {k: v.clone() for k, v in hi.forward(x, policy_temperature=1.0).items() if torch.is_tensor(v)}
    for rep in range(2):  # the second forward replays the recorded launch plan
        o_md = md.forward(x, policy_temperature=1.0)
        torch.cuda.synchronize()
        for k in ("raw_policy", "log_policy", "value", "advantage"):
            e = rel_err(o_md[k].cpu().numpy(), g[f"{tag}_fwd_{k}"])
            print(f"NATURE_SPLIT_FWD {tag} {k} pass={rep} rel_err={e:.3e} high={rel_err(o_hi[k].cpu().numpy(), g[f'{tag}_fwd_{k}']):.3e}")
            assert e < 1e-4, (tag, k, e)
        if "forward" in {p for _l, p in models.NATURE_SPLIT}:
            assert not torch.equal(o_md["raw_policy"], o_hi["raw_policy"])


def test_gradients_match_float64_with_the_nets_own_gates(gold):
    g, meta = gold
    worst = {}
    for precision in ("high", "medium"):
        net, _ = build(meta, "small", precision)
        d = minibatch(net, g, meta)
        got = {k: v.detach().cpu().numpy().copy() for k, v in net.grads.items()}
        ref = float64_gradients(net, d, meta)
        for name, r in ref.items():
            if r is None:
                assert float(np.abs(got[name]).max()) == 0.0, name
                continue
            e = rel_err(got[name], r)
            print(f"NATURE_SPLIT_GRAD small {precision} {name} rel_err={e:.3e} bar={GRAD_BAR:.0e}")
            if precision == "medium":
                worst[name] = e
    for name, e in worst.items():
        assert e < GRAD_BAR, (name, e)


def key_tree(cp):
    """The keys of a checkpoint: top level, the model's tensors, and each optimiser's state_dict two levels down."""
    def keys(obj, depth):
        return {k: keys(v, depth - 1) for k, v in obj.items()} if isinstance(obj, dict) and depth else None
    return {k: keys(v, 2 if k.endswith("optimizer_state_dict") else 1 if k == "model_state_dict" else 0) for k, v in cp.items()}


def make_runner(seed, tmp, architecture, precision):
    from ppo_amd import envs, logger, rollout
    from ppo_amd.config import args
    args.setup([*FLAGS, f"--model_architecture={architecture}", f"--output_folder={tmp}", f"--precision={precision}"])
    torch.manual_seed(seed)
    shape, nA = envs.get_env_spec()
    model = models.TVFModel("nature", encoder_args={"base_channels": 32}, input_dims=shape, actions=nA, device="cuda",
                            architecture=architecture, hidden_units=512, head_scale=0.1, head_bias=True, precision=precision)
    r = rollout.Runner(model, logger.Logger(quiet=True))
    r.vec_env = envs.create_envs_classic()
    r.reset()
    return r


@pytest.mark.parametrize("architecture", ["single", "dual"])
def test_runner_under_medium_resumes_bit_identically(tmp_path, architecture):
    np.random.seed(9)
    a = make_runner(1, str(tmp_path), architecture, "medium")
    nets = [a.policy_net] if architecture == "single" else [a.policy_net, a.value_net]
    assert all(n.split_bf16 == bool(models.NATURE_SPLIT) and n.precision == "medium" for n in nets)
    for _ in range(2):
        iteration(a)
    torch.cuda.synchronize()
    for n in nets:
        assert torch.isfinite(n.flat).all() and torch.isfinite(n.grad).all()
    path = a.save_checkpoint(str(tmp_path / "checkpoint-000M-params.pt"), a.step)
    iteration(a)
    torch.cuda.synchronize()
    np.random.seed(12345)
    b = make_runner(2, str(tmp_path), architecture, "medium")
    assert b.load_checkpoint(str(tmp_path / "checkpoint-000M-params.pt")) == 2 * 8 * 16 and os.path.exists(path)
    iteration(b)
    torch.cuda.synchronize()
    assert torch.equal(a.all_obs, b.all_obs) and torch.equal(a.actions, b.actions)
    for na, nb in zip(nets, [b.policy_net] if architecture == "single" else [b.policy_net, b.value_net]):
        assert torch.equal(na.flat, nb.flat) and torch.equal(na.exp_avg, nb.exp_avg) and torch.equal(na.exp_avg_sq, nb.exp_avg_sq)
    # the checkpoint holds what a `high` run's holds: no key added
    np.random.seed(9)
    c = make_runner(1, str(tmp_path), architecture, "high")
    assert not c.policy_net.split_bf16
    iteration(c)
    high_path = c.save_checkpoint(str(tmp_path / "checkpoint-high-params.pt"), c.step)
    from ppo_amd import checkpoint
    assert key_tree(checkpoint.load(path)) == key_tree(checkpoint.load(high_path))


def test_train_py_runs_nature_under_medium(tmp_path):
    cmd = [sys.executable, os.path.join(ROOT, "train.py"), "--env_type=synthetic", "--model_encoder=nature", "--precision=medium",
           "--device=cuda:0", "--agents=8", "--n_steps=16", f"--epochs={(2 * 8 * 16 - 1) / 1e6}",
           "--policy_opt_mini_batch_size=64", "--value_opt_mini_batch_size=64", "--distil_opt_mini_batch_size=64",
           "--env_warmup_period=5", f"--output_folder={tmp_path}", "--restore=never"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
