"""GPU: the IMPALA encoder with batch_norm=True (rl/impala.py:63-76) - DualHeadNet's own pair of methods on the kernels of
csrc/batchnorm.hip - against float64 torch (tests/impala_batchnorm_torch.py) on the same parameters, buffers and inputs,
and against the reference's own outputs, buffers and gradients (tests/golden/impala_batchnorm_golden.npz,
make_impala_batchnorm_golden.py).  Biases, beta and log_std are non-zero (oracle/trained_params.perturbed_state_dict);
gamma and the running statistics are randomised here.

Bars, the project's own (tests/test_impala_downsample_gpu.py): forward rows, buffers and encoder.stacks.* gradients - the
batch-norm ones included - within 1e-4 of the reference tensor's max, dense and head gradients within 1e-5.  Gradients are
compared with every ReLU mask and max-pool selection taken from the net's own saved maps."""
import functools
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import impala_batchnorm_torch as BN  # noqa: E402
from oracle import model_torch as R  # noqa: E402
from oracle import trained_params as T  # noqa: E402
from ppo_amd import models  # noqa: E402

N_ACTIONS = 6
HEADS = ("raw_policy", "log_policy", "value", "advantage")
TAGS = ["pool", "stride"]
# name -> (input dims, batch, encoder arguments); the two fixture sets' geometries, the Atari shape (specialised
# convolution kernels, 16-byte aligned and odd planes) and a net whose last map is 1x1
CASES = {
    "pool_4x20x20": ((4, 20, 20), 8, {}),
    "stride_3x12x10_c8_16_b1": ((3, 12, 10), 8, {"down_sample": "stride", "channels": (8, 16), "n_block": 1}),
    "pool_4x84x84": ((4, 84, 84), 2, {}),
    "pool_2x5x6": ((2, 5, 6), 5, {}),
}
FUSED = ("stack_full", "stack_chain", "stack_tail", "block_forward", "bf16x3")


def recording(net):
    """The names of the launches `net` makes from here on."""
    calls, orig = [], net._call
    net._call = lambda fn, *a: (calls.append(fn), orig(fn, *a))[1]
    return calls


def randomise_bn(net, seed):
    """gamma ~ U(0.5, 1.5), running_mean ~ N(0, 0.2), running_var ~ U(0.5, 2), a counter that is not zero."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name, t in net.state_dict().items():
        if ".bn" not in name:
            continue
        kind = name.rsplit(".", 1)[1]
        if kind == "weight":
            sd[name] = torch.rand(t.shape, generator=g) + 0.5
        elif kind == "running_mean":
            sd[name] = torch.randn(t.shape, generator=g) * 0.2
        elif kind == "running_var":
            sd[name] = torch.rand(t.shape, generator=g) * 1.5 + 0.5
        elif kind == "num_batches_tracked":
            sd[name] = torch.tensor(5)
    net.load_state_dict(sd, strict=False)


def build(dims, enc, precision="high", seed=11):
    torch.manual_seed(seed)
    net = models.DualHeadNet("impala", dims, N_ACTIONS, hidden_units=64, head_scale=0.1, head_bias=True, device="cuda",
                             batch_norm=True, precision=precision, **enc)
    net.load_state_dict(T.perturbed_state_dict(net.state_dict(), seed=21))
    randomise_bn(net, 3)
    return net


def geom(net):
    return dict(n_stacks=len(net.spec.channels), n_block=net.spec.n_block, down_sample=net.spec.down_sample)


def double_sd(net):
    return {k: (v.detach().cpu().double() if v.is_floating_point() else v.detach().cpu().clone()) for k, v in net.state_dict().items()}


@functools.lru_cache(maxsize=None)
def case(name):
    """The net of one case in eval mode, its uint8 input and its float64 eval-mode forward, built once."""
    dims, B, enc = CASES[name]
    net = build(dims, enc).eval()
    x = torch.randint(0, 256, (B, *dims), generator=torch.Generator().manual_seed(5), dtype=torch.uint8)
    with torch.no_grad():
        ref = BN.forward_eval(double_sd(net), x.double() / 255.0, **geom(net))
    return net, x.cuda(), ref


def rel_err(got, ref):
    got, ref = torch.as_tensor(got).detach().cpu().double(), torch.as_tensor(ref).detach().cpu().double()
    return (got - ref.reshape(got.shape)).abs().max().item() / max(ref.abs().max().item(), 1e-30)


def bar(name):
    return 1e-4 if name.startswith("encoder.stacks.") else 1e-5


@pytest.mark.parametrize("name", list(CASES))
def test_eval_forward_against_float64(name):
    net, x, ref = case(name)
    assert net.batch_norm and not net.training and net.takes_obs_index(x) is False and not net.split_bf16
    out = net.forward(x)
    for key, got in (("raw_policy", out["raw_policy"]), ("value", out["value"]), ("h", out["_acts"]["h"])):
        e = rel_err(got, ref[key])
        print(f"IMPALA_BN eval forward {name} {key} rel_err={e:.3e}")
        assert e < 1e-4, (name, key, e)


@pytest.mark.parametrize("name", list(CASES))
def test_train_mode_forwards_against_float64(name):
    """Two consecutive batch-statistics forwards of a fresh net: outputs and every buffer against the float64 replay."""
    dims, B, enc = CASES[name]
    net = build(dims, enc)
    assert net.training  # nn.Module's default
    sd = double_sd(net)
    for step in range(2):
        x = torch.randint(0, 256, (B, *dims), generator=torch.Generator().manual_seed(40 + step), dtype=torch.uint8)
        with torch.no_grad():
            ref, new = BN.forward_train(sd, x.double() / 255.0, **geom(net))
        sd.update(new)
        out = net.forward(x.cuda())
        torch.cuda.synchronize()
        for key in ("raw_policy", "value"):
            e = rel_err(out[key], ref[key])
            print(f"IMPALA_BN train forward {name} step {step} {key} rel_err={e:.3e}")
            assert e < 1e-4, (name, step, key, e)
        for bname, t in net.buffers.items():
            if bname.endswith("num_batches_tracked"):
                assert int(t) == int(sd[bname]) == 6 + step
            else:
                e = rel_err(t, sd[bname])
                assert e < 1e-4, (name, step, bname, e)


@pytest.mark.parametrize("name", list(CASES))
def test_recorded_and_replayed_plans_agree(name):
    """Eval mode: the plan's replay and the training forward give the recorded forward's bits.  Training mode: two nets
    from one state, one recording then replaying its plan, one with plans off - same bits, same buffers."""
    net, x, _ref = case(name)
    first = net.forward(x)["_acts"]["h"].clone()
    replay = net.forward(x)["_acts"]["h"].clone()
    assert any(k[1] == x.shape[0] and k[-1] is False for k in net._plans), "no eval-mode launch plan for this batch"
    acts, _o, _B, _dheads = net._train_forward(x)
    assert torch.equal(first, replay) and torch.equal(first, acts["h"])
    dims, B, enc = CASES[name]
    a, b = build(dims, enc), build(dims, enc)
    b.use_plans = False
    for step in range(3):  # a: recorded, replayed, replayed
        ha, hb = a.forward(x)["_acts"]["h"].clone(), b.forward(x)["_acts"]["h"].clone()
        assert torch.equal(ha, hb), step
        for bname in a.buffers:
            assert torch.equal(a.buffers[bname], b.buffers[bname]), (step, bname)
    assert any(k[-1] is True for k in a._plans) and not b._plans
    assert int(next(t for n, t in a.buffers.items() if n.endswith("tracked"))) == 5 + 3
    # the two modes are different plans of one net
    h_eval = a.eval().forward(x)["_acts"]["h"].clone()
    assert not torch.equal(h_eval, ha) and {k[-1] for k in a._plans} == {True, False}


def test_training_forward_in_training_mode_raises():
    dims, _B, enc = CASES["pool_2x5x6"]
    net = build(dims, enc)
    x = torch.zeros((3, *dims), dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match="batch statistics"):
        net.encode(x, train=True)
    with pytest.raises(RuntimeError, match="batch statistics"):
        net._train_forward(x)
    net.eval()
    net._train_forward(x)
    assert net.train() is net and net.training and not net.eval().training


@pytest.mark.parametrize("name", list(CASES))
def test_gradients_against_float64_with_shared_kinks(name):
    net, x, _ref = case(name)
    B = x.shape[0]
    g = torch.Generator(device="cpu").manual_seed(17)
    actions = torch.randint(0, N_ACTIONS, (B,), generator=g, dtype=torch.int32).cuda()
    old_log_pac = (torch.randn(B, generator=g) * 0.1 - 1.7).cuda()
    old_log_policy = torch.log_softmax(torch.randn(B, N_ACTIONS, generator=g), dim=1).cuda()
    adv = torch.randn(B, generator=g).cuda()
    # returns well away from the values, all on one side (see tests/test_impala_downsample_gpu.py)
    ret = (torch.randn(B, 1, generator=g) * 0.3 + 3.0).cuda()
    before = {k: v.clone() for k, v in net.buffers.items()}
    calls = recording(net)
    try:
        acts, o, B_, dheads = net._train_forward(x)
        stats = net._buf("loss_stats", (B, 8))
        net._call("ppo_ppo_loss_f32", o.data_ptr(), B, net.nh, net.n_actions, net.vh, actions.data_ptr(), old_log_pac.data_ptr(),
                  old_log_policy.data_ptr(), adv.data_ptr(), ret.data_ptr(), 0.2, 0.01, 0.5, 1.0 / B, dheads.data_ptr(),
                  stats.data_ptr(), None)
        net.backward(acts, dheads)
        torch.cuda.synchronize()
    finally:
        del net._call
    n_bn = 2 * net.spec.n_block * len(net.spec.channels)
    assert calls.count("ppo_batchnorm_running_forward_f32") == n_bn and calls.count("ppo_batchnorm_running_backward_f32") == n_bn
    assert "ppo_batchnorm_batch_forward_f32" not in calls and not [c for c in calls if any(f in c for f in FUSED)], calls
    assert all(torch.equal(before[k], v) for k, v in net.buffers.items()), "an eval-mode pass changed a buffer"
    sd = {k: (v.detach().cpu().double().requires_grad_(k in net.params) if v.is_floating_point() else v.cpu())
          for k, v in net.state_dict().items()}
    cpu_acts = {k: v.cpu() for k, v in acts.items() if isinstance(v, torch.Tensor)}
    out = BN.forward_eval_shared_kinks(sd, x.cpu().double() / 255.0, cpu_acts, **geom(net))
    loss = R.ppo_loss(out, actions.cpu().long(), old_log_pac.cpu().double(), adv.cpu().double(), ret.cpu().double())
    assert torch.isfinite(loss)
    loss.backward()
    worst = {}
    for pname in net.params:
        p = sd[pname]
        if p.grad is None:  # advantage head, log_std: not in this loss
            assert float(net.grads[pname].abs().max()) == 0.0, pname
            continue
        assert float(p.grad.abs().max()) > 0, pname
        worst[pname] = rel_err(net.grads[pname], p.grad)
        print(f"IMPALA_BN gradient {name} {pname} rel_err={worst[pname]:.3e} bar={bar(pname):.0e}")
    assert sum(".bn" in n for n in worst) == 2 * n_bn
    for pname, e in worst.items():
        assert e < bar(pname), (name, pname, e)


def test_precision_medium_changes_no_bit():
    hi, x, _ref = case("pool_4x84x84")
    dims, _B, enc = CASES["pool_4x84x84"]
    md = build(dims, enc, precision="medium").eval()
    assert not md.split_bf16
    calls = recording(md)
    try:
        got = md.forward(x)["_acts"]["h"].clone()
        acts, _o, B, dheads = md._train_forward(x)
        dheads.fill_(1.0 / B)
        md.backward(acts, dheads)
        g_md = md.grad.clone()
    finally:
        del md._call
    assert not [c for c in calls if any(f in c for f in FUSED)], calls
    acts, _o, B, dheads = hi._train_forward(x)
    dheads.fill_(1.0 / B)
    hi.backward(acts, dheads)
    assert torch.equal(got, hi.forward(x)["_acts"]["h"]) and torch.equal(g_md, hi.grad)


def test_the_default_path_is_untouched():
    """A net without batch norm built in the same process makes the launches and the bits it makes when the argument is
    not given at all, fused launches among them, and has no buffers or batch-norm parameters."""
    case("pool_4x84x84")
    x = torch.randint(0, 256, (3, 4, 84, 84), generator=torch.Generator().manual_seed(2), dtype=torch.uint8).cuda()
    outs, lists = [], []
    for kwargs in ({}, {"batch_norm": False}):
        torch.manual_seed(7)
        net = models.DualHeadNet("impala", (4, 84, 84), N_ACTIONS, hidden_units=64, head_scale=0.1, head_bias=True,
                                 device="cuda", **kwargs)
        assert not net.batch_norm and not net.buffers and not [n for n in net.params if ".bn" in n]
        assert net.takes_obs_index(x) and all(len(k) == 4 for k in net._plans)
        calls = recording(net)
        outs.append({k: v.clone() for k, v in net.forward(x).items() if k in HEADS})
        acts, _o, B, dheads = net._train_forward(x)
        dheads.fill_(1.0 / B)
        net.backward(acts, dheads)
        torch.cuda.synchronize()
        outs[-1]["grad"] = net.grad.clone()
        lists.append(list(calls))
        assert all(len(k) == 4 for k in net._plans)
        assert not [c for c in calls if "batchnorm" in c] and [c for c in calls if "stack" in c]
    assert lists[0] == lists[1]
    for k in outs[0]:
        assert torch.equal(outs[0][k], outs[1][k]), k


# ---------------------------------------------------------------------------------------------- against the reference
@pytest.fixture(scope="module")
def gold(golden_dir):
    return (np.load(os.path.join(golden_dir, "impala_batchnorm_golden.npz")),
            json.load(open(os.path.join(golden_dir, "impala_batchnorm_golden.json"))))


def make_golden_net(g, meta, tag):
    enc = {k: (tuple(v) if isinstance(v, list) else v) for k, v in meta[tag]["encoder_args"].items()}
    torch.manual_seed(meta[tag]["seed"])
    net = models.DualHeadNet("impala", tuple(meta[tag]["input_dims"]), meta["n_actions"], hidden_units=meta[tag]["hidden_units"],
                             head_scale=meta["head_scale"], head_bias=meta["head_bias"], device="cuda", **enc)
    assert net.batch_norm and net.training
    net.load_state_dict({f"{name}.{p}": torch.from_numpy(g[f"{tag}_bn_{name}.{p}"]) for name in meta[tag]["bn_layers"]
                         for p in ("weight", "bias")}, strict=False)
    return net


def golden_train_forwards(g, meta, tag, net):
    for k in range(meta["n_train_forwards"]):
        out = net.forward(torch.from_numpy(g[f"{tag}_train{k}_x"]).cuda(), policy_temperature=1.0)
        torch.cuda.synchronize()
        for key in HEADS:
            e = rel_err(out[key], g[f"{tag}_train{k}_{key}"])
            print(f"IMPALA_BN golden train forward {tag} {k} {key} rel_err={e:.3e}")
            assert e < 1e-4, (tag, k, key, e)
        for name, t in net.buffers.items():
            ref = g[f"{tag}_train{k}_buf_{name}"]
            if name.endswith("num_batches_tracked"):
                assert int(t) == int(ref) == k + 1, name
            else:
                assert rel_err(t, ref) < 1e-4, (tag, k, name)


@pytest.mark.parametrize("tag", TAGS)
def test_matches_reference(gold, tag):
    """The fixture's whole sequence: key order, three train-mode forwards with their buffers, then eval mode - one forward
    and one policy minibatch with every gradient."""
    g, meta = gold
    assert meta[tag]["relu_margin"] >= 1e-5 and (meta[tag]["pool_margin"] is None or meta[tag]["pool_margin"] >= 1e-5)
    net = make_golden_net(g, meta, tag)
    assert list(net.state_dict().keys()) == meta[tag]["state_dict_keys"]
    assert net.parameter_order() == meta[tag]["param_names"]
    assert net.n_parameters() == sum(int(np.prod(v["shape"])) for v in meta[tag]["params"].values())
    golden_train_forwards(g, meta, tag, net)
    net.eval()
    kept = {k: v.clone() for k, v in net.buffers.items()}
    x = torch.from_numpy(g[f"{tag}_fwd_x"]).cuda()
    for _ in range(2):  # the second forward replays the recorded launch plan
        out = net.forward(x, policy_temperature=1.0)
        torch.cuda.synchronize()
        for k in HEADS:
            e = rel_err(out[k], g[f"{tag}_fwd_{k}"])
            print(f"IMPALA_BN golden eval forward {tag} {k} rel_err={e:.3e}")
            assert e < 1e-4, (tag, k, e)
    d = {k: g[f"{tag}_mb_{k}"] for k in ("prev_state", "actions", "log_policy", "log_pac", "advantages", "returns")}
    stats = net.ppo_minibatch(
        torch.from_numpy(d["prev_state"]).cuda(), torch.from_numpy(d["actions"].astype(np.int32)).cuda(),
        torch.from_numpy(d["log_pac"]).cuda(), torch.from_numpy(d["log_policy"]).cuda(),
        torch.from_numpy(d["advantages"]).cuda(), torch.from_numpy(d["returns"]).cuda(),
        eps_clip=meta["ppo_epsilon"], ent_coef=meta["entropy_bonus"], vf_coef=meta["ppo_vf_coef"], loss_scale=1.0)
    torch.cuda.synchronize()
    s = stats.cpu().numpy().astype(np.float64)
    loss, kl_approx, kl_true, clip_frac = g[f"{tag}_mb_result"]
    assert abs(-s[:, 6].mean() - loss) < 1e-4 * max(1.0, abs(loss))
    assert abs(s[:, 4].mean() - kl_approx) < 1e-5 + 1e-4 * abs(kl_approx)
    assert abs(s[:, 5].mean() - kl_true) < 1e-5 + 1e-4 * abs(kl_true)
    assert abs(s[:, 3].mean() - clip_frac) < 1e-9
    assert all(torch.equal(kept[k], v) for k, v in net.buffers.items())
    worst = {}
    for name in meta[tag]["param_names"]:
        if name in meta[tag]["grad_none"]:
            assert float(net.grads[name].abs().max()) == 0.0, name
            continue
        worst[name] = rel_err(net.grads[name], g[f"{tag}_grad_{name}"])
        print(f"IMPALA_BN golden gradient {tag} {name} rel_err={worst[name]:.3e} bar={bar(name):.0e}")
    for name, e in worst.items():
        assert e < bar(name), (tag, name, e)


@pytest.mark.parametrize("tag", TAGS)
def test_state_dict_round_trips(gold, tag):
    g, meta = gold
    a = make_golden_net(g, meta, tag)
    golden_train_forwards(g, meta, tag, a)
    sd = OrderedDictCopy(a.state_dict())
    assert list(sd) == meta[tag]["state_dict_keys"]
    assert sd[meta[tag]["bn_layers"][0] + ".num_batches_tracked"].dtype == torch.int64
    torch.manual_seed(1)
    b = make_golden_net(g, meta, tag)
    b.load_state_dict(sd)
    for k, v in b.state_dict().items():
        assert torch.equal(v, sd[k].cuda()), k
    missing = {k: v for k, v in sd.items() if not k.endswith("bn0.running_var")}
    with pytest.raises(KeyError, match="running_var"):
        b.load_state_dict(missing)
    x = torch.from_numpy(g[f"{tag}_fwd_x"]).cuda()
    assert torch.equal(a.eval().forward(x)["raw_policy"], b.eval().forward(x)["raw_policy"])
    # the optimiser state keeps the reference's parameter indices
    a.exp_avg, a.exp_avg_sq, a._adam_step = torch.ones_like(a.flat), torch.ones_like(a.flat), 3
    osd = a.optimizer_state_dict()
    assert osd["param_groups"][0]["params"] == list(range(len(meta[tag]["param_names"])))
    i = meta[tag]["param_names"].index(meta[tag]["bn_layers"][0] + ".weight")
    assert tuple(osd["state"][i]["exp_avg"].shape) == tuple(a.params[meta[tag]["bn_layers"][0] + ".weight"].shape)


def OrderedDictCopy(sd):
    from collections import OrderedDict
    return OrderedDict((k, v.detach().cpu().clone()) for k, v in sd.items())
