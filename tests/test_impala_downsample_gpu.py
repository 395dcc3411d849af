"""GPU: the IMPALA encoder with down_sample='stride' (first convolutions on the generic stride-2 kernels,
ppo_conv3x3s2_any_*, no max-pool) and down_sample='none' (stride 1, no max-pool) against float64 torch
(tests/impala_downsample_torch.py) on the same parameters and inputs, and against the reference's own outputs and
gradients (tests/golden/impala_downsample_golden.npz, make_impala_downsample_golden.py).  Biases and log_std are non-zero
(oracle/trained_params.perturbed_state_dict).

Bars, the project's own: forward rows and encoder.stacks.* gradients within 1e-4 of the reference tensor's max, dense and
head gradients within 1e-5 (tests/test_impala_any_gpu.py, tests/test_nature_gpu.py); the --precision=medium forward within
1e-4 of the largest output (tests/test_bf16x3_gpu.py).  Gradients are compared with every ReLU mask taken from the net's
own saved activations; these modes have no max-pool, so nothing else is shared and no element is left out.
"""
import functools
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import impala_downsample_torch as D  # noqa: E402
from oracle import trained_params as T  # noqa: E402
from ppo_amd import models  # noqa: E402

N_ACTIONS = 6
# name -> (mode, input dims, batch, further encoder arguments)
CASES = {
    "stride_3x20x28": ("stride", (3, 20, 28), 5, {}),
    "stride_2x5x6": ("stride", (2, 5, 6), 4, {}),              # the last map is 1x1
    "stride_4x84x84": ("stride", (4, 84, 84), 2, {}),          # blocks on specialised / fused launches
    "stride_3x20x28_c8_24_b1": ("stride", (3, 20, 28), 5, {"channels": (8, 24), "n_block": 1}),
    "none_3x12x10_c8_16_b1": ("none", (3, 12, 10), 5, {"channels": (8, 16), "n_block": 1}),
    "none_1x9x9": ("none", (1, 9, 9), 7, {}),
}


def first_convs(net):
    return [f"encoder.stacks.{si}.firstconv" for si in range(len(net.spec.channels))]


def recording(net):
    """The names of the launches `net` makes from here on."""
    calls, orig = [], net._call
    net._call = lambda fn, *a: (calls.append(fn), orig(fn, *a))[1]
    return calls


@functools.lru_cache(maxsize=None)
def case(name):
    """The net of one case (biases and log_std non-zero), its uint8 input and its float64 forward, built once."""
    mode, dims, B, enc = CASES[name]
    torch.manual_seed(11)
    net = models.DualHeadNet("impala", dims, N_ACTIONS, hidden_units=64, head_scale=0.1, head_bias=True, device="cuda",
                             down_sample=mode, **enc)
    net.load_state_dict(T.perturbed_state_dict(net.state_dict(), seed=21))
    g = torch.Generator(device="cpu").manual_seed(5)
    x = torch.randint(0, 256, (B, *dims), generator=g, dtype=torch.uint8)
    n_stacks, n_block = len(net.spec.channels), net.spec.n_block
    with torch.no_grad():
        ref = D.forward(T.as_double(net.state_dict()), x.double() / 255.0, n_stacks=n_stacks, n_block=n_block, down_sample=mode)
    return net, x.cuda(), ref, n_stacks, n_block, mode


def rel_err(got, ref):
    got, ref = torch.as_tensor(got).detach().cpu().double(), torch.as_tensor(ref).detach().cpu().double()
    return (got - ref.reshape(got.shape)).abs().max().item() / max(ref.abs().max().item(), 1e-30)


@pytest.mark.parametrize("name", list(CASES))
def test_generic_convs_and_the_gathered_minibatch_path(name):
    net, x, _ref, _ns, _nb, mode = case(name)
    assert net.spec.down_sample == mode
    if mode == "stride":
        assert all(fc in net.generic_convs for fc in first_convs(net))
        assert not any((fc, tr) in net._pk for fc in first_convs(net) for tr in (0, 1)), "a strided convolution has packed weights"
    if name == "stride_4x84x84":
        assert net.generic_convs == first_convs(net)  # only those: the blocks keep their specialised kernels
    assert net.takes_obs_index(x) is False
    index = torch.arange(x.shape[0], dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError):
        net._train_forward(x, index, obs_indexed=True)


@pytest.mark.parametrize("name", list(CASES))
def test_forward_against_float64(name):
    net, x, ref, _ns, _nb, _mode = case(name)
    out = net.forward(x)
    for key, got in (("raw_policy", out["raw_policy"]), ("value", out["value"]), ("h", out["_acts"]["h"])):
        e = rel_err(got, ref[key])
        print(f"IMPALA_DS forward {name} {key} rel_err={e:.3e}")
        assert e < 1e-4, (name, key, e)


@pytest.mark.parametrize("name", list(CASES))
def test_inference_plan_and_training_forward_agree_bitwise(name):
    net, x, _ref, _ns, _nb, _mode = case(name)
    first = net.forward(x)["_acts"]["h"].clone()        # records the launch plan (or replays an earlier test's)
    replay = net.forward(x)["_acts"]["h"].clone()       # replays it
    assert any(k[1] == x.shape[0] for k in net._plans), "no launch plan was recorded for this batch"
    acts, _o, _B, _dheads = net._train_forward(x)
    assert torch.equal(first, replay) and torch.equal(first, acts["h"])


@pytest.mark.parametrize("name", list(CASES))
def test_no_launch_with_a_max_pool_is_taken(name):
    net, x, _ref, n_stacks, _nb, mode = case(name)
    calls = recording(net)
    try:
        acts, _o, B, dheads = net._train_forward(x)
        dheads.fill_(1.0 / B)
        net.backward(acts, dheads)
        torch.cuda.synchronize()
    finally:
        del net._call
    assert not [c for c in calls if "pool" in c or "stack_full" in c or "stack_chain" in c], calls
    for si in range(n_stacks):
        assert acts[f"idx{si}"] is None
    assert not any(k[0].startswith("tidx") for k in net._bufs)
    if mode == "stride":
        assert calls.count("ppo_conv3x3s2_any_forward_f32") == n_stacks
        assert calls.count("ppo_conv3x3s2_any_backward_weight_f32") == n_stacks
        assert calls.count("ppo_conv3x3s2_any_backward_data_f32") == n_stacks - 1
    else:
        assert not [c for c in calls if "s2_any" in c]
    if name == "stride_4x84x84":
        # the residual blocks behind the strided convolutions keep the launches of the 'pool' net
        assert calls.count("ppo_impala_stack_tail_forward_f32") == 2 and calls.count("ppo_impala_stack_tail_backward_f32") >= 2
        assert "ppo_conv3x3_any_forward_f32" not in calls


@pytest.mark.parametrize("name", list(CASES))
def test_gradients_against_float64_with_shared_kinks(name):
    from oracle import model_torch as R
    net, x, _ref, n_stacks, n_block, mode = case(name)
    B = x.shape[0]
    g = torch.Generator(device="cpu").manual_seed(17)
    actions = torch.randint(0, N_ACTIONS, (B,), generator=g, dtype=torch.int32).cuda()
    old_log_pac = (torch.randn(B, generator=g) * 0.1 - 1.7).cuda()
    old_log_policy = torch.log_softmax(torch.randn(B, N_ACTIONS, generator=g), dim=1).cuda()
    adv = torch.randn(B, generator=g).cuda()
    # Returns well away from the values, all on one side: see tests/test_impala_any_gpu.py (value_head.bias is ONE number
    # whose gradient is a sum that must not cancel for "1e-5 of the tensor's max" to speak about a kernel).
    ret = (torch.randn(B, 1, generator=g) * 0.3 + 3.0).cuda()
    acts, o, B_, dheads = net._train_forward(x)
    assert B_ == B
    stats = net._buf("loss_stats", (B, 8))
    net._call("ppo_ppo_loss_f32", o.data_ptr(), B, net.nh, net.n_actions, net.vh, actions.data_ptr(), old_log_pac.data_ptr(),
              old_log_policy.data_ptr(), adv.data_ptr(), ret.data_ptr(), 0.2, 0.01, 0.5, 1.0 / B, dheads.data_ptr(),
              stats.data_ptr(), None)
    net.backward(acts, dheads)
    torch.cuda.synchronize()
    sd = {k: v.detach().double().requires_grad_(True) for k, v in net.params.items()}
    out = D.forward_shared_kinks(sd, x.double() / 255.0, acts, n_stacks=n_stacks, n_block=n_block, down_sample=mode)
    loss = R.ppo_loss(out, actions.long(), old_log_pac.double(), adv.double(), ret.double())
    assert torch.isfinite(loss)
    loss.backward()
    worst = {}
    for pname, p in sd.items():
        if p.grad is None:  # advantage head, log_std: not in this loss
            assert float(net.grads[pname].abs().max()) == 0.0, pname
            continue
        assert float(p.grad.abs().max()) > 0, pname
        e = rel_err(net.grads[pname], p.grad)
        worst[pname] = e
        bar = 1e-4 if pname.startswith("encoder.stacks.") else 1e-5
        print(f"IMPALA_DS gradient {name} {pname} rel_err={e:.3e} bar={bar:.0e}")
    for pname, e in worst.items():
        assert e < (1e-4 if pname.startswith("encoder.stacks.") else 1e-5), (name, pname, e)


def test_the_default_path_is_untouched():
    """A 'pool' net built in the same process as the others keeps every specialised launch and its bits."""
    case("stride_4x84x84")
    x = torch.randint(0, 256, (3, 4, 84, 84), generator=torch.Generator(device="cpu").manual_seed(2), dtype=torch.uint8).cuda()
    outs = []
    for kwargs in ({}, {"down_sample": "pool"}):
        torch.manual_seed(7)
        net = models.DualHeadNet("impala", (4, 84, 84), N_ACTIONS, hidden_units=64, head_scale=0.1, head_bias=True,
                                 device="cuda", **kwargs)
        assert net.spec.down_sample == "pool" and net.generic_convs == []
        assert net.takes_obs_index(x)
        calls = recording(net)
        outs.append({k: v.clone() for k, v in net.forward(x).items() if k in ("raw_policy", "value", "advantage")})
        torch.cuda.synchronize()
        assert not [c for c in calls if "s2_any" in c] and [c for c in calls if "pool" in c or "stack" in c]
    for k in outs[0]:
        assert torch.equal(outs[0][k], outs[1][k]), k


# ---------------------------------------------------------------------------------------------- against the reference
@pytest.fixture(scope="module")
def gold(golden_dir):
    return (np.load(os.path.join(golden_dir, "impala_downsample_golden.npz")),
            json.load(open(os.path.join(golden_dir, "impala_downsample_golden.json"))))


def make_golden_net(meta, tag):
    enc = dict(meta[tag]["encoder_args"])
    if "channels" in enc:
        enc["channels"] = tuple(enc["channels"])
    torch.manual_seed(meta[tag]["seed"])
    return models.DualHeadNet("impala", tuple(meta[tag]["input_dims"]), meta["n_actions"], hidden_units=meta[tag]["hidden_units"],
                              head_scale=meta["head_scale"], head_bias=meta["head_bias"], device="cuda", **enc)


@pytest.mark.parametrize("tag", ["stride", "none"])
def test_forward_matches_reference(gold, tag):
    g, meta = gold
    net = make_golden_net(meta, tag)
    assert list(net.state_dict().keys()) == meta[tag]["param_names"]
    assert net.n_parameters() == sum(int(np.prod(v["shape"])) for v in meta[tag]["params"].values())
    assert list(net.spec.out_shape) == meta[tag]["out_shape"]
    x = torch.from_numpy(g[f"{tag}_fwd_x"]).cuda()
    for _ in range(2):  # the second forward replays the recorded launch plan
        out = net.forward(x, policy_temperature=1.0)
        torch.cuda.synchronize()
        for k in ("raw_policy", "log_policy", "value", "advantage"):
            e = rel_err(out[k], torch.from_numpy(g[f"{tag}_fwd_{k}"]))
            print(f"IMPALA_DS golden forward {tag} {k} rel_err={e:.3e}")
            assert e < 1e-4, (tag, k, e)


@pytest.mark.parametrize("tag", ["stride", "none"])
def test_policy_minibatch_matches_reference_runner(gold, tag):
    g, meta = gold
    assert meta[tag]["relu_margin"] >= 1e-5
    net = make_golden_net(meta, tag)
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
    worst = {}
    for name in meta[tag]["param_names"]:
        if name in meta[tag]["grad_none"]:
            assert float(net.grads[name].abs().max()) == 0.0, name
            continue
        worst[name] = rel_err(net.grads[name], torch.from_numpy(g[f"{tag}_grad_{name}"]))
        bar = 1e-4 if name.startswith("encoder.stacks.") else 1e-5
        print(f"IMPALA_DS golden gradient {tag} {name} rel_err={worst[name]:.3e} bar={bar:.0e}")
    for name, e in worst.items():
        assert e < (1e-4 if name.startswith("encoder.stacks.") else 1e-5), (tag, name, e)


def test_precision_medium_keeps_the_strided_convolutions_exact_and_the_blocks_split():
    """--precision=medium on a (4, 84, 84) 'stride' net: the 32-channel stacks' blocks run as split-bf16 launches behind
    exact-float32 strided convolutions; the forward stays within 1e-4 of float64's largest output."""
    hi, x, ref, _ns, _nb, _mode = case("stride_4x84x84")
    torch.manual_seed(11)
    md = models.DualHeadNet("impala", (4, 84, 84), N_ACTIONS, hidden_units=64, head_scale=0.1, head_bias=True, device="cuda",
                            precision="medium", down_sample="stride")
    md.load_state_dict(hi.state_dict())
    assert md.split_bf16 and md.generic_convs == first_convs(md)
    assert not any(isinstance(k[0], str) for k in md._pk16), "a strided first convolution has a split-bf16 packing"
    calls = recording(md)
    out = md.forward(x)
    torch.cuda.synchronize()
    assert calls.count("ppo_conv3x3s2_any_forward_f32") == 3 and calls.count("ppo_impala_stack_tail_forward_bf16x3") >= 2
    assert not [c for c in calls if "pool" in c]
    # a training pass takes the split backward chains of the blocks and the exact strided gradients of the first convolutions
    del calls[:]
    acts, _o, B, dheads = md._train_forward(x)
    dheads.fill_(1.0 / B)
    md.backward(acts, dheads)
    torch.cuda.synchronize()
    assert torch.isfinite(md.grad).all() and all(float(md.grads[fc + ".weight"].abs().max()) > 0 for fc in first_convs(md))
    assert calls.count("ppo_conv3x3s2_any_backward_weight_f32") == 3 and calls.count("ppo_conv3x3s2_any_backward_data_f32") == 2
    assert len([c for c in calls if c.startswith("ppo_impala_stack_tail_backward") and c.endswith("bf16x3")]) >= 2
    assert not [c for c in calls if "pool" in c]
    print(f"IMPALA_DS medium forward h rel_err={rel_err(out['_acts']['h'], ref['h']):.3e}")
    for key in ("raw_policy", "log_policy", "value", "advantage"):
        e = rel_err(out[key], ref[key])
        print(f"IMPALA_DS medium forward {key} rel_err={e:.3e}")
        assert e <= 1e-4, (key, e)
