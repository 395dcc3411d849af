"""GPU: the IMPALA encoder at observation shapes, channel lists and block counts the specialised 3x3 kernels have no
instantiation for - every such convolution on the generic kernels (csrc/conv3x3_any.hip) - against float64 torch
(oracle/model_torch.py) on the same parameters and inputs.  Biases and log_std are non-zero
(oracle/trained_params.perturbed_state_dict; tests/test_bias_sensitivity_cpu.py says why that matters).

Bars, the project's own: forward rows and encoder.stacks.* gradients within 1e-4 of the reference tensor's max, dense and
head gradients within 1e-5 (tests/test_model_gpu.py).  Gradients are compared with every ReLU mask and max-pool
selection taken from the net's own saved activations (oracle.model_torch.forward_shared_kinks), so no element is left
out.  float32 torch alone sits at 1.3e-6 or better on these forwards, so the float64 reference is far inside the bar.
"""
import functools

import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from oracle import model_torch as R  # noqa: E402
from oracle import trained_params as T  # noqa: E402
from ppo_amd import models  # noqa: E402

N_ACTIONS = 6
# name -> (input dims, batch, encoder arguments)
CASES = {
    "3x20x28": ((3, 20, 28), 5, {}),
    "12x33x31": ((12, 33, 31), 3, {}),
    "1x9x9": ((1, 9, 9), 7, {}),
    "2x5x6": ((2, 5, 6), 4, {}),            # the last map is 1x1
    "4x96x96": ((4, 96, 96), 2, {}),        # --env_resolution=muzero
    "12x84x84": ((12, 84, 84), 2, {}),      # Atari RGB: only the first convolution is generic
    "3x20x28_c8_24_b1": ((3, 20, 28), 5, {"channels": (8, 24), "n_block": 1}),
}


def conv_names(channels, n_block):
    return [n for si in range(len(channels)) for n in
            [f"encoder.stacks.{si}.firstconv"] + [f"encoder.stacks.{si}.blocks.{bi}.conv{ci}" for bi in range(n_block) for ci in range(2)]]


@functools.lru_cache(maxsize=None)
def case(name):
    """The net of one case (biases and log_std non-zero), its uint8 input and its float64 forward, built once."""
    dims, B, enc = CASES[name]
    torch.manual_seed(11)
    net = models.DualHeadNet("impala", dims, N_ACTIONS, hidden_units=64, head_scale=0.1, head_bias=True, device="cuda", **enc)
    net.load_state_dict(T.perturbed_state_dict(net.state_dict(), seed=21))
    g = torch.Generator(device="cpu").manual_seed(5)
    x = torch.randint(0, 256, (B, *dims), generator=g, dtype=torch.uint8)
    n_stacks, n_block = len(net.spec.channels), net.spec.n_block
    with torch.no_grad():
        ref = R.forward(T.as_double(net.state_dict()), x.double() / 255.0, n_stacks=n_stacks, n_block=n_block)
    return net, x.cuda(), ref, n_stacks, n_block


def rel_err(got, ref):
    return (got.detach().cpu().double() - ref.detach().cpu().double()).abs().max().item() / max(ref.abs().max().item(), 1e-30)


@pytest.mark.parametrize("name", list(CASES))
def test_generic_convs_lists_the_layers_without_a_specialised_kernel(name):
    net, x, _ref, _ns, _nb = case(name)
    if name == "12x84x84":
        assert net.generic_convs == ["encoder.stacks.0.firstconv"]
    else:
        assert net.generic_convs == conv_names(net.spec.channels, net.spec.n_block)
    assert net.takes_obs_index(x) is False
    index = torch.arange(x.shape[0], dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError):
        net._train_forward(x, index, obs_indexed=True)


def test_the_shapes_that_ran_before_keep_every_specialised_launch():
    for dims in ((4, 84, 84), (5, 84, 84), (3, 64, 64), (4, 64, 64)):
        net = models.DualHeadNet("impala", dims, N_ACTIONS, hidden_units=64, head_scale=0.1, head_bias=True, device="cuda")
        assert net.generic_convs == []
        assert net.takes_obs_index(torch.zeros((1, *dims), dtype=torch.uint8, device="cuda"))


@pytest.mark.parametrize("name", list(CASES))
def test_forward_against_float64(name):
    net, x, ref, _ns, _nb = case(name)
    out = net.forward(x)
    for key, got in (("raw_policy", out["raw_policy"]), ("value", out["value"]), ("h", out["_acts"]["h"])):
        e = rel_err(got, ref[key])
        print(f"IMPALA_ANY forward {name} {key} rel_err={e:.3e}")
        assert e < 1e-4, (name, key, e)


@pytest.mark.parametrize("name", list(CASES))
def test_inference_plan_and_training_forward_agree_bitwise(name):
    net, x, _ref, _ns, _nb = case(name)
    first = net.forward(x)["_acts"]["h"].clone()        # records the launch plan (or replays an earlier test's)
    replay = net.forward(x)["_acts"]["h"].clone()       # replays it
    assert any(k[1] == x.shape[0] for k in net._plans), "no launch plan was recorded for this batch"
    acts, _o, _B, _dheads = net._train_forward(x)
    assert torch.equal(first, replay) and torch.equal(first, acts["h"])


@pytest.mark.parametrize("name", list(CASES))
def test_gradients_against_float64_with_shared_kinks(name):
    net, x, _ref, n_stacks, n_block = case(name)
    B = x.shape[0]
    g = torch.Generator(device="cpu").manual_seed(17)
    actions = torch.randint(0, N_ACTIONS, (B,), generator=g, dtype=torch.int32).cuda()
    old_log_pac = (torch.randn(B, generator=g) * 0.1 - 1.7).cuda()
    old_log_policy = torch.log_softmax(torch.randn(B, N_ACTIONS, generator=g), dim=1).cuda()
    adv = torch.randn(B, generator=g).cuda()
    # Returns well away from the values (|V| < 1 with these heads), all on one side: value_head.bias is ONE number whose
    # gradient is sum_b (V_b - R_b) / B, and "1e-5 of the tensor's max" is then the relative error of that sum.  With
    # returns straddling the values its terms cancel, and the float32 rounding of V itself (6e-8 of |V|, whoever
    # computes it) divided by what is left of the sum is no statement about any kernel.
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
    out = R.forward_shared_kinks(sd, x.double() / 255.0, acts, n_stacks=n_stacks, n_block=n_block)
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
        assert e < bar, (name, pname, e)
    print(f"IMPALA_ANY gradients {name} worst rel_err={max(worst.values()):.3e} at {max(worst, key=worst.get)}")


@pytest.mark.parametrize("name", ["4x96x96", "12x84x84"])
def test_ppo_minibatch_on_the_gathered_rows_runs_and_steps(name):
    """The whole minibatch call the Runner makes when takes_obs_index is False: gathered observations, per-sample arrays
    read through the index; then the optimiser step, after which the next forward sees the new weights."""
    dims, B, enc = CASES[name]
    torch.manual_seed(3)
    net = models.DualHeadNet("impala", dims, N_ACTIONS, hidden_units=64, head_scale=0.1, head_bias=True, device="cuda", **enc)
    g = torch.Generator(device="cpu").manual_seed(23)
    whole = 3 * B
    x = torch.randint(0, 256, (B, *dims), generator=g, dtype=torch.uint8).cuda()
    index = torch.randperm(whole, generator=g)[:B].int().cuda()
    actions = torch.randint(0, N_ACTIONS, (whole,), generator=g, dtype=torch.int32).cuda()
    old_log_policy = torch.log_softmax(torch.randn(whole, N_ACTIONS, generator=g), dim=1).cuda()
    old_log_pac = old_log_policy.gather(1, actions.long()[:, None])[:, 0].contiguous()
    adv, ret = torch.randn(whole, generator=g).cuda(), torch.randn(whole, 1, generator=g).cuda()
    before = net.forward(x)["raw_policy"].clone()
    stats = net.ppo_minibatch(x, actions, old_log_pac, old_log_policy, adv, ret, index=index, obs_indexed=False)
    assert torch.isfinite(stats).all()
    flat = net.flat.clone()
    net.adam_step()
    for pname in net.generic_convs:
        o, shape = net._offsets[pname + ".weight"]
        assert not torch.equal(net.flat[o:o + 9 * shape[0] * shape[1]], flat[o:o + 9 * shape[0] * shape[1]]), pname
    after = net.forward(x)["raw_policy"]
    assert torch.isfinite(after).all() and not torch.equal(before, after)
