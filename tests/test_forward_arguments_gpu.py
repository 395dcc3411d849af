"""GPU: the per-call inputs of DualHeadNet.encode are arguments - `index`, `tail`, `chain_split` - and what became of the
tail comes back as acts["tail_taken"].  The kernels behind the tail have their own tests (tests/test_nn_ops_gpu.py); here
the host side: the tail reaches the dense + heads launch when the call records its launch list and when it replays it,
each replay with the tail of its own call; a net without that launch hands the tail back untouched; nothing stays on
the net between calls.  Everything is compared bit for bit with the separate launches on the same net.
"""
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from oracle import trained_params as T  # noqa: E402
from ppo_amd import models  # noqa: E402

N_ACTIONS, B, SEED = 6, 5, 0x9E3779B97F4A7C15
# name -> (encoder, input dims, arguments, "has the dense + heads launch")
NETS = {
    "impala-relu": ("impala", (3, 20, 28), dict(channels=(8, 24), n_block=1), True),  # the smallest net that has it
    "impala-tanh": ("impala", (3, 20, 28), dict(channels=(8, 24), n_block=1, activation_fn="tanh"), False),
    "mlp-tanh": ("mlp", (11,), dict(activation_fn="tanh"), False),  # _encode_mlp never takes a tail
}
GONE = ("obs_index", "loss_tail", "act_tail", "allow_chain_split")


def make(name):
    """A fresh net (no recorded launch list yet) with non-zero biases, and its input."""
    encoder, dims, kw, fused = NETS[name]
    torch.manual_seed(11)
    net = models.DualHeadNet(encoder, dims, N_ACTIONS, hidden_units=64, head_scale=0.1, head_bias=True, device="cuda", **kw)
    net.load_state_dict(T.perturbed_state_dict(net.state_dict(), seed=21))
    g = torch.Generator(device="cpu").manual_seed(5)
    if encoder == "mlp":
        x = torch.randn((B, *dims), generator=g)
    else:
        x = torch.randint(0, 256, (B, *dims), generator=g, dtype=torch.uint8)
    return net, x.cuda(), fused


class ActionRows:
    """Output buffers of one action step (log_policy, actions, log_pac, raw_policy, values), filled with a value no
    launch writes."""

    def __init__(self, vh):
        f = dict(dtype=torch.float32, device="cuda")
        self.vh = vh
        self.bufs = [torch.full((B, N_ACTIONS), 123.0, **f), torch.full((B,), -1, dtype=torch.int32, device="cuda"),
                     torch.full((B,), 123.0, **f), torch.full((B, N_ACTIONS), 123.0, **f), torch.full((B, vh), 123.0, **f)]
        self.fresh = [t.clone() for t in self.bufs]

    def tail(self, counter):
        return (N_ACTIONS, 1.0, SEED, counter, *[t.data_ptr() for t in self.bufs], self.vh)

    def untouched(self):
        return all(torch.equal(a, b) for a, b in zip(self.bufs, self.fresh))

    def act(self, net, row, counter):
        """The action step as a launch of its own on the head rows `row`."""
        net._call("ppo_policy_act_f32", row.data_ptr(), B, net.nh, N_ACTIONS, 1.0, None, SEED, counter, 0,
                  *[t.data_ptr() for t in self.bufs], self.vh)


@pytest.mark.parametrize("name", list(NETS))
def test_inference_tail_rides_on_the_recorded_and_the_replayed_launch(name):
    net, x, fused = make(name)
    assert not net._plans
    for k, counter in enumerate((0, 1000, 3 * 2**40 + 7)):  # the first call records the launch list, the others replay it
        got = ActionRows(net.vh)
        acts = net.encode(x, False, tail=got.tail(counter))
        row = net.heads(acts, "i").clone()
        assert acts["tail_taken"] is fused
        assert len(net._plans) == 1
        if not fused:
            torch.cuda.synchronize()
            assert got.untouched()  # the tail came back: its caller launches the action step, as Runner._policy_step does
            got.act(net, row, counter)
        # a call without a tail directly after one with a tail: nothing carries over
        plain = net.encode(x, False)
        assert plain["tail_taken"] is False
        ref = ActionRows(net.vh)
        ref_row = net.heads(plain, "i")
        ref.act(net, ref_row, counter)
        torch.cuda.synchronize()
        assert torch.equal(row, ref_row), (name, k)
        assert not ref.untouched()
        for what, a, b in zip(("log_policy", "actions", "log_pac", "raw_policy", "values"), got.bufs, ref.bufs):
            assert torch.equal(a, b), (name, k, what)
    assert not [a for a in GONE if hasattr(net, a)]


@pytest.mark.parametrize("name", ["impala-relu", "impala-tanh"])
def test_ppo_minibatch_is_the_training_forward_the_loss_and_the_backward(name):
    """With the loss inside the dense + heads launch (relu) and as a launch of its own (tanh): statistics and gradient
    of ppo_minibatch against _train_forward + ppo_ppo_loss_f32 + backward."""
    net, x, fused = make(name)
    g = torch.Generator(device="cpu").manual_seed(17)
    actions = torch.randint(0, N_ACTIONS, (B,), generator=g, dtype=torch.int32).cuda()
    old_log_pac = (torch.randn(B, generator=g) * 0.1 - 1.7).cuda()
    old_log_policy = torch.log_softmax(torch.randn(B, N_ACTIONS, generator=g), dim=1).cuda()
    adv, ret = torch.randn(B, generator=g).cuda(), (torch.randn(B, 1, generator=g) * 0.3 + 3.0).cuda()
    calls, orig = [], net._call
    net._call = lambda fn, *a: (calls.append(fn), orig(fn, *a))[1]
    net.grad.zero_()
    stats_m = net.ppo_minibatch(x, actions, old_log_pac, old_log_policy, adv, ret).clone()
    grad_m = net.grad.clone()
    net._call = orig
    assert ("ppo_dense_heads_loss_forward_f32" in calls) == fused and ("ppo_ppo_loss_f32" in calls) == (not fused)
    net.grad.zero_()
    acts, o, B_, dheads = net._train_forward(x)
    assert B_ == B and acts["tail_taken"] is False
    stats = net._buf("loss_stats", (B, 8))
    stats.zero_()
    net._call("ppo_ppo_loss_f32", o.data_ptr(), B, net.nh, net.n_actions, net.vh, actions.data_ptr(), old_log_pac.data_ptr(),
              old_log_policy.data_ptr(), adv.data_ptr(), ret.data_ptr(), 0.2, 0.01, 0.5, 1.0 / B, dheads.data_ptr(),
              stats.data_ptr(), None)
    net.backward(acts, dheads)
    torch.cuda.synchronize()
    assert torch.isfinite(stats_m).all() and float(grad_m.abs().max()) > 0
    assert torch.equal(stats_m, stats) and torch.equal(grad_m, net.grad)
    assert not [a for a in GONE if hasattr(net, a)]


@pytest.mark.parametrize("name", ["impala-relu", "mlp-tanh"])
def test_an_index_that_cannot_be_honoured_raises(name):
    net, x, _fused = make(name)
    idx = torch.arange(B, dtype=torch.int32, device="cuda")
    assert net.takes_obs_index(x) is False  # (generic first convolution; float32 features)
    with pytest.raises(ValueError):
        net.encode(x, False, index=idx)
    with pytest.raises(ValueError):
        net.encode(x, True, index=idx)
