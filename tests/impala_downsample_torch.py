"""Test helper: the IMPALA policy / value network of oracle/model_torch.py for the three `down_sample` modes
(rl/impala.py:96, 102-108) as plain torch ops in any float dtype - 'pool' is oracle.model_torch's own, 'stride' has the
first convolution of every stack at stride 2 and no max-pool, 'none' has it at stride 1 and no max-pool.  Takes a
``state_dict`` with the reference's key names (relative to policy_net)."""
import torch
import torch.nn.functional as F

from oracle import model_torch as R


def _heads(sd, flat, relu_flat, relu_h):
    h = F.linear(relu_flat(flat), sd["encoder.dense.weight"], sd["encoder.dense.bias"])
    f = relu_h(h)
    raw = F.linear(f, sd["policy_head.weight"], sd.get("policy_head.bias"))
    return {"raw_policy": raw, "log_policy": F.log_softmax(raw, dim=1),
            "value": F.linear(f, sd["value_head.weight"], sd.get("value_head.bias")),
            "advantage": F.linear(f, sd["advantage_head.weight"], sd.get("advantage_head.bias")), "h": h}


def _first_conv(sd, x, si, down_sample):
    p = f"encoder.stacks.{si}.firstconv."
    return F.conv2d(x, sd[p + "weight"], sd[p + "bias"], stride=2 if down_sample == "stride" else 1, padding=1)


def forward(sd, x, n_stacks=3, n_block=2, down_sample="pool"):
    """x: [B,C,H,W] float (already scaled).  Returns dict(raw_policy, log_policy, value, advantage, h)."""
    if down_sample == "pool":
        return R.forward(sd, x, n_stacks=n_stacks, n_block=n_block)
    assert down_sample in ("stride", "none")
    for si in range(n_stacks):
        x = _first_conv(sd, x, si, down_sample)
        for bi in range(n_block):
            b = f"encoder.stacks.{si}.blocks.{bi}."
            r = F.conv2d(F.relu(x), sd[b + "conv0.weight"], sd[b + "conv0.bias"], padding=1)
            r = F.conv2d(F.relu(r), sd[b + "conv1.weight"], sd[b + "conv1.bias"], padding=1)
            x = x + r
    return _heads(sd, x.reshape(x.shape[0], -1), F.relu, F.relu)


def forward_shared_kinks(sd, x, acts, n_stacks=3, n_block=2, down_sample="pool"):
    """Same network, but every ReLU mask is taken from `acts` (the HIP path's own saved pre-activations) instead of being
    re-decided, as oracle.model_torch.forward_shared_kinks does: in float64 this is the exact gradient of the function
    the HIP path evaluated.  Without a max-pool ReLU is the only kink.  acts: 'q{si}_{bi}_in', 'a{si}_{bi}', 'flat', 'h'."""
    if down_sample == "pool":
        return R.forward_shared_kinks(sd, x, acts, n_stacks=n_stacks, n_block=n_block)
    assert down_sample in ("stride", "none")
    dt = x.dtype

    def relu_as(t, ref):
        return t * (ref > 0).to(dt)

    for si in range(n_stacks):
        x = _first_conv(sd, x, si, down_sample)
        for bi in range(n_block):
            b = f"encoder.stacks.{si}.blocks.{bi}."
            r = F.conv2d(relu_as(x, acts[f"q{si}_{bi}_in"]), sd[b + "conv0.weight"], sd[b + "conv0.bias"], padding=1)
            r = F.conv2d(relu_as(r, acts[f"a{si}_{bi}"]), sd[b + "conv1.weight"], sd[b + "conv1.bias"], padding=1)
            x = x + r
    return _heads(sd, x.reshape(x.shape[0], -1), lambda t: relu_as(t, acts["flat"]), lambda t: relu_as(t, acts["h"]))
