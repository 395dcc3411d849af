"""Test helper: the IMPALA policy / value network with batch_norm=True (rl/impala.py:63-76: bn0 / bn1 = nn.BatchNorm2d
with torch's defaults in every residual block) as plain torch ops in any float dtype, for the three `down_sample` modes.
Takes a ``state_dict`` with the reference's key names (relative to policy_net), buffers included.

  forward_train   model.train(): every layer normalises with its batch's statistics; returns the outputs and the updated
                  buffers (running_mean / running_var in the dtype of x, num_batches_tracked + 1), the input dict untouched
  forward_eval    model.eval(): every layer is the affine map of its running statistics
  forward_eval_shared_kinks   forward_eval with every ReLU mask and max-pool selection taken from the HIP path's saved
                  maps, as impala_downsample_torch.forward_shared_kinks: acts 'z0_{si}_{bi}', 'z1_{si}_{bi}', 'idx{si}',
                  'flat', 'h'
"""
import torch
import torch.nn.functional as F

EPS, MOMENTUM = 1e-5, 0.1


def _heads(sd, flat, relu_flat, relu_h):
    h = F.linear(relu_flat(flat), sd["encoder.dense.weight"], sd["encoder.dense.bias"])
    f = relu_h(h)
    raw = F.linear(f, sd["policy_head.weight"], sd.get("policy_head.bias"))
    return {"raw_policy": raw, "log_policy": F.log_softmax(raw, dim=1),
            "value": F.linear(f, sd["value_head.weight"], sd.get("value_head.bias")),
            "advantage": F.linear(f, sd["advantage_head.weight"], sd.get("advantage_head.bias")), "h": h}


def _first(sd, x, si, down_sample, idx=None):
    p = f"encoder.stacks.{si}.firstconv."
    c = F.conv2d(x, sd[p + "weight"], sd[p + "bias"], stride=2 if down_sample == "stride" else 1, padding=1)
    if down_sample != "pool":
        return c
    if idx is None:
        return F.max_pool2d(c, kernel_size=3, stride=2, padding=1)
    idx = idx.long()  # the HIP path's winning taps ky * 3 + kx
    B, C, Ho, Wo = idx.shape
    W = c.shape[3]
    oy = torch.arange(Ho).view(1, 1, Ho, 1)
    ox = torch.arange(Wo).view(1, 1, 1, Wo)
    pos = (2 * oy - 1 + idx // 3) * W + (2 * ox - 1 + idx % 3)
    return c.flatten(2).gather(2, pos.flatten(2)).view(B, C, Ho, Wo)


def _affine(sd, base, x, mean, var):
    bc = (None, slice(None), None, None)
    s = sd[base + ".weight"] / torch.sqrt(var + EPS)
    return x * s[bc] + (sd[base + ".bias"] - mean * s)[bc]


def _bn_train(sd, base, x, new):
    m = x.numel() // x.shape[1]
    mean, var = x.mean(dim=(0, 2, 3)), x.var(dim=(0, 2, 3), unbiased=False)
    new[base + ".running_mean"] = (1 - MOMENTUM) * sd[base + ".running_mean"].to(x.dtype) + MOMENTUM * mean
    new[base + ".running_var"] = (1 - MOMENTUM) * sd[base + ".running_var"].to(x.dtype) + MOMENTUM * var * (m / (m - 1))
    new[base + ".num_batches_tracked"] = sd[base + ".num_batches_tracked"] + 1
    return _affine(sd, base, x, mean, var)


def _bn_eval(sd, base, x):
    return _affine(sd, base, x, sd[base + ".running_mean"].to(x.dtype), sd[base + ".running_var"].to(x.dtype))


def _net(sd, x, n_stacks, n_block, down_sample, bn, relu0, relu1, relu_flat, relu_h, idx):
    for si in range(n_stacks):
        x = _first(sd, x, si, down_sample, idx(si))
        for bi in range(n_block):
            b = f"encoder.stacks.{si}.blocks.{bi}."
            r = F.conv2d(relu0(bn(b + "bn0", x), si, bi), sd[b + "conv0.weight"], sd[b + "conv0.bias"], padding=1)
            r = F.conv2d(relu1(bn(b + "bn1", r), si, bi), sd[b + "conv1.weight"], sd[b + "conv1.bias"], padding=1)
            x = x + r
    return _heads(sd, x.reshape(x.shape[0], -1), relu_flat, relu_h)


def _plain(t, *_):
    return F.relu(t)


def forward_train(sd, x, n_stacks=3, n_block=2, down_sample="pool"):
    """(outputs, updated buffers) of one train-mode forward; x: [B,C,H,W] float (already scaled)."""
    new = {}
    out = _net(sd, x, n_stacks, n_block, down_sample, lambda base, t: _bn_train(sd, base, t, new), _plain, _plain, F.relu,
               F.relu, lambda si: None)
    return out, new


def forward_eval(sd, x, n_stacks=3, n_block=2, down_sample="pool"):
    return _net(sd, x, n_stacks, n_block, down_sample, lambda base, t: _bn_eval(sd, base, t), _plain, _plain, F.relu, F.relu,
                lambda si: None)


def forward_eval_shared_kinks(sd, x, acts, n_stacks=3, n_block=2, down_sample="pool"):
    dt = x.dtype

    def relu_as(t, ref):
        return t * (ref > 0).to(dt)

    return _net(sd, x, n_stacks, n_block, down_sample, lambda base, t: _bn_eval(sd, base, t),
                lambda t, si, bi: relu_as(t, acts[f"z0_{si}_{bi}"]), lambda t, si, bi: relu_as(t, acts[f"z1_{si}_{bi}"]),
                lambda t: relu_as(t, acts["flat"]), lambda t: relu_as(t, acts["h"]),
                lambda si: acts[f"idx{si}"] if down_sample == "pool" else None)
