"""oracle/trained_params.py — TEST INFRASTRUCTURE, NOT PRODUCT.

Every initialiser of ppo_amd/models.py zeroes its bias and log_std starts at zero, so a network built from them cannot
tell a bias that is read from the wrong channel, from the wrong layer, twice or not at all from a correct one.  The helpers
here give the network tests parameters as training leaves them - every bias and log_std non-zero - and the list of
single-tensor bias faults those tests must be able to see.  Plain torch on the CPU; only tests/ imports this module.
"""
import re
import zlib
from collections import OrderedDict

import torch
import torch.nn.functional as F

HEADS = ("policy_head", "value_head", "advantage_head", "tvf_head")
# same-shaped bias tensors a wiring slip could exchange unnoticed: (pattern, replacement) on the parameter name
_SWAPS = ((re.compile(r"^(encoder\.stacks\.\d+\.blocks\.\d+)\.conv0\.bias$"), r"\1.conv1.bias"),   # a block's two convolutions
          (re.compile(r"^encoder\.conv2\.bias$"), "encoder.conv3.bias"),                           # Nature: both 64 channels
          (re.compile(r"^encoder\.fc1\.bias$"), "encoder.fc2.bias"))                               # MLP: both `hidden` wide


def perturbed_state_dict(sd, seed, sigma=0.1):
    """A copy of `sd` (an initialiser's or a net's state_dict) as CPU float32 tensors in which every `*.bias` is drawn
    from N(0, sigma) and `log_std`, where present, from N(0, 0.3); weights stay as they are.  A tensor's draw depends
    on `seed`, its name and its shape only - not on the order of the keys, which differs between the initialisers and
    a net's state_dict.  (A TVF feature mask is the net's business: its load_state_dict re-applies it.)"""
    out = OrderedDict()
    for name, t in sd.items():
        t = torch.as_tensor(t).detach().to("cpu", torch.float32).clone()
        g = torch.Generator().manual_seed(zlib.crc32(f"{int(seed)}:{name}".encode()))
        if name.endswith(".bias"):
            t = torch.randn(t.shape, generator=g) * sigma
        elif name == "log_std":
            t = torch.randn(t.shape, generator=g) * 0.3
        out[name] = t
    return out


def bias_names(sd):
    return [n for n in sd if n.endswith(".bias")]


def single_faults(sd):
    """Yield (label, faulty copy of sd) for every single-tensor bias fault a network test must notice: each bias zeroed
    (a layer that never adds it), each bias of more than one element rotated by one channel (a slipped channel offset),
    and each same-shaped pair exchanged (swapped pointers)."""
    def variant(**changed):
        v = OrderedDict(sd)
        v.update(changed)
        return v

    for name in bias_names(sd):
        yield f"{name} zeroed", variant(**{name: torch.zeros_like(sd[name])})
    for name in bias_names(sd):
        if sd[name].numel() > 1:
            yield f"{name} rotated by one channel", variant(**{name: torch.roll(sd[name], 1)})
    for name in bias_names(sd):
        for pattern, repl in _SWAPS:
            other = pattern.sub(repl, name)
            if other != name and other in sd and sd[other].shape == sd[name].shape:
                yield f"{name} <-> {other}", variant(**{name: sd[other], other: sd[name]})


def nature_forward(sd, x):
    """NatureCNN + heads (rl/models.py:130-145, 467-506) in the dtype of its arguments: x [B, C, H, W] already scaled,
    returns the fused head row [policy | value | advantage (| tvf)]."""
    h = x
    for name, stride in (("conv1", 4), ("conv2", 2), ("conv3", 1)):
        h = F.relu(F.conv2d(h, sd[f"encoder.{name}.weight"], sd[f"encoder.{name}.bias"], stride=stride))
    feat = F.relu(F.linear(h.reshape(h.shape[0], -1), sd["encoder.fc.weight"], sd["encoder.fc.bias"]))
    return torch.cat([F.linear(feat, sd[f"{n}.weight"], sd.get(f"{n}.bias")) for n in HEADS if f"{n}.weight" in sd], dim=1)


def head_row(out):
    """[raw_policy | value | advantage (| tvf)] from the result dict of oracle.model_torch.forward / mlp_forward."""
    cols = [out["raw_policy"], out["value"], out["advantage"]]
    if "tvf_value" in out:
        cols.append(out["tvf_value"].reshape(out["value"].shape[0], -1))
    return torch.cat(cols, dim=1)


def as_double(sd, requires_grad=False):
    return OrderedDict((k, torch.as_tensor(v).detach().cpu().double().requires_grad_(requires_grad)) for k, v in sd.items())
