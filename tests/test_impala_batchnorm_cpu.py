"""CPU: the batch-norm IMPALA net (rl/impala.py:63-76) without a GPU - the plain-torch helper
(tests/impala_batchnorm_torch.py) against the reference's own outputs, buffers and gradients
(tests/golden/impala_batchnorm_golden.npz, make_impala_batchnorm_golden.py), the initial parameters, key order and
optimiser order of ppo_amd.models against the same fixture, and the bars of the GPU tests shown reachable in float32.

Bars, the project's own (tests/test_impala_downsample_gpu.py): forward rows, buffers and encoder.stacks.* gradients within
1e-4 of the reference tensor's maximum, dense and head gradients within 1e-5."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import impala_batchnorm_torch as BN  # noqa: E402
from conftest import GOLDEN  # noqa: E402
from oracle import model_torch as R  # noqa: E402
from ppo_amd import models  # noqa: E402

TAGS = ["pool", "stride"]
HEADS = ("raw_policy", "log_policy", "value", "advantage")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CHILD = r'''
import hashlib, json, sys
sys.path.insert(0, sys.argv[2])
import numpy as np
import torch
from ppo_amd import models

job = json.loads(sys.argv[1])
args = {k: (tuple(v) if isinstance(v, list) else v) for k, v in job["encoder_args"].items() if k != "batch_norm"}
torch.manual_seed(job["seed"])
spec = models.ImpalaSpec(tuple(job["input_dims"]), hidden_units=job["hidden"], **args)
init = models.init_parameters(spec, job["n_actions"], 1, job["head_scale"], job["head_bias"], batch_norm=True)
print(json.dumps([[n, list(t.shape), hashlib.sha256(np.ascontiguousarray(t.numpy()).tobytes()).hexdigest()]
                  for n, t in init.items()]))
'''


@functools.lru_cache(maxsize=None)
def gold():
    return (np.load(os.path.join(GOLDEN, "impala_batchnorm_golden.npz")),
            json.load(open(os.path.join(GOLDEN, "impala_batchnorm_golden.json"))))


def spec_of(meta, tag):
    enc = {k: (tuple(v) if isinstance(v, list) else v) for k, v in meta[tag]["encoder_args"].items() if k != "batch_norm"}
    return models.ImpalaSpec(tuple(meta[tag]["input_dims"]), hidden_units=meta[tag]["hidden_units"], **enc)


@functools.lru_cache(maxsize=None)
def initial(tag):
    """init_parameters of the set's seed, and the spec."""
    g, meta = gold()
    sp = spec_of(meta, tag)
    torch.manual_seed(meta[tag]["seed"])
    return models.init_parameters(sp, meta["n_actions"], 1, meta["head_scale"], meta["head_bias"], batch_norm=True), sp


def fixture_state(tag, dtype):
    """The state dict the fixture's forwards start from: initial parameters, the recorded gamma / beta, fresh buffers."""
    g, meta = gold()
    init, sp = initial(tag)
    sd = {k: v.clone().to(dtype) for k, v in init.items()}
    for name in meta[tag]["bn_layers"]:
        c = sd[name + ".weight"].numel()
        sd[name + ".weight"] = torch.from_numpy(g[f"{tag}_bn_{name}.weight"]).to(dtype)
        sd[name + ".bias"] = torch.from_numpy(g[f"{tag}_bn_{name}.bias"]).to(dtype)
        sd[name + ".running_mean"], sd[name + ".running_var"] = torch.zeros(c, dtype=dtype), torch.ones(c, dtype=dtype)
        sd[name + ".num_batches_tracked"] = torch.zeros((), dtype=torch.int64)
    return sd, dict(n_stacks=len(sp.channels), n_block=sp.n_block, down_sample=sp.down_sample)


def rel_err(got, ref):
    got, ref = torch.as_tensor(got).detach().double(), torch.as_tensor(ref).detach().double()
    return (got - ref.reshape(got.shape)).abs().max().item() / max(ref.abs().max().item(), 1e-30)


@functools.lru_cache(maxsize=None)
def replay(tag, dtype):
    """The fixture's sequence through the helper in `dtype`: ([(outputs, buffers) of the three train-mode forwards], the
    eval-mode forward, the minibatch's gradients by autograd)."""
    g, meta = gold()
    sd, geom = fixture_state(tag, dtype)
    steps = []
    with torch.no_grad():
        for k in range(meta["n_train_forwards"]):
            x = torch.from_numpy(g[f"{tag}_train{k}_x"]).to(dtype) / 255.0
            out, new = BN.forward_train(sd, x, **geom)
            sd.update(new)
            steps.append((out, dict(new)))
        fwd = BN.forward_eval(sd, torch.from_numpy(g[f"{tag}_fwd_x"]).to(dtype) / 255.0, **geom)
    leaf = {k: (v.clone().requires_grad_(True) if v.is_floating_point() and not models.is_bn_buffer(k) else v) for k, v in sd.items()}
    out = BN.forward_eval(leaf, torch.from_numpy(g[f"{tag}_mb_prev_state"]).to(dtype) / 255.0, **geom)
    loss = R.ppo_loss(out, torch.from_numpy(g[f"{tag}_mb_actions"]), torch.from_numpy(g[f"{tag}_mb_log_pac"]).to(dtype),
                      torch.from_numpy(g[f"{tag}_mb_advantages"]).to(dtype), torch.from_numpy(g[f"{tag}_mb_returns"]).to(dtype),
                      eps=meta["ppo_epsilon"], ent_coef=meta["entropy_bonus"], vf_coef=meta["ppo_vf_coef"])
    loss.backward()
    return steps, fwd, {k: v.grad for k, v in leaf.items() if v.is_floating_point() and v.requires_grad}, float(loss.detach())


def bar(name):
    return 1e-4 if name.startswith("encoder.stacks.") else 1e-5


@pytest.mark.parametrize("tag", TAGS)
def test_float64_helper_reproduces_the_reference(tag):
    g, meta = gold()
    assert meta[tag]["relu_margin"] >= 1e-5 and (meta[tag]["pool_margin"] is None or meta[tag]["pool_margin"] >= 1e-5)
    steps, fwd, grads, loss = replay(tag, torch.float64)
    for k, (out, new) in enumerate(steps):
        for key in HEADS:
            assert rel_err(out[key], g[f"{tag}_train{k}_{key}"]) < 1e-4, (k, key)
        for name, t in new.items():
            ref = g[f"{tag}_train{k}_buf_{name}"]
            if name.endswith("num_batches_tracked"):
                assert int(t) == int(ref) == k + 1
            else:
                assert rel_err(t, ref) < 1e-4, (k, name)
    for key in HEADS:
        assert rel_err(fwd[key], g[f"{tag}_fwd_{key}"]) < 1e-4, key
    assert abs(loss - g[f"{tag}_mb_result"][0]) < 1e-4 * max(1.0, abs(g[f"{tag}_mb_result"][0]))
    assert any(".bn0.weight" in n for n in grads) and any(".bn1.bias" in n for n in grads)
    for name in meta[tag]["param_names"]:
        if name in meta[tag]["grad_none"]:
            assert grads[name] is None or float(grads[name].abs().max()) == 0.0, name
            continue
        e = rel_err(grads[name], g[f"{tag}_grad_{name}"])
        assert e < bar(name), (name, e)


@pytest.mark.parametrize("tag", TAGS)
def test_float32_helper_stays_inside_the_bars(tag):
    """The GPU tests hold float32 HIP arithmetic to these bars against float64; plain float32 torch meets them."""
    (s64, f64, g64, _l), (s32, f32, g32, _m) = replay(tag, torch.float64), replay(tag, torch.float32)
    for (o64, b64), (o32, b32) in zip(s64, s32):
        for key in HEADS + ("h",):
            assert rel_err(o32[key], o64[key]) < 1e-4, key
        for name in b64:
            assert rel_err(b32[name].double(), b64[name].double()) < 1e-4, name
    for key in HEADS + ("h",):
        assert rel_err(f32[key], f64[key]) < 1e-4, key
    for name, ref in g64.items():
        if ref is not None:
            assert rel_err(g32[name], ref) < bar(name), name


@pytest.mark.parametrize("tag", TAGS)
def test_initial_parameters_key_order_and_hashes(tag):
    g, meta = gold()
    init, _sp = initial(tag)
    assert models.state_dict_names(init.keys(), True) == meta[tag]["state_dict_keys"]
    # the hashes are of a host with MKL's LAPACK pinned (the heads' orthogonal initialiser is a QR factorisation): a child
    r = subprocess.run([sys.executable, "-c", _CHILD, json.dumps({"seed": meta[tag]["seed"], "input_dims": meta[tag]["input_dims"],
                        "hidden": meta[tag]["hidden_units"], "encoder_args": meta[tag]["encoder_args"], "n_actions": meta["n_actions"],
                        "head_scale": meta["head_scale"], "head_bias": meta["head_bias"]}), ROOT],
                       env=dict(os.environ, **meta["mkl_env"]), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    pinned = json.loads(r.stdout.strip().splitlines()[-1])
    assert [n for n, _s, _h in pinned] == list(init) and len(pinned) == len(meta[tag]["params"])
    for name, shape, sha in pinned:
        assert shape == meta[tag]["params"][name]["shape"], name
        assert sha == meta[tag]["params"][name]["sha256"], name
    for name in meta[tag]["bn_layers"]:
        assert bool((init[name + ".weight"] == 1).all()) and bool((init[name + ".bias"] == 0).all())
    # batch norm draws nothing: every other tensor is what the same seed gives without it
    torch.manual_seed(meta[tag]["seed"])
    plain = models.init_parameters(spec_of(meta, tag), meta["n_actions"], 1, meta["head_scale"], meta["head_bias"])
    assert [n for n in init if ".bn" not in n] == list(plain)
    assert all(torch.equal(init[n], t) for n, t in plain.items())


@pytest.mark.parametrize("tag", TAGS)
def test_adam_parameter_order_is_named_parameters(tag):
    _g, meta = gold()
    init, _sp = initial(tag)
    order = [n for n in models.state_dict_names(init.keys(), True) if not models.is_bn_buffer(n)]
    assert order == meta[tag]["param_names"]
    block = [n for n in order if n.startswith("encoder.stacks.0.blocks.0.")]
    assert [n.split(".")[-2] for n in block[::2]] == ["conv0", "conv1", "bn0", "bn1"]


def test_impala_spec_still_refuses_the_argument():
    with pytest.raises(NotImplementedError, match="batch_norm") as e:
        models.ImpalaSpec((4, 84, 84), batch_norm=True)
    assert "no HIP path" not in str(e.value)
    assert models.ImpalaSpec((4, 84, 84), batch_norm=False).flat == 32 * 11 * 11
