"""CPU: the host side of Random Network Distillation.

tests/golden/rnd_golden.json (tests/golden/make_rnd_golden.py) holds the sha256 of every initial parameter of the
reference's prediction_net / target_net inside TVFModel(encoder="nature", single, (4, 36, 36), hidden 64, use_rnd=True,
value_head_names=("ext", "int")) under torch.manual_seed(seed).  ppo_amd.models draws policy_net first
(init_parameters) and then init_rnd_parameters - the order of TVFModel's constructor (rl/models.py:605-622) - and must
arrive at the same tensors under the same names.  The policy net's orthogonal initialiser is a LAPACK QR factorisation,
so - as in tests/test_nature_init.py - the draws are made in a child process with MKL pinned the way the fixture's were.
The argument checks of TVFModel(use_rnd=True) come before any device is touched, so they run here too."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_CHILD = r'''
import hashlib, json, sys
sys.path.insert(0, sys.argv[2])
import numpy as np
import torch
from ppo_amd import models

job = json.loads(sys.argv[1])
torch.manual_seed(job["seed"])
spec = models.NatureSpec(tuple(job["input_dims"]), hidden_units=job["hidden"])
models.init_parameters(spec, job["n_actions"], 2, job["head_scale"], job["head_bias"])  # policy_net, heads ("ext", "int")
pred, target = models.init_rnd_parameters(tuple(job["input_dims"]))
print(json.dumps({net: [[n, list(t.shape), hashlib.sha256(np.ascontiguousarray(t.numpy()).tobytes()).hexdigest()]
                        for n, t in init.items()] for net, init in (("prediction_net", pred), ("target_net", target))}))
'''


@pytest.fixture(scope="module")
def meta(golden_dir):
    return json.load(open(os.path.join(golden_dir, "rnd_golden.json")))


def test_initial_parameters_match_the_reference(meta):
    job = {"seed": meta["seed"], "input_dims": meta["input_dims"], "hidden": meta["hidden_units"],
           "n_actions": meta["n_actions"], "head_scale": meta["head_scale"], "head_bias": meta["head_bias"]}
    r = subprocess.run([sys.executable, "-c", _CHILD, json.dumps(job), ROOT], env=dict(os.environ, **meta["mkl_env"]),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    for net in ("prediction_net", "target_net"):
        assert [n for n, _s, _h in got[net]] == meta["param_names"][net]
        for name, shape, sha in got[net]:
            assert shape == meta["params"][net][name]["shape"], (net, name)
            assert sha == meta["params"][net][name]["sha256"], (net, name)
    # RNDPredictor(single_channel_input_dims) keeps its default hidden_units whatever the model's (rl/models.py:621-622)
    assert meta["params"]["prediction_net"]["out.weight"]["shape"] == [512, 512]
    assert meta["params"]["target_net"]["out.weight"]["shape"] == [512, 64]
    assert meta["params"]["prediction_net"]["conv1.weight"]["shape"] == [32, 1, 8, 8]


def test_biases_start_at_zero_and_weights_are_scaled():
    import numpy as np
    import torch
    from ppo_amd import models
    torch.manual_seed(0)
    plain = [torch.nn.Conv2d(1, 32, kernel_size=(8, 8), stride=(4, 4)).weight.data.clone()]
    torch.manual_seed(0)
    pred, target = models.init_rnd_parameters((4, 36, 36))
    assert torch.equal(pred["conv1.weight"], plain[0] * (np.sqrt(2) * 1.3))
    for init in (pred, target):
        for name, t in init.items():
            if name.endswith(".bias"):
                assert not t.any(), name
    assert list(target) == [f"{m}.{p}" for m in ("conv1", "conv2", "conv3", "out") for p in ("weight", "bias")]


def test_constructor_checks_are_the_references():
    from ppo_amd import models
    kw = dict(encoder="nature", input_dims=(4, 36, 36), actions=6, architecture="single", hidden_units=64, use_rnd=True)
    with pytest.raises(AssertionError, match="RND requires int value head."):
        models.TVFModel(observation_normalization=True, value_head_names=("ext",), **kw)
    with pytest.raises(AssertionError, match="rnd requires observation normalization."):
        models.TVFModel(observation_normalization=False, value_head_names=("ext", "int"), **kw)
    with pytest.raises(NotImplementedError, match="TVF"):
        models.TVFModel(observation_normalization=True, value_head_names=("ext", "int"), tvf_fixed_head_horizons=[1, 10],
                        tvf_fixed_head_weights=[1.0, 1.0], **kw)


def test_rnd_geometry_rejects_small_images():
    from ppo_amd import rnd
    layers, flat = rnd.rnd_geometry((4, 84, 84))
    assert [(l[1], l[2], l[7], l[8]) for l in layers] == [(1, 32, 20, 20), (32, 64, 9, 9), (64, 64, 7, 7)] and flat == 3136
    assert rnd.rnd_geometry((4, 36, 36))[1] == 64
    with pytest.raises(ValueError, match="too small"):
        rnd.rnd_geometry((4, 35, 36))
