"""CPU: the initialiser of the Nature encoder reproduces the reference's initial weights bit for bit.

tests/golden/nature_golden.json (tests/golden/make_nature_golden.py) holds the sha256 of every parameter of the
reference's TVFModel(encoder="nature", single) built under torch.manual_seed(seed), at (4, 84, 84) / hidden 512 and at
(4, 36, 36) / hidden 64; ppo_amd.models.init_parameters(NatureSpec(...)) must draw the same values from the same seed,
under the same names and in the same order (rl/models.py:114-125 CustomConv2d x 3 + CustomLinear, :364-368 heads;
rl/tensor_utilities.py:69-94).  The orthogonal initialiser is a LAPACK QR factorisation, so - as in
tests/test_model_init.py - the draws are made in a child process with MKL pinned the way the fixture's were."""
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

out = []
for job in json.loads(sys.argv[1]):
    torch.manual_seed(job["seed"])
    spec = models.NatureSpec(tuple(job["input_dims"]), hidden_units=job["hidden"])
    init = models.init_parameters(spec, job["n_actions"], 1, job["head_scale"], job["head_bias"])
    out.append({"kind": spec.kind, "out_shape": list(spec.out_shape), "flat": spec.flat,
                "params": [[n, list(t.shape), hashlib.sha256(np.ascontiguousarray(t.numpy()).tobytes()).hexdigest()]
                           for n, t in init.items()]})
print(json.dumps(out))
'''


@pytest.fixture(scope="module")
def drawn(golden_dir):
    meta = json.load(open(os.path.join(golden_dir, "nature_golden.json")))
    jobs = [{"seed": meta[tag]["seed"], "input_dims": meta[tag]["input_dims"], "hidden": meta[tag]["hidden_units"],
             "n_actions": meta["n_actions"], "head_scale": meta["head_scale"], "head_bias": meta["head_bias"]}
            for tag in ("full", "small")]
    r = subprocess.run([sys.executable, "-c", _CHILD, json.dumps(jobs), ROOT], env=dict(os.environ, **meta["mkl_env"]),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    return meta, dict(zip(("full", "small"), got))


@pytest.mark.parametrize("tag,out_shape", [("full", [64, 7, 7]), ("small", [64, 1, 1])])
def test_initial_parameters_match_the_reference(drawn, tag, out_shape):
    meta, got = drawn
    want, mine = meta[tag], got[tag]
    assert mine["kind"] == "nature" and mine["out_shape"] == out_shape and mine["flat"] == out_shape[0] * out_shape[1] * out_shape[2]
    # the reference lists a module's own parameter (log_std) ahead of its children's; DualHeadNet.state_dict does the same
    names = [n for n, _s, _h in mine["params"]]
    assert ["log_std"] + [n for n in names if n != "log_std"] == want["param_names"]
    assert names[:8] == [f"encoder.{layer}.{p}" for layer in ("conv1", "conv2", "conv3", "fc") for p in ("weight", "bias")]
    for name, shape, sha in mine["params"]:
        assert shape == want["params"][name]["shape"], name
        assert sha == want["params"][name]["sha256"], name
