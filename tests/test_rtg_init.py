"""CPU: geometry and initialiser of the RTG encoder (rl/models.py:172-213).

RtgSpec reproduces the sizes the reference's constructor finds by a forward pass (max_pool2d(., 2, 2) floors), and
ppo_amd.models.init_parameters(RtgSpec(...)) draws the reference's initial weights bit for bit: tests/golden/rtg_golden.json
(tests/golden/make_rtg_golden.py) holds the sha256 of every parameter of the reference's TVFModel(encoder="rtg", single)
built under torch.manual_seed(seed), at (4, 84, 84) / hidden 512 and at (4, 36, 46) / hidden 64.  All four layers keep
torch's default initialisation (plain nn.Conv2d / nn.Linear: no LAPACK), the heads are the orthogonal CustomLinear, so -
as in tests/test_nature_init.py - the draws are made in a child process with MKL pinned the way the fixture's were."""
import json
import os
import subprocess
import sys

import pytest

from ppo_amd import models
from ppo_amd.config import Config

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
    spec = models.RtgSpec(tuple(job["input_dims"]), hidden_units=job["hidden"])
    init = models.init_parameters(spec, job["n_actions"], 1, job["head_scale"], job["head_bias"])
    out.append({"kind": spec.kind, "out_shape": list(spec.out_shape), "flat": spec.flat,
                "params": [[n, list(t.shape), hashlib.sha256(np.ascontiguousarray(t.numpy()).tobytes()).hexdigest()]
                           for n, t in init.items()]})
print(json.dumps(out))
'''


def sizes(spec):
    """[(conv h, conv w, pooled h, pooled w)] per layer."""
    return [tuple(layer[8:12]) for layer in spec.layers]


def test_geometry_full_size():
    sp = models.RtgSpec((4, 84, 84), hidden_units=512)
    assert sp.kind == "rtg" and sp.hidden_units == 512
    assert sizes(sp) == [(41, 41, 20, 20), (20, 20, 10, 10), (10, 10, 5, 5)]
    assert sp.pool_shapes == [(32, 41, 41), (64, 20, 20), (64, 10, 10)]
    assert sp.out_shape == (64, 5, 5) and sp.flat == 1600
    # (name, cin, cout, kernel, stride, padding, h_in, w_in)
    assert [layer[:8] for layer in sp.layers] == [("conv1", 4, 32, 4, 2, 0, 84, 84), ("conv2", 32, 64, 3, 1, 1, 20, 20),
                                                   ("conv3", 64, 64, 3, 1, 1, 10, 10)]


def test_geometry_odd_sides():
    """(4, 36, 46): an odd height at pool 1, odd widths at pools 2 and 3."""
    sp = models.RtgSpec((4, 36, 46), hidden_units=64)
    assert sizes(sp) == [(17, 22, 8, 11), (8, 11, 4, 5), (4, 5, 2, 2)]
    assert sp.out_shape == (64, 2, 2) and sp.flat == 256


def test_geometry_smallest_input_and_ignored_arguments():
    sp = models.RtgSpec((1, 18, 18), base_channels=7, channels=(1, 2), down_sample="stride")  # **ignore_args
    assert sizes(sp) == [(8, 8, 4, 4), (4, 4, 2, 2), (2, 2, 1, 1)]
    assert sp.out_shape == (64, 1, 1) and sp.flat == 64 and sp.hidden_units == 512
    assert models.RtgSpec((4, 18, 18)).layers[0][1] == 4


def test_refusals():
    with pytest.raises(ValueError, match=r"\[C, H, W\]"):
        models.RtgSpec((128,))
    with pytest.raises(ValueError, match="too small"):
        models.RtgSpec((4, 17, 84))
    with pytest.raises(ValueError, match="too small"):
        models.RtgSpec((4, 84, 17))
    with pytest.raises(ValueError, match="hidden_units"):
        models.RtgSpec((4, 84, 84), hidden_units=0)


def test_config_keeps_the_encoder():
    cfg = Config()
    cfg.setup(["--model_encoder=rtg"])
    assert cfg.model.encoder == "rtg"


@pytest.fixture(scope="module")
def drawn(golden_dir):
    meta = json.load(open(os.path.join(golden_dir, "rtg_golden.json")))
    jobs = [{"seed": meta[tag]["seed"], "input_dims": meta[tag]["input_dims"], "hidden": meta[tag]["hidden_units"],
             "n_actions": meta["n_actions"], "head_scale": meta["head_scale"], "head_bias": meta["head_bias"]}
            for tag in ("full", "small")]
    r = subprocess.run([sys.executable, "-c", _CHILD, json.dumps(jobs), ROOT], env=dict(os.environ, **meta["mkl_env"]),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    return meta, dict(zip(("full", "small"), got))


@pytest.mark.parametrize("tag,out_shape", [("full", [64, 5, 5]), ("small", [64, 2, 2])])
def test_initial_parameters_match_the_reference(drawn, tag, out_shape):
    meta, got = drawn
    want, mine = meta[tag], got[tag]
    assert mine["kind"] == "rtg" and mine["out_shape"] == out_shape and mine["flat"] == out_shape[0] * out_shape[1] * out_shape[2]
    # the reference lists a module's own parameter (log_std) ahead of its children's; DualHeadNet.state_dict does the same
    names = [n for n, _s, _h in mine["params"]]
    assert ["log_std"] + [n for n in names if n != "log_std"] == want["param_names"]
    assert names[:8] == [f"encoder.{layer}.{p}" for layer in ("conv1", "conv2", "conv3", "fc") for p in ("weight", "bias")]
    for name, shape, sha in mine["params"]:
        assert shape == want["params"][name]["shape"], name
        assert sha == want["params"][name]["sha256"], name
