"""CPU: the IMPALA encoder's `down_sample` argument ('pool' | 'stride' | 'none', rl/models.py:62-80, rl/impala.py:85-123)
on the host side - ImpalaSpec's geometry against torch.nn.Conv2d / max_pool2d output shapes computed here, the argument
checks, and init_parameters against the reference's initial weights.

tests/golden/impala_downsample_golden.json (tests/golden/make_impala_downsample_golden.py) holds the sha256 of every
parameter of the reference's TVFModel(encoder="impala", encoder_args={'down_sample': m}, single) built under
torch.manual_seed(seed); ppo_amd.models.init_parameters(ImpalaSpec(..., down_sample=m)) must draw the same values from
the same seed under the same names and in the same order - the stride of a convolution does not enter its initialiser.
The heads' orthogonal initialiser is a LAPACK QR factorisation, so - as in tests/test_nature_init.py - the draws are made
in a child process with MKL pinned the way the fixture's were."""
import json
import os
import subprocess
import sys

import pytest

torch = pytest.importorskip("torch")

from ppo_amd import models  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(4, 84, 84), (3, 64, 64), (3, 20, 28), (2, 5, 6), (1, 1, 1)]
MODES = ["pool", "stride", "none"]


def torch_stack_shapes(input_dims, channels, mode):
    """[(cin, cout, h_in, w_in, h_out, w_out)] from the shapes torch's own layers produce on a one-image batch."""
    c, h, w = input_dims
    x = torch.zeros(1, c, h, w)
    stacks = []
    for cout in channels:
        y = torch.nn.Conv2d(x.shape[1], cout, 3, stride=2 if mode == "stride" else 1, padding=1)(x)
        if mode == "pool":
            y = torch.nn.functional.max_pool2d(y, kernel_size=3, stride=2, padding=1)
        stacks.append((x.shape[1], cout, x.shape[2], x.shape[3], y.shape[2], y.shape[3]))
        x = y
    return stacks, tuple(x.shape[1:])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("input_dims", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("channels", [(16, 32, 32), (8, 24)], ids=["default", "8-24"])
def test_spec_geometry_matches_torch(input_dims, mode, channels):
    with torch.no_grad():
        stacks, out_shape = torch_stack_shapes(input_dims, channels, mode)
    sp = models.ImpalaSpec(input_dims, channels=channels, hidden_units=64, down_sample=mode)
    assert sp.down_sample == mode
    assert [tuple(s) for s in sp.stacks] == stacks
    assert tuple(sp.out_shape) == out_shape and sp.flat == out_shape[0] * out_shape[1] * out_shape[2]
    if mode == "none":
        assert tuple(sp.out_shape[1:]) == tuple(input_dims[1:])


@pytest.mark.parametrize("input_dims", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_stride_and_pool_share_every_map_shape(input_dims):
    """floor((h + 2 - 2 - 1) / 2) + 1 == (h + 1) // 2: behind the first convolution a 'stride' net's maps are a 'pool'
    net's, so its residual blocks keep their launches."""
    a = models.ImpalaSpec(input_dims, down_sample="pool")
    b = models.ImpalaSpec(input_dims, down_sample="stride")
    assert a.stacks == b.stacks and a.out_shape == b.out_shape and a.flat == b.flat


def test_default_is_pool():
    assert models.ImpalaSpec((4, 84, 84)).down_sample == "pool"
    assert models.ImpalaSpec((4, 84, 84)).out_shape == (32, 11, 11)


@pytest.mark.parametrize("bad", ["avg", "Pool", "", None, 2])
def test_bad_mode_raises_the_references_error(bad):
    with pytest.raises(ValueError, match="Invalid down_sample mode"):
        models.ImpalaSpec((4, 84, 84), down_sample=bad)


@pytest.mark.parametrize("mode", MODES)
def test_batch_norm_is_not_implemented(mode):
    with pytest.raises(NotImplementedError, match="batch_norm"):
        models.ImpalaSpec((4, 84, 84), down_sample=mode, batch_norm=True)
    assert models.ImpalaSpec((4, 84, 84), down_sample=mode, batch_norm=False).down_sample == mode


_CHILD = r'''
import hashlib, json, sys
sys.path.insert(0, sys.argv[2])
import numpy as np
import torch
from ppo_amd import models

out = []
for job in json.loads(sys.argv[1]):
    args = dict(job["encoder_args"])
    if "channels" in args:
        args["channels"] = tuple(args["channels"])
    torch.manual_seed(job["seed"])
    spec = models.ImpalaSpec(tuple(job["input_dims"]), hidden_units=job["hidden"], **args)
    init = models.init_parameters(spec, job["n_actions"], 1, job["head_scale"], job["head_bias"])
    out.append({"kind": spec.kind, "out_shape": list(spec.out_shape), "flat": spec.flat,
                "params": [[n, list(t.shape), hashlib.sha256(np.ascontiguousarray(t.numpy()).tobytes()).hexdigest()]
                           for n, t in init.items()]})
print(json.dumps(out))
'''
TAGS = ("stride", "none")


@pytest.fixture(scope="module")
def drawn(golden_dir):
    meta = json.load(open(os.path.join(golden_dir, "impala_downsample_golden.json")))
    jobs = [{"seed": meta[tag]["seed"], "input_dims": meta[tag]["input_dims"], "hidden": meta[tag]["hidden_units"],
             "encoder_args": meta[tag]["encoder_args"], "n_actions": meta["n_actions"], "head_scale": meta["head_scale"],
             "head_bias": meta["head_bias"]} for tag in TAGS]
    r = subprocess.run([sys.executable, "-c", _CHILD, json.dumps(jobs), ROOT], env=dict(os.environ, **meta["mkl_env"]),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    return meta, dict(zip(TAGS, got))


@pytest.mark.parametrize("tag,out_shape", [("stride", [32, 5, 5]), ("none", [16, 12, 10])])
def test_initial_parameters_match_the_reference(drawn, tag, out_shape):
    meta, got = drawn
    want, mine = meta[tag], got[tag]
    assert want["encoder_args"]["down_sample"] == tag and want["out_shape"] == out_shape
    assert mine["kind"] == "impala" and mine["out_shape"] == out_shape and mine["flat"] == out_shape[0] * out_shape[1] * out_shape[2]
    # the reference lists a module's own parameter (log_std) ahead of its children's; DualHeadNet.state_dict does the same
    names = [n for n, _s, _h in mine["params"]]
    assert ["log_std"] + [n for n in names if n != "log_std"] == want["param_names"]
    assert names[:2] == ["encoder.stacks.0.firstconv.weight", "encoder.stacks.0.firstconv.bias"]
    for name, shape, sha in mine["params"]:
        assert shape == want["params"][name]["shape"], name
        assert sha == want["params"][name]["sha256"], name
