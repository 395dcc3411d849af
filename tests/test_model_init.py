"""CPU: our parameter initialiser reproduces the reference's initial weights bit for bit.

model_golden.json holds sha256 / moments of every parameter of a reference
TVFModel(impala, single) built under torch.manual_seed(1) (tests/golden/make_model_golden.py);
ppo_amd.models.init_impala_parameters must draw the same values from the same seed
(reference construction order: rl/models.py:348-368, :73-84, rl/impala.py:60-62,96-100;
initialisers: rl/tensor_utilities.py:40-95).

The orthogonal initialiser is a LAPACK QR factorisation, whose last bits depend on the host CPU's vector code path
and on the thread count under MKL's default dispatch.  So the draws are made in a child process with MKL pinned to one
code path (MKL reads its settings once, at its first call), and compared with the reference's draws under the same
pin (tests/golden/init_pinned_golden.json, tests/golden/make_init_pinned_golden.py): bit for bit on any x86 host."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from ppo_amd.models import ImpalaSpec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# argv: the jobs (JSON), the repository root.  Prints, per job, {parameter name: [shape, sha256]}.
_CHILD = r'''
import hashlib, json, sys
sys.path.insert(0, sys.argv[2])
import numpy as np
import torch
from ppo_amd import models


def digest(t):
    a = np.ascontiguousarray(t.numpy())
    return [list(a.shape), hashlib.sha256(a.tobytes()).hexdigest()]


out = []
for job in json.loads(sys.argv[1]):
    if job["kind"] == "impala":
        torch.manual_seed(job["seed"])
        spec = models.ImpalaSpec(tuple(job["input_dims"]), hidden_units=job["hidden"])
        init = models.init_impala_parameters(spec, job["n_actions"], 1, job["head_scale"], job["head_bias"])
        out.append({n: digest(t) for n, t in init.items()})
        continue
    scaled = models.tvf_feature_mask(job["n_tvf"], job["hidden"], *job["mask"]) if job["mask"] else None
    torch.manual_seed(job["seed"])
    spec = models.MLPSpec(tuple(job["input_dims"]), hidden_units=job["hidden"])
    got = {}
    for prefix in ("policy_net", "value_net"):  # drawn in sequence, as the dual architecture does
        init = models.init_parameters(spec, job["n_actions"], 1, job["head_scale"], job["head_bias"], job["n_tvf"])
        if scaled is not None:
            init["tvf_head.weight"] = init["tvf_head.weight"] * scaled  # DualHeadNet._build_tvf_feature_mask
        got.update({f"{prefix}.{n}": digest(t) for n, t in init.items()})
    out.append(got)
print(json.dumps(out))
'''


def _pinned_init(golden_dir, jobs):
    """Our initial parameters for `jobs`, drawn under the fixture's MKL settings; and the fixture's hashes."""
    pinned = json.load(open(os.path.join(golden_dir, "init_pinned_golden.json")))
    r = subprocess.run([sys.executable, "-c", _CHILD, json.dumps(jobs), ROOT], env=dict(os.environ, **pinned["mkl_env"]),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1]), pinned["params"]


def _assert_bitwise(got, want, label):
    assert set(got) == set(want), label
    for name, info in want.items():
        shape, sha = got[name]
        assert shape == info["shape"], (label, name)
        assert sha == info["sha256"], (label, name)


def _metas(golden_dir):
    shapes = json.load(open(os.path.join(golden_dir, "shapes_golden.json")))
    return {"c2": json.load(open(os.path.join(golden_dir, "model_golden.json"))), "c3": shapes["c3"], "c4": shapes["c4"]}


@pytest.mark.parametrize("tag,n_params", [("c2", 1092579), ("c3", 630126), ("c4", 1091549)])
def test_initial_parameters_match_reference_bitwise(golden_dir, tag, n_params):
    """c2: 4x84x84 / 6 actions (Pong), c3: 3x64x64 / 15 actions (procgen), c4: 4x84x84 / 4 actions (Breakout)."""
    meta = _metas(golden_dir)[tag]
    (got,), want = _pinned_init(golden_dir, [dict(
        kind="impala", seed=meta["seed"], input_dims=meta["input_dims"], hidden=meta["hidden_units"],
        n_actions=meta["n_actions"], head_scale=meta["head_scale"], head_bias=meta["head_bias"])])
    assert set(got) == set(meta["params"])
    assert all(got[n][0] == info["shape"] for n, info in meta["params"].items())
    _assert_bitwise(got, want[tag], tag)
    assert sum(int(np.prod(s)) for s, _ in got.values()) == n_params  # c2: SURVEY.md §8a R9 [probed] parameter count at 6 actions


def test_geometry():
    spec = ImpalaSpec((4, 84, 84))
    assert spec.out_shape == (32, 11, 11) and spec.flat == 3872
    assert ImpalaSpec((3, 64, 64)).flat == 32 * 8 * 8


def test_mlp_dual_tvf_initial_parameters_match_reference_bitwise(golden_dir):
    """MLP encoder, dual architecture (policy_net then value_net drawn in sequence), with and without the
    TVF head (tests/golden/make_variants_golden.py; rl/models.py:157-161, 364-384, 605-607)."""
    meta = json.load(open(os.path.join(golden_dir, "variants_golden.json")))
    gold = np.load(os.path.join(golden_dir, "variants_golden.npz"))
    tags = ("mlp_gauss_tvf", "mlp_disc")
    jobs = []
    for tag in tags:
        m = meta[tag]
        n_tvf = len(gold[f"{tag}_tvf_horizons"]) if f"{tag}_tvf_horizons" in gold else 0
        jobs.append(dict(kind="mlp", seed=7, input_dims=m["input_dims"], hidden=m["hidden"], n_actions=m["n_actions"],
                         head_scale=m["head_scale"], head_bias=m["head_bias"], n_tvf=n_tvf, mask=None))
    got, want = _pinned_init(golden_dir, jobs)
    for tag, g in zip(tags, got):
        assert set(g) == set(meta[tag]["params"]), tag
        _assert_bitwise(g, want[tag], tag)


@pytest.mark.parametrize("tag", ["sparsity", "window"])
def test_tvf_feature_masks_and_masked_initial_head_match_reference_bitwise(golden_dir, tag):
    """--tvf_feature_sparsity / --tvf_feature_window (rl/models.py:386-421; tests/golden/make_tvf_mask_golden.py): the
    0 / 1 mask and the masked, rescaled initial TVF head from the same seeds as the reference, bit for bit."""
    from ppo_amd.models import tvf_feature_mask
    meta = json.load(open(os.path.join(golden_dir, "tvf_mask_golden.json")))[tag]
    gold = np.load(os.path.join(golden_dir, "tvf_mask_golden.npz"))
    K, H = len(gold["horizons"]), meta["hidden"]
    scaled = tvf_feature_mask(K, H, meta["tvf_feature_sparsity"], meta["tvf_feature_window"])
    assert np.array_equal(torch.gt(scaled, 0).to(torch.uint8).numpy(), gold[f"{tag}_mask"])
    (got,), want = _pinned_init(golden_dir, [dict(
        kind="mlp", seed=7, input_dims=meta["input_dims"], hidden=H, n_actions=meta["n_actions"],
        head_scale=meta["head_scale"], head_bias=meta["head_bias"], n_tvf=K,
        mask=[meta["tvf_feature_sparsity"], meta["tvf_feature_window"]])])
    assert set(got) == set(meta["params"])
    _assert_bitwise(got, want[tag], tag)
    assert np.array_equal(gold[f"{tag}_init_value_net.tvf_head.weight"], gold[f"{tag}_w0"])
