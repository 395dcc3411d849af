"""Writes tests/golden/humanoid_init_{policy,value}_net.npz: the initial parameters of the `humanoid` variant of
variants_golden.npz (make_variants_golden.py), one file per net.

variants_golden.json records only the sha256 of every parameter the reference drew under torch.manual_seed(7).  The
orthogonal initialiser is a LAPACK QR factorisation whose last bits depend on the host (tests/test_model_init.py), so a
net built on another host starts a few ulp away from the one the recorded forward outputs belong to - at 256 hidden units
and 128 TVF heads that alone is ~0.9 of the forward bar of tests/test_variants_gpu.py.  This script draws the parameters
with ppo_amd's initialiser and writes them only if EVERY one hashes to the reference's recorded sha256, i.e. on a host
that takes the fixture's code path; the tests then load these instead of drawing their own.

    python tests/golden/make_humanoid_init_golden.py
"""
import hashlib
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from ppo_amd import models  # noqa: E402

TAG = "humanoid"


def main():
    gold = np.load(os.path.join(HERE, "variants_golden.npz"))
    m = json.load(open(os.path.join(HERE, "variants_golden.json")))[TAG]
    torch.manual_seed(7)
    spec = models.MLPSpec(tuple(m["input_dims"]), hidden_units=m["hidden"])
    for prefix in ("policy_net", "value_net"):  # drawn in sequence, as the dual architecture does
        init = models.init_parameters(spec, m["n_actions"], 1, m["head_scale"], m["head_bias"],
                                      len(gold[f"{TAG}_tvf_horizons"]))
        out = {}
        for name, t in init.items():
            a = np.ascontiguousarray(t.numpy())
            want = m["params"][f"{prefix}.{name}"]
            if list(a.shape) != want["shape"] or hashlib.sha256(a.tobytes()).hexdigest() != want["sha256"]:
                raise SystemExit(f"{prefix}.{name}: this host does not draw the reference's parameters; nothing written")
            out[name] = a
        path = os.path.join(HERE, f"{TAG}_init_{prefix}.npz")
        np.savez_compressed(path, **out)
        print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
