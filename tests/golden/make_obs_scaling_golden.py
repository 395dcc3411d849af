#!/usr/bin/env python3
"""Generate tests/golden/obs_scaling_golden.npz / .json: the REFERENCE's TVFModel under observation_scaling = centered
and unit, on CPU.

Build container only (needs the reference checkout; see ref_shim.py):  python tests/golden/make_obs_scaling_golden.py

Three seeded single-architecture models with 64 hidden units (MKL pinned as in make_nature_golden.py: the orthogonal
initialisation):
  nature       on (4, 36, 36)
  impala       on (3, 16, 16)
  impala_norm  the same impala weights with observation_normalization=True, its statistics after three updates of 8
               uint8 observations each - taken under each scaling, since the normaliser sees prep_for_model's output
For each: the policy net's state dict (`<tag>.<name>`; impala_norm shares impala's), a uint8 batch of 8 (`<tag>_x`), and
per scaling `<tag>_<scaling>_log_policy` / `_value` of model.forward(x, output="policy"); for impala_norm also
`_obs_mean`, `_obs_var`, `_obs_count` per scaling.  The weights do not depend on the scaling: one model per tag, its
`observation_scaling` attribute switched between forwards.
"""
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
PINNED = {"MKL_CBWR": "COMPATIBLE", "MKL_NUM_THREADS": "1", "OMP_NUM_THREADS": "1"}
SEED, MB, N_ACTIONS, HIDDEN = 31, 8, 6, 64
SCALINGS = ("centered", "unit")
MODELS = {"nature": ("nature", (4, 36, 36), False), "impala": ("impala", (3, 16, 16), False),
          "impala_norm": ("impala", (3, 16, 16), True)}


def main():
    from ref_shim import load_reference
    load_reference(["--model_architecture=single", "--env_embed_time=False", "--device=cpu", "--output_folder=/tmp/ref_golden_out",
                    f"--agents={MB}", "--n_steps=4", f"--seed={SEED}"])
    import torch
    from rl import config, models
    args = config.args
    out, meta = {}, {"seed": SEED, "n_actions": N_ACTIONS, "hidden_units": HIDDEN, "scalings": list(SCALINGS), "mkl_env": PINNED,
                     "head_scale": args.model.head_scale, "head_bias": args.model.head_bias, "models": {}}
    for tag, (encoder, dims, norm) in MODELS.items():
        rng = np.random.default_rng(SEED + len(tag))
        x = rng.integers(0, 256, size=(MB, *dims), dtype=np.uint8)
        x[0, :, 0, :] = 0  # zeros along a border: where a converted padding would show
        out[f"{tag}_x"] = x
        updates = [rng.integers(0, 256, size=(MB, *dims), dtype=np.uint8) for _ in range(3)]
        meta["models"][tag] = {"encoder": encoder, "input_dims": list(dims), "observation_normalization": norm,
                               "weights": "impala" if norm else tag}
        for scaling in SCALINGS:
            torch.manual_seed(SEED)
            model = models.TVFModel(
                encoder=encoder, encoder_args=None, input_dims=dims, actions=N_ACTIONS, device="cpu", architecture="single",
                dtype=torch.float32, hidden_units=HIDDEN, encoder_activation_fn="relu", observation_normalization=norm,
                head_scale=args.model.head_scale, head_bias=args.model.head_bias, value_head_names=("ext",),
                observation_scaling=scaling)
            sd = {n: p.detach().numpy().copy() for n, p in model.policy_net.state_dict().items()}
            if not norm:
                for n, a in sd.items():
                    key = f"{tag}.{n}"
                    assert key not in out or np.array_equal(out[key], a), "the initialisation depends on the scaling"
                    out[key] = a
                meta["models"][tag]["state_dict"] = list(sd)
            else:
                assert all(np.array_equal(out[f"impala.{n}"], a) for n, a in sd.items())
                for u in updates:
                    model.perform_normalization(model.prep_for_model(u), update_normalization=True)
                out[f"{tag}_{scaling}_obs_mean"] = np.asarray(model.obs_rms.mean, np.float64).copy()
                out[f"{tag}_{scaling}_obs_var"] = np.asarray(model.obs_rms.var, np.float64).copy()
                out[f"{tag}_{scaling}_obs_count"] = np.asarray(float(model.obs_rms.count))
                meta["norm_eps"] = float(model.norm_eps)
            with torch.no_grad():
                r = model.forward(x, output="policy")
            out[f"{tag}_{scaling}_log_policy"] = r["log_policy"].numpy()
            out[f"{tag}_{scaling}_value"] = r["value"].numpy()
    path = os.path.join(HERE, "obs_scaling_golden.npz")
    np.savez_compressed(path, **out)
    json.dump(meta, open(os.path.join(HERE, "obs_scaling_golden.json"), "w"), indent=1)
    print("obs_scaling_golden:", len(out), "arrays,", sum(v.nbytes for v in out.values()) / 1e6, "MB raw,",
          os.path.getsize(path) / 2 ** 20, "MiB on disk")
    assert os.path.getsize(path) < 2 ** 20


if __name__ == "__main__":
    if os.environ.get("MKL_CBWR") != PINNED["MKL_CBWR"]:
        sys.exit(subprocess.call([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=dict(os.environ, **PINNED)))
    main()
