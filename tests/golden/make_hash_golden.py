#!/usr/bin/env python3
"""Generate tests/golden/hash_golden.npz / .json: the REFERENCE's state hashes on CPU.

Build container only (needs the reference checkout; see ref_shim.py):  python tests/golden/make_hash_golden.py

The hashes come from the reference's own rl.hash.LinearStateHasher (CPU, float32 nn.Linear).  Its caller,
Runner.generate_hashes (rl/rollout.py:652-699), needs a Runner and cv2, which the shim mocks, so the preprocessing lines
are RESTATED here in NumPy / torch, line for line: the quantisation (:670-671), the four inputs (:674-684, with
prep_for_model's x / 255 and perform_normalization's clamp((x - mu) / (std + eps), -5, 5), rl/models.py:692) and the
channel filter (:665-668: the first plane for atari, everything otherwise).

Cases: every combination of
  shape    (1, 12, 12) one plane (D = 144), (4, 13, 11) one plane of four (D = 143: odd, rows of 572 bytes),
           (3, 8, 8) all planes (D = 192)
  input    raw, raw_centered, normed, normed_offset (mu / std stored per shape, eps = EPS)
  quantize 1, 8
  bias     0, 0.5
  bits     5, 16, 20
on B = 6 uint8 observations per shape, in the order of itertools.product(shape, input, quantize, bias, bits) - the .json
holds the axes, not a list of 144 cases.  Stored: the observations, mu and std, the hashes [case, B], the sha256 of every
weight / bias pair, and per case (`margins` [case, 2]) the smallest |p| over its B x bits projections and the largest
float32 bound (D + 2) 2^-24 (sum |w x| + |b|) - what a float32 sum of D + 1 terms can be off by, whatever its order.

The seed of the observations is the first (from SEED upwards) for which NO projection of any case lies inside that bound:
the reference's float32 result and the float64 sum (also computed here, and checked) then agree on every bit, and a test
against this file has nothing to exclude.
"""
import hashlib
import itertools
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
SEED, B, EPS = 1, 6, 0.003
SHAPES = (((1, 12, 12), 1), ((4, 13, 11), 1), ((3, 8, 8), 3))  # (observation shape, planes hashed)
MODES = ("raw", "raw_centered", "normed", "normed_offset")
QUANTIZE, BIAS, BITS = (1, 8), (0.0, 0.5), (5, 16, 20)


def hash_input(torch, obs, planes, mode, q, mu, std):
    """What generate_hashes hands to the hasher (rl/rollout.py:665-684), in this project's words: bytes rounded down to a
    multiple of q, the leading `planes` planes, then the input mode.  The same values: uint8 for raw (the hasher converts),
    float64 for raw_centered, float32 torch for the normed modes."""
    floored = obs - obs % q if q else obs  # uint8 in, uint8 out
    if mode in ("raw", "raw_centered"):
        picked = floored[:, :planes]
        return picked if mode == "raw" else picked.astype(np.float64) - 128.0
    scaled = torch.from_numpy(floored).float() / 255  # prep_for_model
    normed = ((scaled - torch.from_numpy(mu)) / (torch.from_numpy(std) + EPS)).clamp(-5, 5)[:, :planes]
    return normed + 3.0 if mode == "normed_offset" else normed


def main():
    from ref_shim import load_reference
    load_reference(["--device=cpu", "--output_folder=/tmp/ref_golden_out"])
    import torch
    from rl import hash as ref_hash

    cases = list(itertools.product(range(len(SHAPES)), MODES, QUANTIZE, BIAS, BITS))
    for seed in range(SEED, SEED + 256):
        rng = np.random.default_rng(seed)
        out, meta_cases, sha, ok = {}, [], {}, True
        data = []
        for k, (shape, _planes) in enumerate(SHAPES):
            obs = rng.integers(0, 256, (B, *shape), dtype=np.uint8)
            mu = rng.uniform(0.2, 0.6, shape).astype(np.float32)
            std = rng.uniform(0.05, 0.3, shape).astype(np.float32)
            out[f"obs_{k}"], out[f"mu_{k}"], out[f"std_{k}"] = obs, mu, std
            data.append((obs, mu, std))
        hashes = np.zeros((len(cases), B), np.int32)
        for ci, (k, mode, q, bias, bits) in enumerate(cases):
            shape, planes = SHAPES[k]
            obs, mu, std = data[k]
            space = (planes, *shape[1:])
            hasher = ref_hash.LinearStateHasher(space, bits, device="cpu", bias=bias)
            x = hash_input(torch, obs, planes, mode, q, mu, std)
            hashes[ci] = hasher(x if isinstance(x, np.ndarray) else x.clone())
            w = hasher.projection.weight.detach().numpy()
            b = hasher.projection.bias.detach().numpy()
            D = w.shape[1]
            sha[f"{D}_{bits}_{bias}"] = {"weight": hashlib.sha256(w.tobytes()).hexdigest(),
                                         "bias": hashlib.sha256(b.tobytes()).hexdigest()}
            # the float64 sum of the same float32 inputs
            x32 = (torch.from_numpy(x) if isinstance(x, np.ndarray) else x).to(torch.float32).numpy().reshape(B, -1)
            terms = x32.astype(np.float64)[:, None, :] * w.astype(np.float64)[None]
            p = terms.sum(-1) + b.astype(np.float64)
            bound = (D + 2) * 2.0 ** -24 * (np.abs(terms).sum(-1) + np.abs(b.astype(np.float64)))
            if (np.abs(p) <= bound).any():
                ok = False
                break
            h64 = ((p > 0) * (1 << np.arange(bits))).sum(-1).astype(np.int32)
            assert np.array_equal(h64, hashes[ci]), (seed, ci, "float64 and the reference's float32 disagree outside the bound")
            meta_cases.append((float(np.abs(p).min()), float(bound.max())))
        if ok:
            break
    else:
        raise SystemExit("no seed found")
    out["hashes"] = hashes
    # the per-case margins, in case order: [case, 2] = (smallest |p|, largest float32 bound)
    out["margins"] = np.asarray(meta_cases, np.float64)
    # the cases are itertools.product(shapes, input, quantize, bias, bits) in that order: the axes say it all
    meta = {"seed": seed, "B": B, "eps": EPS, "shapes": [{"obs": list(s), "planes": p} for s, p in SHAPES],
            "axes": {"input": list(MODES), "quantize": list(QUANTIZE), "bias": list(BIAS), "bits": list(BITS)},
            "sha256": sha, "hash_seed": 12345}
    np.savez_compressed(os.path.join(HERE, "hash_golden.npz"), **out)
    with open(os.path.join(HERE, "hash_golden.json"), "w") as f:
        json.dump(meta, f, separators=(",", ":"))
    print(f"seed {seed}: {len(cases)} cases, min |p| {out['margins'][:, 0].min():.3e}, "
          f"max float32 bound {out['margins'][:, 1].max():.3e}, "
          f"{os.path.getsize(os.path.join(HERE, 'hash_golden.npz'))} + "
          f"{os.path.getsize(os.path.join(HERE, 'hash_golden.json'))} bytes")


if __name__ == "__main__":
    main()
