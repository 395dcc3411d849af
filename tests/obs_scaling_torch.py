"""Test helper (no test in here): --observation_scaling's three preparations of a uint8 observation as the reference
writes them in torch (rl/models.py:846-855), the shortcuts a kernel must NOT take, and the constants the library gives the
two signed ones.

    scaled    x / 255
    centered  (x / 255 - 0.5) * 1
    unit      (x / 255 - 0.5) * 6

torch rounds every operation on its own, in float32.  tests/test_obs_scaling_cpu.py counts, over all 256 bytes, how
many each shortcut gets wrong; tests/test_obs_scaling_gpu.py holds every load of the library to `prep` bit for bit."""
from fractions import Fraction

import numpy as np
import torch

SCALINGS = ("scaled", "centered", "unit")
SIGNED = ("centered", "unit")
IN_MODE = {"scaled": 2, "centered": 4, "unit": 5}     # PPO_IN_U8, PPO_IN_U8_CENTERED, PPO_IN_U8_UNIT (include/ppo_amd.h)
OBS_PREP = {"scaled": 1, "centered": 2, "unit": 3}    # PPO_OBS_U8, PPO_OBS_U8_CENTERED, PPO_OBS_U8_UNIT
HASH_MODE = {("normed", "scaled"): 2, ("normed_offset", "scaled"): 3, ("normed", "centered"): 8,
             ("normed_offset", "centered"): 9, ("normed", "unit"): 10, ("normed_offset", "unit"): 11}


def prep(x: torch.Tensor, scaling: str) -> torch.Tensor:
    """prep_for_model's arithmetic on a uint8 tensor, the reference's expressions verbatim -> float32."""
    assert x.dtype == torch.uint8
    x = x.float()
    if scaling == "scaled":
        return x / 255.0
    if scaling == "centered":
        return ((x / 255.0) - 0.5) * 1
    if scaling == "unit":
        return ((x / 255.0) - 0.5) * 6
    raise ValueError(f"Invalid observation_scaling mode {scaling}")


def all_bytes() -> torch.Tensor:
    return torch.arange(256, dtype=torch.int32).to(torch.uint8)


def table(scaling: str) -> torch.Tensor:
    """prep of the 256 bytes, float32 [256]."""
    return prep(all_bytes(), scaling)


def exact(scaling: str):
    """The exact rational value per byte."""
    k = {"scaled": (Fraction(0), 1), "centered": (Fraction(1, 2), 1), "unit": (Fraction(1, 2), 6)}[scaling]
    return [(Fraction(b, 255) - k[0]) * k[1] for b in range(256)]


def round_f32(q: Fraction) -> np.float32:
    """The float32 nearest to a rational (ties to even), by exact comparison."""
    c = np.float32(float(q))  # float(Fraction) is correctly rounded to float64; one of c's neighbours may be nearer to q
    best = c
    for cand in (np.nextafter(c, np.float32(-np.inf)), np.nextafter(c, np.float32(np.inf))):
        dc, db = abs(Fraction(float(cand)) - q), abs(Fraction(float(best)) - q)
        if dc < db or (dc == db and int(np.float32(cand).view(np.uint32)) % 2 == 0):
            best = cand
    return np.float32(best)


def shortcuts(scaling: str):
    """name -> float32 [256]: forms that look equivalent and are not."""
    x = all_bytes().float()
    q = x / 255.0
    out = {"single_rounding": torch.from_numpy(np.array([round_f32(v) for v in exact(scaling)], dtype=np.float32))}
    if scaling == "unit":
        # q * 6 - 3 with one rounding: q has 24 significant bits, so the float64 expression is exact before it is rounded
        out["fma"] = (q.double() * 6.0 - 3.0).float()
        out["folded_scale"] = x * torch.tensor(6.0 / 255.0, dtype=torch.float32) - 3.0
    return out


def differing(a: torch.Tensor, b: torch.Tensor) -> int:
    return int((a.view(torch.int32) != b.view(torch.int32)).sum())
