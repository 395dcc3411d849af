"""CPU: state hashing - the hasher's seeded parameters against tests/golden/hash_golden.json (the reference's own
LinearStateHasher; tests/golden/make_hash_golden.py), the binary bonus's threshold against a NumPy restatement of the
reference's calc_threshold, the `hash` flag group, and the argument checks of the four C entry points (they run before any
HIP call, so no GPU is needed)."""
import hashlib
import json
import os

import numpy as np
import pytest

from ppo_amd.config import Config


@pytest.fixture(scope="module")
def meta(golden_dir):
    return json.load(open(os.path.join(golden_dir, "hash_golden.json")))


def test_seeded_weights_and_bias_are_the_references(meta):
    from ppo_amd import hashing
    assert hashing.HASH_SEED == meta["hash_seed"] == 12345 and len(meta["sha256"]) == 3 * 3 * 2
    for key, want in meta["sha256"].items():
        d, bits, bias = key.split("_")
        w, b = hashing.hasher_parameters(int(d), int(bits), float(bias))
        assert tuple(w.shape) == (int(bits), int(d)) and tuple(b.shape) == (int(bits),)
        assert str(w.dtype) == str(b.dtype) == "torch.float32"
        assert hashlib.sha256(w.numpy().tobytes()).hexdigest() == want["weight"], key
        assert hashlib.sha256(b.numpy().tobytes()).hexdigest() == want["bias"], key
        assert float(w.abs().max()) <= 0.01 and float(b.abs().max()) <= float(bias)
    # two constructions give the same numbers whatever the global RNG did in between
    import torch
    a = hashing.hasher_parameters(144, 16, 0.5)
    torch.manual_seed(99)
    torch.rand(7)
    c = hashing.hasher_parameters(144, 16, 0.5)
    assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])


def reference_threshold(counts):
    """What rl/rollout.py:910-916 computes, written as a loop: walk the counts in ascending order keeping a running total
    (the sums np.cumsum forms, in its order); stop at the first total that is at least half the grand total; the answer is
    that total minus the one before it - and for the very first bin, minus the grand total (the reference's index -1)."""
    totals, running = [], np.float64(0.0)
    for c in sorted(float(v) for v in counts):
        running = running + np.float64(c) if totals else np.float64(c)
        totals.append(running)
    half = totals[-1] / 2
    first = next(k for k, t in enumerate(totals) if t >= half)
    return totals[first] - totals[first - 1]


def test_threshold_matches_the_restatement():
    from ppo_amd.hashing import StateHashTracker, bonus_threshold
    assert StateHashTracker.threshold is bonus_threshold
    rng = np.random.default_rng(0)
    planted = np.zeros(64)
    planted[[3, 9, 17, 40, 41]] = [7.25, 1.0, 0.37, 12.5, 2.0]
    dense = rng.random(256) * 9
    for table in (planted, dense, np.zeros(32), np.eye(1, 16, 5)[0] * 4.5):
        before = table.copy()
        got, want = bonus_threshold(table), reference_threshold(table)
        assert np.float64(got).tobytes() == np.float64(want).tobytes()
        assert np.array_equal(table, before)  # the table itself is not sorted in place
    # planted: sorted 0.37 1 2 7.25 12.5, half of 23.12 is reached inside the last bin
    assert bonus_threshold(planted) == (0.37 + 1.0 + 2.0 + 7.25 + 12.5) - (0.37 + 1.0 + 2.0 + 7.25)
    assert bonus_threshold(np.zeros(32)) == 0.0           # index 0, and `idx - 1` reads the last element: 0 - 0
    assert bonus_threshold(np.eye(1, 16, 5)[0] * 4.5) == 4.5


def test_a_hasher_on_the_cpu_is_refused():
    from ppo_amd import _lib, hashing
    for device in ("cpu", "meta"):
        with pytest.raises(_lib.PpoAmdError, match="no CPU path"):
            hashing.LinearStateHasher((1, 4, 4), 8, device=device)


def test_hash_flags_defaults_and_parsed_values():
    c = Config().setup([])
    h = c.hash  # rl/config.py:417-426
    assert (h.enabled, h.bits, h.bonus, h.method, h.input) == (False, 16, 0.0, "linear", "raw")
    assert (h.bonus_method, h.rescale, h.quantize, h.bias, h.decay) == ("hyperbolic", 1, 1, 0.0, 0.99)
    assert "hash_enabled" not in c.flatten()
    on = Config().setup(["--hash_enabled=True", "--hash_bits=12", "--hash_bonus=0.25", "--hash_method=linear",
                         "--hash_input=raw_centered", "--hash_bonus_method=binary", "--hash_rescale=1", "--hash_quantize=8",
                         "--hash_bias=0.5", "--hash_decay=0.9"])
    h = on.hash
    assert on._ignored == []
    assert (h.enabled, h.bits, h.bonus, h.method, h.input) == (True, 12, 0.25, "linear", "raw_centered")
    assert (h.bonus_method, h.rescale, h.quantize, h.bias, h.decay) == ("binary", 1, 8.0, 0.5, 0.9)
    flat = on.flatten()
    assert flat["hash_enabled"] is True and flat["hash_bits"] == 12 and flat["use_intrinsic_rewards"] is True
    assert Config().setup(["--hash_enabled"]).hash.enabled is True
    assert Config().setup(["--hash_enabled", "true", "--hash_bits", "9"]).hash.bits == 9


def test_a_line_that_does_not_enable_hashing_parses_as_before():
    for line in (["--hash_bonus=0.1", "--replay_size=4", "--agents=8"],
                 ["--hash_enabled=False", "--hash_bonus=0.1", "--hash_bits=8", "--agents=8"]):
        c = Config().setup(line)
        assert c._ignored == [a for a in line if a != "--agents=8"] and c.agents == 8
        assert c.hash.enabled is False and c.hash.bonus == 0.0 and c.hash.bits == 16
        assert c.use_intrinsic_rewards is False
    # a Config that parsed a hashing line and then a plain one holds the defaults again
    c = Config()
    c.setup(["--hash_enabled=True", "--hash_bonus=0.1"])
    c.setup([])
    assert c.hash.enabled is False and c.hash.bonus == 0.0 and c.use_intrinsic_rewards is False


@pytest.mark.parametrize("rnd,bonus,want", [(False, 0.0, False), (False, 0.1, True), (True, 0.0, True), (True, 0.1, True)])
def test_use_intrinsic_rewards(rnd, bonus, want):
    line = ["--hash_enabled=True", f"--hash_bonus={bonus}"]
    if rnd:
        line += ["--rnd_enabled=True", "--observation_normalization=True"]
    assert Config().setup(line).use_intrinsic_rewards is want
    if not bonus:
        assert Config().setup(line[2:]).use_intrinsic_rewards is rnd  # the same without hashing at all


def test_a_bonus_needs_hashing_enabled():
    assert Config().setup(["--hash_enabled=True", "--hash_bonus=0.1"]).hash.bonus == 0.1
    # the flags are parsed (the line enables hashing) and the last --hash_enabled wins: a bonus is left without hashing
    with pytest.raises(AssertionError, match="must be enabled"):
        Config().setup(["--hash_enabled=True", "--hash_bonus=0.1", "--hash_enabled=False"])
    # --hash_enabled=False alone: the hash flags are not parsed at all (previous test), so there is no bonus to refuse
    assert Config().setup(["--hash_enabled=False", "--hash_bonus=0.1"]).hash.bonus == 0.0


@pytest.mark.parametrize("flag,match", [("--hash_method=conv", "conv"), ("--hash_rescale=2", "rescale"),
                                        ("--hash_quantize=1.5", "quantize")])
def test_what_is_not_built_raises(flag, match):
    with pytest.raises(NotImplementedError, match=match):
        Config().setup(["--hash_enabled=True", flag])
    assert flag in Config().setup([flag])._ignored  # without hashing the flag is ignored as before


def test_bad_flag_values_raise():
    for flag in ("--hash_input=pixels", "--hash_bonus_method=cubic", "--hash_bits=25", "--hash_bits=0", "--hash_method=mlp"):
        with pytest.raises(ValueError):
            Config().setup(["--hash_enabled=True", flag])


def test_argument_validation_needs_no_gpu(hip_lib):
    one = 1 << 12  # any non-null address: the checks return before anything is read
    err = lambda: hip_lib.ppo_last_error()  # noqa: E731
    hash_args = lambda bits, obs=one, w=one, b=one, out=one, mode=0, mu=None: (  # noqa: E731
        obs, 2, 4, 8, 8, 1, 0, mode, mu, mu, 0.0, w, b, bits, out, None)
    for bits in (0, 25):
        assert hip_lib.ppo_state_hash_i32(*hash_args(bits)) == -1
        assert b"ppo_state_hash_i32" in err() and b"bits" in err()
    for kw in ({"obs": None}, {"w": None}, {"b": None}, {"out": None}, {"mode": 2}):  # normed without mu / std
        assert hip_lib.ppo_state_hash_i32(*hash_args(16, **kw)) == -1
        assert b"ppo_state_hash_i32" in err() and b"null" in err()
    assert hip_lib.ppo_state_hash_i32(one, 2, 4, 0, 8, 1, 0, 0, None, None, 0.0, one, one, 16, one, None) == -1
    assert b"bad shape" in err()
    assert hip_lib.ppo_state_hash_i32(one, 2, 4, 8, 8, 2, 0, 0, None, None, 0.0, one, one, 16, one, None) == -1
    assert b"planes" in err()
    assert hip_lib.ppo_state_hash_i32(one, 2, 4, 8, 8, 1, 0, 7, None, None, 0.0, one, one, 16, one, None) == -1
    assert b"mode" in err()

    assert hip_lib.ppo_hash_counts_update_f64(None, 4, 8, 0.99, one, one, 64, None) == -1
    assert b"ppo_hash_counts_update_f64" in err() and b"null" in err()
    assert hip_lib.ppo_hash_counts_update_f64(one, 4, 0, 0.99, one, one, 64, None) == -1 and b"bad shape" in err()
    assert hip_lib.ppo_hash_counts_update_f64(one, 4, 8, 0.99, one, one, 0, None) == -1 and b"n_bins" in err()

    assert hip_lib.ppo_hash_bonus_f32(one, 32, None, 64, 0, 0.0, 0.1, one, None) == -1
    assert b"ppo_hash_bonus_f32" in err() and b"null" in err()
    assert hip_lib.ppo_hash_bonus_f32(one, 32, one, 64, 3, 0.0, 0.1, one, None) == -1 and b"method" in err()
    assert hip_lib.ppo_hash_bonus_f32(one, -1, one, 64, 0, 0.0, 0.1, one, None) == -1 and b"bad size" in err()

    assert hip_lib.ppo_hash_count_stats(one, one, 64, None, None) == -1
    assert b"ppo_hash_count_stats" in err() and b"null" in err()
    assert hip_lib.ppo_hash_count_stats(one, one, (1 << 24) + 1, one, None) == -1 and b"n_bins" in err()
