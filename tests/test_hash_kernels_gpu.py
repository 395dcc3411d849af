"""GPU: the state-hashing kernels (csrc/state_hash.hip) - hashes against tests/golden/hash_golden.npz (the reference's own
LinearStateHasher on CPU, tests/golden/make_hash_golden.py) and against a float64 NumPy projection, the count tables against
the reference's float64 loop byte for byte, the bonus and the two logged counts.

Nothing here has a tolerance.  A hash bit is the sign of a float64 sum; the only bits a correct kernel may get "wrong" are
those with |p| <= (D + 2) 2^-53 (sum |w x| + |b|), and every test asserts that its inputs have none (smallest |p| over
all inputs of this file, computed on the CPU: 2.8e-5, against bounds below 3.7e-9)."""
import itertools
import json
import os

import numpy as np
import pytest

import hash_numpy as HN

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from ppo_amd import hashing  # noqa: E402


@pytest.fixture(scope="module")
def gold(golden_dir):
    return (np.load(os.path.join(golden_dir, "hash_golden.npz")),
            json.load(open(os.path.join(golden_dir, "hash_golden.json"))))


class Norm:
    """What hash_observations reads of an ObsNormalizer."""

    def __init__(self, mu, std, eps):
        self.mu, self.std = (torch.from_numpy(np.ascontiguousarray(a, np.float32).reshape(-1)).cuda() for a in (mu, std))
        self.norm_eps, self.F = float(eps), self.mu.numel()


def rows_of(buffer_rows, skip):
    """The rows as a slice at a non-zero offset of a larger device buffer."""
    pad = np.zeros((skip, *buffer_rows.shape[1:]), np.uint8) + 7
    whole = torch.from_numpy(np.concatenate([pad, buffer_rows, pad])).cuda()
    return whole[skip:skip + buffer_rows.shape[0]]


# ---------------------------------------------------------------- against the reference
def test_every_fixture_case_hashes_as_the_reference(gold):
    g, meta = gold
    hashers = {}
    ax = meta["axes"]
    cases = list(itertools.product(range(len(meta["shapes"])), ax["input"], ax["quantize"], ax["bias"], ax["bits"]))
    assert len(cases) == 3 * 4 * 2 * 2 * 3 == len(g["hashes"]) == len(g["margins"])
    for ci, (k, mode, q, bias, bits) in enumerate(cases):
        obs = g[f"obs_{k}"]
        space = (meta["shapes"][k]["planes"], *obs.shape[2:])
        assert list(obs.shape[1:]) == meta["shapes"][k]["obs"]
        key = (space, bits, bias)
        if key not in hashers:
            hashers[key] = hashing.LinearStateHasher(space, bits, device="cuda", bias=bias)
        got = hashers[key].hash_observations(rows_of(obs, 2), quantize=q, mode=mode,
                                             norm=Norm(g[f"mu_{k}"], g[f"std_{k}"], meta["eps"]))
        assert got.dtype == torch.int32
        assert np.array_equal(got.cpu().numpy(), g["hashes"][ci]), (ci, cases[ci])  # no exclusions: see the margins
        assert g["margins"][ci, 0] > g["margins"][ci, 1]


# ---------------------------------------------------------------- against float64
SETTINGS = (("raw", 0, 0.0, 16), ("raw_centered", 8, 0.5, 20), ("normed", 1, 0.0, 5), ("normed_offset", 8, 0.5, 16),
            ("raw", 3, 0.5, 24), ("raw_centered", 0, 0.0, 1))
# (observation shape, planes, B): the fixture's shapes at every B of {1, 37, 64}, rows of 105 bytes (no row but the first is
# 4-byte aligned), and the product's geometry - one plane of a 4 x 84 x 84 stack, two trips through the loop over D
GEOMETRIES = [(shape, planes, B) for shape, planes in (((1, 12, 12), 1), ((4, 13, 11), 1), ((3, 8, 8), 3))
              for B in (1, 37, 64)] + [((3, 5, 7), 3, 37), ((4, 84, 84), 1, 33)]


@pytest.mark.parametrize("shape,planes,B", GEOMETRIES)
def test_hashes_are_the_sign_of_the_float64_projection(shape, planes, B):
    rng = np.random.default_rng(sum(shape) * 1000 + B)
    obs = rng.integers(0, 256, (B, *shape), dtype=np.uint8)
    mu = rng.uniform(0.2, 0.6, shape).astype(np.float32)
    std = rng.uniform(0.05, 0.3, shape).astype(np.float32)
    dev = rows_of(obs, 1)
    assert dev.data_ptr() % 4 == (int(np.prod(shape)) % 4)
    for mode, q, bias, bits in SETTINGS:
        h = hashing.LinearStateHasher((planes, *shape[1:]), bits, device="cuda", bias=bias)
        got = h.hash_observations(dev, quantize=q, mode=mode, norm=Norm(mu, std, 0.003)).cpu().numpy()
        want, p, bound = HN.project(HN.hash_input(obs, planes, mode, q, mu, std, 0.003), h.weight.cpu().numpy(),
                                    h.bias.cpu().numpy())
        print(f"HASH {shape} B={B} {mode} q={q} bias={bias} bits={bits} min|p|={np.abs(p).min():.3e} max bound={bound.max():.3e}")
        assert not (np.abs(p) <= bound).any(), "an input of this test lies inside the rounding bound: pick another seed"
        assert np.array_equal(got, want), (mode, q, bias, bits, np.flatnonzero(got != want))
        assert (got >= 0).all() and (got < 2 ** bits).all()


def test_the_hash_does_not_depend_on_alignment_batch_or_repetition():
    rng = np.random.default_rng(5)
    shape, B = (4, 12, 12), 37
    obs = rng.integers(0, 256, (B, *shape), dtype=np.uint8)
    h = hashing.LinearStateHasher((1, 12, 12), 16, device="cuda", bias=0.5)
    aligned = torch.from_numpy(obs).cuda()
    first = h.hash_observations(aligned, quantize=8, mode="raw_centered")
    assert torch.equal(first, h.hash_observations(aligned, quantize=8, mode="raw_centered"))  # twice: the same
    parts = torch.cat([h.hash_observations(aligned[:5], quantize=8, mode="raw_centered"),
                       h.hash_observations(aligned[5:], quantize=8, mode="raw_centered")])
    assert torch.equal(first, parts)                                                           # split: the same
    flat = torch.zeros(obs.size + 1, dtype=torch.uint8, device="cuda")
    flat[1:].copy_(aligned.view(-1))
    shifted = flat[1:].view(B, *shape)  # the same rows one byte off: the scalar path walks them in the same order
    assert shifted.data_ptr() % 4 == 1 and shifted.is_contiguous()
    assert torch.equal(first, h.hash_observations(shifted, quantize=8, mode="raw_centered"))
    out = torch.full((B + 2,), -7, dtype=torch.int32, device="cuda")
    h.hash_observations(aligned, out=out[1:B + 1], quantize=8, mode="raw_centered")
    assert torch.equal(out[1:B + 1], first) and int(out[0]) == -7 and int(out[-1]) == -7     # nothing written outside


def test_all_zero_rows_hash_to_zero_and_numpy_input_round_trips():
    h = hashing.LinearStateHasher((3, 8, 8), 16, device="cuda", bias=0.0)
    zeros = torch.zeros((5, 3, 8, 8), dtype=torch.uint8, device="cuda")
    assert not h.hash_observations(zeros).any()  # 0 > 0 is false for every bit
    rng = np.random.default_rng(2)
    obs = rng.integers(0, 256, (4, 3, 8, 8), dtype=np.uint8)
    got = h(obs)
    assert isinstance(got, np.ndarray) and got.dtype == np.int32
    assert np.array_equal(got, h(torch.from_numpy(obs).cuda()).cpu().numpy())
    assert np.array_equal(got, HN.project(HN.hash_input(obs, 3), h.weight.cpu().numpy(), h.bias.cpu().numpy())[0])
    with pytest.raises(TypeError):
        h(obs.astype(np.float32))
    with pytest.raises(ValueError):
        h.hash_observations(torch.zeros((2, 3, 8, 9), dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="normaliser"):
        h.hash_observations(zeros, mode="normed")


# ---------------------------------------------------------------- counts
def tracker(n_steps, agents, bits, **kw):
    return hashing.StateHashTracker(hashing.LinearStateHasher((1, 4, 4), bits, device="cuda"), n_steps, agents, **kw)


def planted_hashes():
    """[6, 9] over 64 bins: several envs on one bin in one step, one bin hit in consecutive steps, bins never hit, one entry
    out of range."""
    h = np.array([[5, 5, 5, 9, 17, 5, 40, 63, 0],
                  [5, 9, 9, 22, 22, 22, 22, 41, 0],
                  [5, 64, 30, 31, 32, 33, 34, 35, 36],   # 64: one past the table
                  [63, 63, 63, 63, 63, 63, 63, 63, 63],
                  [5, 1, 2, 3, 4, 6, 7, 8, 10],
                  [17, 17, 9, 9, 40, 40, 0, 0, 63]], np.int32)
    assert h.shape == (6, 9) and 50 not in h and 12 not in h
    return h


@pytest.mark.parametrize("case", ["planted", "two_blocks"])
def test_count_tables_are_bit_identical_to_the_float64_loop(case):
    rng = np.random.default_rng(7)
    if case == "planted":
        N, A, bits, decay = 6, 9, 6, 0.99
        hashes = planted_hashes()
    else:  # 2048 bins = two workgroups, 11 steps = a full chunk of 8 and a partial one, hits on both sides of the seam
        N, A, bits, decay = 11, 33, 11, 0.9
        pool = np.array([0, 1, 511, 1022, 1023, 1024, 1025, 1500, 2046, 2047, 2048, -1, 700, 701, 1300], np.int32)
        hashes = rng.choice(pool, size=(N, A)).astype(np.int32)
    n = 2 ** bits
    # tables of an earlier, decayed state: non-integer values
    glob = np.floor(rng.random(n) * 5) * (rng.random(n) < 0.5)
    recent = rng.random(n) * 3 * (rng.random(n) < 0.6)
    tr = tracker(N, A, bits, decay=decay)
    tr.global_counts.copy_(torch.from_numpy(glob))
    tr.recent_counts.copy_(torch.from_numpy(recent))
    tr.obs_hashes.copy_(torch.from_numpy(hashes))
    tr.update_counts()
    want_g, want_r = glob.copy(), recent.copy()
    HN.count_loop(hashes, decay, want_g, want_r)
    got_g, got_r = tr.global_counts.cpu().numpy(), tr.recent_counts.cpu().numpy()
    assert got_g.dtype == got_r.dtype == np.float64
    assert got_g.tobytes() == want_g.tobytes()
    assert got_r.tobytes() == want_r.tobytes()
    in_range = (hashes >= 0) & (hashes < n)
    assert not in_range.all() and got_g.sum() - glob.sum() == in_range.sum()  # the out-of-range entries changed nothing
    never = np.setdiff1d(np.arange(n), hashes[in_range])
    assert len(never) and np.array_equal(got_g[never], glob[never])
    # N separate multiplications, not decay ** N
    assert got_r[never].tobytes() != (recent[never] * decay ** N).tobytes() or not recent[never].any()
    # a second rollout continues from the tables as they stand
    tr.update_counts()
    HN.count_loop(hashes, decay, want_g, want_r)
    assert tr.global_counts.cpu().numpy().tobytes() == want_g.tobytes()
    assert tr.recent_counts.cpu().numpy().tobytes() == want_r.tobytes()


# ---------------------------------------------------------------- bonus, stats
@pytest.mark.parametrize("method", ["hyperbolic", "quadratic", "binary"])
@pytest.mark.parametrize("bonus", [0.1, -0.25])
def test_bonus_is_the_float64_expression_stored_as_float32(method, bonus):
    rng = np.random.default_rng(11)
    N, A, bits = 6, 9, 6
    hashes = planted_hashes()
    hashes[2, 1] = 12
    recent = 0.05 + rng.random(64) * 7
    rewards = rng.normal(size=(N, A)).astype(np.float32)
    tr = tracker(N, A, bits, bonus=bonus, bonus_method=method)
    tr.recent_counts.copy_(torch.from_numpy(recent))
    tr.obs_hashes.copy_(torch.from_numpy(hashes))
    dev = torch.from_numpy(rewards).cuda()
    tr.add_bonus(dev)
    threshold = HN_threshold(recent) if method == "binary" else None
    want = HN.bonus(rewards, hashes, recent, method, bonus, threshold)
    assert want.dtype == np.float32 and not np.array_equal(want, rewards)
    assert dev.cpu().numpy().tobytes() == want.tobytes()
    if method == "binary":
        assert tr.last_threshold == threshold
        assert {float(x) for x in np.unique(np.where(recent[hashes] < threshold, 1.0, -1.0))} == {1.0, -1.0}


def HN_threshold(recent):
    x = np.cumsum(np.sort(recent))
    i = np.searchsorted(x, x[-1] / 2)
    return float(x[i] - x[i - 1])


@pytest.mark.parametrize("bits", [6, 16])
def test_stats_are_the_two_count_nonzero_expressions(bits):
    rng = np.random.default_rng(bits)
    n = 2 ** bits
    glob = np.floor(rng.random(n) * 4) * (rng.random(n) < 0.4)
    recent = rng.random(n) * 2.5 * (rng.random(n) < 0.7)  # zeros, values below 1 and values from 1 up
    recent[:4] = [1.0, 0.9999999999999999, 1.0000000000000002, 0.0]
    tr = tracker(4, 4, bits)
    tr.global_counts.copy_(torch.from_numpy(glob))
    tr.recent_counts.copy_(torch.from_numpy(recent))
    want = (int(np.count_nonzero(glob)), int(np.count_nonzero(recent.astype(int))))
    assert tr.stats() == want and tr.stats() == want  # (the pair is overwritten, not accumulated)
    assert 0 < want[1] < np.count_nonzero(recent)
    tr.reset()
    assert tr.stats() == (0, 0) and not tr.global_counts.any() and not tr.recent_counts.any()
