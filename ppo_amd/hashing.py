"""State hashing on the HIP kernels - host mirror of the reference's rl/hash.py `LinearStateHasher` and of the hashing parts
of its Runner (rl/rollout.py:253-274 set-up, :652-699 generate_hashes, :755-762 the per-step counts, :895-924 the bonus,
:1243-1250 the log lines, :409-411 / :500-502 the checkpoint entries, :541-543 reset).

The reference hashes on the host - observations to float, a float32 BLAS projection, a Python loop over envs at every env
step.  Here the observations stay where they are (the rollout's uint8 buffer in HBM): one launch per env group and step
writes that group's int32 hashes (csrc/state_hash.hip), and the two float64 count tables, the bonus and the two logged
counts are one launch each per rollout.  Nothing is read back but the two logged integers (and, for the `binary` bonus
alone, the recent table, whose threshold is a sort).

Numerics: x is formed in float32 as the reference forms it; the projection is summed in float64 in a fixed order, so a
hash bit is the sign of the true sum and the same bits on every launch (the reference's float32 sum flips bits near zero
between BLAS builds).  The tables are bit-identical to the reference's float64 loop over the same hashes.

Not built (config.verify refuses them): `--hash_method=conv`, `--hash_rescale != 1`, a non-integer `--hash_quantize`.
"""
import numpy as np
import torch

from . import _lib

HASH_SEED = 12345        # rl/hash.py:34
WEIGHT_RANGE = 0.01      # rl/hash.py:35
MAX_BITS = 24
INPUT_MODES = {"raw": _lib.PPO_HASH_RAW, "raw_centered": _lib.PPO_HASH_RAW_CENTERED, "normed": _lib.PPO_HASH_NORMED,
               "normed_offset": _lib.PPO_HASH_NORMED_OFFSET}
# the normed inputs under the signed --observation_scaling values: the normaliser saw prep_for_model's output
# (rl/rollout.py:679-684), so the hash input is formed from the same preparation of the byte
NORMED_MODES = {("normed", "scaled"): _lib.PPO_HASH_NORMED, ("normed_offset", "scaled"): _lib.PPO_HASH_NORMED_OFFSET,
                ("normed", "centered"): _lib.PPO_HASH_NORMED_CENTERED,
                ("normed_offset", "centered"): _lib.PPO_HASH_NORMED_OFFSET_CENTERED,
                ("normed", "unit"): _lib.PPO_HASH_NORMED_UNIT, ("normed_offset", "unit"): _lib.PPO_HASH_NORMED_OFFSET_UNIT}
BONUS_METHODS = {"hyperbolic": _lib.PPO_HASH_BONUS_HYPERBOLIC, "quadratic": _lib.PPO_HASH_BONUS_QUADRATIC,
                 "binary": _lib.PPO_HASH_BONUS_BINARY}


def _p(t):
    return None if t is None else t.data_ptr()


def _call(lib, fn_name, *a):
    rc = getattr(lib, fn_name)(*a, _lib.current_stream())
    if rc != 0:
        _lib.check(rc, fn_name)


def hasher_parameters(in_d: int, bits: int, bias: float = 0.0):
    """(weight [bits, in_d], bias [bits]) float32 on the CPU: LinearStateHasher's projection (rl/hash.py:30-37) - both drawn
    from one fresh CPU generator seeded with 12345, the weight first, so that the hashes need no stored parameters."""
    g = torch.Generator()
    g.manual_seed(HASH_SEED)
    w = torch.empty(int(bits), int(in_d), dtype=torch.float32).uniform_(-WEIGHT_RANGE, WEIGHT_RANGE, generator=g)
    b = torch.empty(int(bits), dtype=torch.float32).uniform_(-float(bias), float(bias), generator=g)
    return w, b


def bonus_threshold(recent):
    """The count below which the `binary` bonus pays +1 (rl/rollout.py:910-916): the size of the bin at which the running
    total of the ascending counts reaches half of everything counted.  With that bin first in the order, `i - 1` wraps
    to the last running total, as it does in the reference; the table is left as it is."""
    running = np.cumsum(np.sort(np.asarray(recent)))
    i = np.searchsorted(running, running[-1] / 2)
    return running[i] - running[i - 1]


class LinearStateHasher:
    """rl/hash.py:22-54.  `input_space` is the shape of what is hashed - (1, H, W) for the first plane of a frame stack,
    (C, H, W) for whole observations.  The weights are drawn on the CPU and uploaded once."""

    def __init__(self, input_space: tuple, output_bits: int = 16, device="cuda", bias=0.0):
        if not 1 <= int(output_bits) <= MAX_BITS:
            raise ValueError(f"output_bits={output_bits}: 1 to {MAX_BITS}")
        if torch.device(device).type != "cuda":  # (the reference's default is "cpu")
            raise _lib.PpoAmdError(f"LinearStateHasher(device={device!r}): the hash is a HIP kernel, there is no CPU path")
        _lib.require_gpu()
        self.lib = _lib.load()
        self.input_space = tuple(int(d) for d in input_space)
        self.bits = int(output_bits)
        self.in_d = int(np.prod(self.input_space))
        self.device = torch.device(device)
        w, b = hasher_parameters(self.in_d, self.bits, bias)
        self.weight, self.bias = w.to(self.device), b.to(self.device)

    def hash_observations(self, obs: torch.Tensor, out: torch.Tensor = None, quantize: int = 0, mode: str = "raw",
                          norm=None):
        """Hashes of uint8 observations [B, C, H, W] on the device (a row slice of a larger buffer is fine), written to
        `out` (int32 [B], contiguous; default: a fresh tensor).  With input_space[0] == 1 < C the first plane alone is read.
        `norm`: the model's ObsNormalizer, whose current float32 constants and observation_scaling the normed modes use.
        No host read."""
        if obs.dtype != torch.uint8 or obs.dim() != 4 or not obs.is_contiguous() or obs.device != self.weight.device:
            raise ValueError(f"expected a contiguous uint8 [B, C, H, W] tensor on {self.weight.device}")
        B, C, H, W = (int(d) for d in obs.shape)
        planes = self.input_space[0]
        if self.input_space[1:] != (H, W) or planes not in (1, C):
            raise ValueError(f"observations {tuple(obs.shape[1:])} do not fit a hasher of {self.input_space}")
        normed = mode in ("normed", "normed_offset")
        if normed and (norm is None or norm.F != C * H * W):
            raise ValueError(f"hash input '{mode}' needs the observation normaliser of {(C, H, W)} observations")
        if out is None:
            out = torch.empty(B, dtype=torch.int32, device=obs.device)
        elif out.dtype != torch.int32 or out.numel() != B or not out.is_contiguous():
            raise ValueError("out must be a contiguous int32 tensor with one entry per row")
        code = NORMED_MODES[mode, getattr(norm, "observation_scaling", "scaled")] if normed else INPUT_MODES[mode]
        _call(self.lib, "ppo_state_hash_i32", _p(obs), B, C, H, W, planes, int(quantize), code,
              _p(norm.mu) if normed else None, _p(norm.std) if normed else None, float(norm.norm_eps) if normed else 0.0,
              _p(self.weight), _p(self.bias), self.bits, _p(out))
        return out

    def __call__(self, x):
        """forward (rl/hash.py:41-54) on uint8 input [B, *input_space]: a device tensor gives a device tensor (no host
        round trip), a NumPy array a NumPy array, as the reference returns."""
        host = isinstance(x, np.ndarray)
        t = torch.from_numpy(np.ascontiguousarray(x)) if host else x
        if t.dtype != torch.uint8:
            raise TypeError("the hash kernel forms its input from uint8 observations (hash_observations: quantise, centre, "
                            "normalise); a float input is not built")
        t = t.to(self.weight.device).reshape(t.shape[0], *self.input_space).contiguous()
        h = self.hash_observations(t)
        return h.cpu().numpy() if host else h

    forward = __call__


class StateHashTracker:
    """What the reference's Runner keeps for hashing: `hash_global_counts` and `hash_recent_counts` (float64 [2^bits]),
    the rollout's `obs_hashes` [N, A], and the per-rollout work on them."""

    def __init__(self, hasher: LinearStateHasher, n_steps: int, agents: int, decay: float = 0.99, bonus: float = 0.0,
                 bonus_method: str = "hyperbolic", quantize: int = 0, mode: str = "raw"):
        if bonus_method not in BONUS_METHODS:
            raise ValueError(f"Invalid hash_bonus_method {bonus_method}")
        if mode not in INPUT_MODES:
            raise ValueError(f"Invalid hash_input {mode}")
        self.hasher, self.lib, self.device = hasher, hasher.lib, hasher.weight.device
        self.N, self.A, self.n_bins = int(n_steps), int(agents), 2 ** hasher.bits
        self.decay, self.bonus, self.bonus_method = float(decay), float(bonus), bonus_method
        self.quantize, self.mode = int(quantize), mode
        self.global_counts = torch.zeros(self.n_bins, dtype=torch.float64, device=self.device)
        self.recent_counts = torch.zeros(self.n_bins, dtype=torch.float64, device=self.device)
        self.obs_hashes = torch.zeros((self.N, self.A), dtype=torch.int32, device=self.device)
        self._stats = torch.zeros(2, dtype=torch.int64, device=self.device)
        self.last_threshold = None

    # ------------------------------------------------------------------ during the rollout
    def hash_step(self, obs: torch.Tensor, t: int, lo: int, hi: int, norm=None):
        """obs_hashes[t, lo:hi] = hash of `obs` (the observations envs [lo, hi) returned at env step t), on the current
        stream; only the hashes are written - the tables wait for update_counts()."""
        self.hasher.hash_observations(obs, out=self.obs_hashes[t, lo:hi], quantize=self.quantize, mode=self.mode, norm=norm)

    # ------------------------------------------------------------------ after the rollout
    threshold = staticmethod(bonus_threshold)

    def update_counts(self, hashes: torch.Tensor = None):
        """rl/rollout.py:758-762 for the N steps of the rollout, in the reference's order, from obs_hashes - or from
        `hashes`, a contiguous int32 [N, A'] tensor: under data parallelism the hashes of every rank's envs, so that the
        tables count what all of them visited and stand identical on every rank (the bonus still reads obs_hashes)."""
        if hashes is None:
            hashes = self.obs_hashes
        elif hashes.dtype != torch.int32 or hashes.dim() != 2 or hashes.shape[0] != self.N or not hashes.is_contiguous() \
                or hashes.device != self.device:
            raise ValueError(f"hashes must be a contiguous int32 [{self.N}, A] tensor on {self.device}")
        _call(self.lib, "ppo_hash_counts_update_f64", _p(hashes), self.N, int(hashes.shape[1]), self.decay,
              _p(self.global_counts), _p(self.recent_counts), self.n_bins)

    def add_bonus(self, int_rewards: torch.Tensor):
        """int_rewards[t, a] += bonus * g(recent[obs_hashes[t, a]]) with the final recent counts (rl/rollout.py:918-924)."""
        if int_rewards.dtype != torch.float32 or tuple(int_rewards.shape) != (self.N, self.A) or not int_rewards.is_contiguous():
            raise ValueError(f"int_rewards must be a contiguous float32 [{self.N}, {self.A}] tensor")
        threshold = 0.0
        if self.bonus_method == "binary":  # a sort of the table: host NumPy, the reference's own expression
            threshold = self.last_threshold = float(bonus_threshold(self.recent_counts.cpu().numpy()))
        _call(self.lib, "ppo_hash_bonus_f32", _p(self.obs_hashes), self.N * self.A, _p(self.recent_counts), self.n_bins,
              BONUS_METHODS[self.bonus_method], threshold, self.bonus, _p(int_rewards))

    def launch_stats(self):
        """Queue the reduction behind the log lines; fetch with stats()."""
        _call(self.lib, "ppo_hash_count_stats", _p(self.global_counts), _p(self.recent_counts), self.n_bins, _p(self._stats))

    @property
    def device_stats(self):
        """The int64 pair launch_stats() fills, on the device: a caller that already copies statistics to the host takes
        it along (Runner.log_returns) instead of paying stats()'s own read."""
        return self._stats

    def stats(self, launch: bool = True):
        """(count_nonzero(global), count_nonzero(recent.astype(int))) - rl/rollout.py:1248-1250; one 16-byte read."""
        if launch:
            self.launch_stats()
        g, r = self._stats.cpu().tolist()
        return int(g), int(r)

    # ------------------------------------------------------------------ checkpoint, reset
    def state_dict(self):
        """The reference's checkpoint entries (rl/rollout.py:409-411): float64 NumPy arrays."""
        return {"hash_global_counts": self.global_counts.cpu().numpy(), "hash_recent_counts": self.recent_counts.cpu().numpy()}

    def load_state_dict(self, sd):
        for key, table in (("hash_global_counts", self.global_counts), ("hash_recent_counts", self.recent_counts)):
            a = np.asarray(sd[key], np.float64)
            if a.shape != (self.n_bins,):
                raise ValueError(f"{key}: {a.shape} in the checkpoint, {(self.n_bins,)} here (--hash_bits differs)")
            table.copy_(torch.from_numpy(np.ascontiguousarray(a)))

    def reset(self):
        """rl/rollout.py:541-543."""
        self.global_counts.zero_()
        self.recent_counts.zero_()
