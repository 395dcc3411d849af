"""Experience replay for the distillation phase - host mirror of the reference's rl/replay.py `ExperienceReplayBuffer`
(:17-279) and `smart_sample` (:282-294), on the HIP kernels of csrc/replay.hip.

The reference keeps the buffer in host NumPy, copies slot by slot in a Python loop per add (:270-273), fancy-indexes the
sample on the host and uploads it, and spends about 1.7 s per logging call on a float32 cdist (:110, :128).  Here the
observations already lie in HBM (Runner.all_obs), so the buffer does too: `data` [max_size, *obs_shape] and `aux`
[max_size, 16] float32 are allocated once, `current_size` says how much is live, an add is one scatter launch, a sample
one gather launch and the diversity statistic one exact integer kernel whose M x M int64 result is all that comes back.

What must equal the reference exactly is WHICH rows go WHERE: `plan_add` is its index arithmetic as a pure host function,
drawing from np.random in the reference's order with the reference's arguments, so that the buffer - and the host RNG
stream behind it, hence every later minibatch permutation - is where the reference's would be.
"""
import math
import time as clock

import numpy as np
import torch

from . import _lib

MODES = ("overwrite", "sequential", "uniform")


def _p(t):
    return None if t is None else t.data_ptr()


def _call(lib, fn_name, *a):
    rc = getattr(lib, fn_name)(*a, _lib.current_stream())
    if rc != 0:
        _lib.check(rc, fn_name)


def plan_add(state, n, mode, max_size, thinning=1.0):
    """The index arithmetic of add_experience (rl/replay.py:217-279) for `n` submitted rows.

    `state` = (current_size, experience_seen, ring_buffer_location).  Returns (source, destination, new_state, added):
    int64 arrays of equal length - row source[i] of the submission goes to slot destination[i], in the reference's order
    of writes - the state after the add, and the reference's `stats_last_entries_added`.  Draws from np.random exactly as
    the reference does: the thinning choice (WITH replacement, :220), the choice of entries (:243), and - for every mode
    but `sequential` - the choice of slots (:268)."""
    size, seen, ring = (int(v) for v in state)
    n, max_size = int(n), int(max_size)
    mask = None
    if thinning < 1:
        mask = np.random.choice(n, size=round(thinning * n))
        n = len(mask)
    if mode == "uniform":
        # a uniform sample over everything seen: the share of new entries falls as 1 / seen (:228-237)
        k = n if seen + n < max_size else math.ceil(n / (seen + n) * max_size)
    elif mode in ("overwrite", "sequential"):
        k = n
    else:
        raise ValueError(f"Invalid mode {mode}")
    ids = np.sort(np.random.choice(n, size=[k], replace=False))
    added = 0
    source, destination = [], []
    # grow while there is room (:249-259) ...
    new_size = min(max_size, size + len(ids))
    if size != new_size:
        new_slots = new_size - size
        source.append(ids[:new_slots])
        destination.append(np.arange(size, new_size))
        ids = ids[new_slots:]
        ring += new_slots
        added += new_slots
    # ... then place the rest by the mode's rule (:261-276); `ring` moves on by all of them even where zip drops some
    if len(ids) > 0:
        if mode == "sequential":
            spots = np.mod(np.arange(ring, ring + len(ids)), new_size)
        else:
            spots = np.random.choice(new_size, size=[min(len(ids), new_size)], replace=False)
        pairs = min(len(ids), len(spots))
        source.append(ids[:pairs])
        destination.append(spots[:pairs])
        ring += len(ids)
        added += len(ids)
    source = np.concatenate(source).astype(np.int64) if source else np.zeros(0, np.int64)
    destination = np.concatenate(destination).astype(np.int64) if destination else np.zeros(0, np.int64)
    if mask is not None:
        source = mask[source].astype(np.int64)
    return source, destination, (new_size, seen + n, ring), added


def last_write_wins(source, destination):
    """Drop all but the LAST source of every destination, order kept: in the reference a slot written twice in one add -
    a `uniform` add that grows the buffer and then draws a slot it has just filled, `sequential` wrapping round a buffer
    smaller than the submission - holds the later row.  The scatter kernel may then assume distinct slots."""
    source, destination = np.asarray(source), np.asarray(destination)
    _, first_from_the_end = np.unique(destination[::-1], return_index=True)
    keep = np.sort(len(destination) - 1 - first_from_the_end)
    return source[keep], destination[keep]


def ks_uniform(x):
    """The one-sample two-sided Kolmogorov-Smirnov statistic of x against the uniform distribution on [0, 1]
    (scipy.stats.kstest(x, scipy.stats.uniform.cdf).statistic, rl/replay.py:139) in NumPy."""
    x = np.sort(np.asarray(x, np.float64).ravel())
    n = len(x)
    cdf = np.clip(x, 0.0, 1.0)
    d_plus = (np.arange(1.0, n + 1) / n - cdf).max()
    d_minus = (cdf - np.arange(0.0, n) / n).max()
    return float(max(d_plus, d_minus))


def diversity_from_sqdist(d2):
    """rl/replay.py:113-124 from the exact squared byte distances [M, M]: L2 distances of the observations scaled to
    [0, 1], their mean (the zero diagonal included), and k1 .. k5 - the mean of the k smallest entries of every column
    with the diagonal at infinity - all in float64."""
    distances = np.sqrt(np.asarray(d2).astype(np.float64)) / 255
    results = {"mean": float(distances.mean())}
    np.fill_diagonal(distances, float("inf"))
    for k in [1, 2, 3, 4, 5]:
        results[f"k{k}"] = float(np.sort(distances, axis=0)[:k].mean())
    return results


class ExperienceReplayBuffer:
    """rl/replay.py:17-279 with the reference's names.  `data` and `aux` are the live rows of two device tensors
    allocated once at `max_size`."""

    N_AUX = _lib.PPO_REPLAY_AUX_FLOATS
    AUX_HASH = 0
    AUX_TIME = 1
    AUX_REWARD = 2
    AUX_ACTION = 3
    AUX_STEP = 4
    AUX_VTARG = 5

    def __init__(self, max_size: int, obs_shape: tuple, obs_dtype, mode="uniform", name="replay", thinning: float = 1.0,
                 device="cuda"):
        if torch.device(device).type != "cuda":
            raise _lib.PpoAmdError(f"ExperienceReplayBuffer(device={device!r}): the buffer lives in HBM and is filled and "
                                   "sampled by HIP kernels, there is no CPU path")
        if mode not in MODES:
            raise ValueError(f"Invalid mode {mode}")
        if int(max_size) <= 0:
            raise ValueError(f"max_size={max_size}: a replay buffer holds at least one row")
        _lib.require_gpu()
        self.lib = _lib.load()
        self.device = torch.device(device)
        self.max_size = int(max_size)
        self.obs_shape = tuple(int(d) for d in obs_shape)
        self.obs_dtype = obs_dtype if isinstance(obs_dtype, torch.dtype) else torch.from_numpy(np.zeros(0, obs_dtype)).dtype
        self.experience_seen = 0
        self.ring_buffer_location = 0
        self.mode = mode
        self.stats_last_entries_added = 0
        self.stats_last_entries_submitted = 0
        self.name = name
        self.thinning = thinning
        self._size = 0
        self._data = torch.zeros((self.max_size, *self.obs_shape), dtype=self.obs_dtype, device=self.device)
        self._aux = torch.zeros((self.max_size, self.N_AUX), dtype=torch.float32, device=self.device)
        self.row_bytes = int(np.prod(self.obs_shape)) * self._data.element_size()
        self._d2 = torch.zeros((_lib.PPO_REPLAY_MAX_PAIRWISE_ROWS ** 2,), dtype=torch.int64, device=self.device)
        self._noted = False

    # ------------------------------------------------------------------ what the reference exposes
    @property
    def current_size(self):
        return self._size

    @property
    def data(self):
        return self._data[:self._size]

    @property
    def aux(self):
        return self._aux[:self._size]

    @property
    def step(self):
        return self.aux[:, self.AUX_STEP]

    @property
    def time(self):
        return self.aux[:, self.AUX_TIME]

    @staticmethod
    def create_aux_buffer(shape: tuple, hash=None, time=None, reward=None, action=None, step=None, vtarg=None):
        """rl/replay.py:172-195: a float64 NumPy record per entry (add_experience narrows it to float32, as the
        reference's float32 buffer does on assignment)."""
        B = ExperienceReplayBuffer
        records = np.zeros([*shape, B.N_AUX], dtype=np.float64)
        columns = ((B.AUX_HASH, hash), (B.AUX_TIME, time), (B.AUX_REWARD, reward), (B.AUX_ACTION, action), (B.AUX_STEP, step),
                   (B.AUX_VTARG, vtarg))
        for column, values in columns:
            if values is None:
                continue
            values = values.detach().cpu().numpy() if isinstance(values, torch.Tensor) else np.asarray(values)
            if column == B.AUX_ACTION and values.ndim == 3:
                values = values[:, :, 0]  # continuous actions: the first component stands for the action (:184-186)
            records[..., column] = values
        return records

    def _rows(self, x, dtype, tail, what):
        t = torch.from_numpy(np.ascontiguousarray(x)) if isinstance(x, np.ndarray) else x
        if tuple(t.shape[1:]) != tail:
            raise AssertionError(f"Invalid shape for {what}, expecting {tail} but found {tuple(t.shape[1:])}.")
        return t, t.to(device=self.device, dtype=dtype).contiguous()

    def add_experience(self, new_experience, new_aux):
        """rl/replay.py:197-279.  new_experience [n, *obs_shape] and new_aux [n, 16]: device tensors (read where they
        lie) or NumPy arrays (uploaded).  One scatter launch; nothing is read back."""
        given, rows = self._rows(new_experience, self.obs_dtype, self.obs_shape, "new experience")
        if given.dtype != self.obs_dtype:
            raise AssertionError(f"Invalid dtype for new experience, expecting {self.obs_dtype} but found {given.dtype}.")
        _, aux = self._rows(new_aux, torch.float32, (self.N_AUX,), "new aux")
        n = int(rows.shape[0])
        if int(aux.shape[0]) != n:
            raise AssertionError(f"{n} rows of experience but {int(aux.shape[0])} aux records")
        self.stats_last_entries_submitted = n
        state = (self._size, self.experience_seen, self.ring_buffer_location)
        source, destination, state, added = plan_add(state, n, self.mode, self.max_size, self.thinning)
        source, destination = last_write_wins(source, destination)
        self.stats_last_entries_added = added
        if len(source):
            plan = torch.from_numpy(np.stack([source, destination]).astype(np.int32)).to(self.device, non_blocking=True)
            _call(self.lib, "ppo_replay_scatter_rows", _p(rows), _p(aux), n, self.row_bytes, _p(plan[0]), _p(plan[1]),
                  len(source), _p(self._data), _p(self._aux), self.max_size)
        self._size, self.experience_seen, self.ring_buffer_location = state

    def gather(self, sample, out, out_aux=None, extra=None, extra_aux=None):
        """out[i] = concatenate(data, extra)[sample[i]] (and the aux records into out_aux) in one launch: the sample of
        rl/rollout.py:2016-2048.  `sample`: int32 device tensor; `extra` [n_b, *obs_shape]: the rollout when mixing."""
        n_b = 0 if extra is None else int(extra.shape[0])
        if sample.dtype != torch.int32 or not sample.is_contiguous() or not out.is_contiguous() or out.dtype != self.obs_dtype \
                or tuple(out.shape) != (sample.numel(), *self.obs_shape):
            raise ValueError("gather: int32 sample [n] and a contiguous out [n, *obs_shape] of the buffer's dtype")
        if extra is not None and (extra.dtype != self.obs_dtype or not extra.is_contiguous() or tuple(extra.shape[1:]) != self.obs_shape):
            raise ValueError("gather: extra must be contiguous [n_b, *obs_shape] of the buffer's dtype")
        if out_aux is not None:
            if out_aux.dtype != torch.float32 or tuple(out_aux.shape) != (sample.numel(), self.N_AUX) or not out_aux.is_contiguous():
                raise ValueError(f"gather: out_aux must be contiguous float32 [n, {self.N_AUX}]")
            if n_b and (extra_aux is None or extra_aux.dtype != torch.float32 or not extra_aux.is_contiguous()
                        or tuple(extra_aux.shape) != (n_b, self.N_AUX)):
                raise ValueError(f"gather: extra_aux must be contiguous float32 [n_b, {self.N_AUX}]")
        if self._size + n_b == 0:
            raise ValueError("gather from an empty replay buffer")
        _call(self.lib, "ppo_replay_gather_rows2", _p(self._data), _p(self._aux), self._size, _p(extra) if n_b else None,
              _p(extra_aux) if n_b and out_aux is not None else None, n_b, self.row_bytes, _p(sample), sample.numel(),
              _p(out), _p(out_aux))
        return out

    def pairwise_sqdist(self, sample):
        """int64 [M, M] on the host: the exact squared L2 distances between the rows `sample` (at most 128) of the
        uint8 buffer.  One launch, one M x M copy."""
        sample = np.asarray(sample)
        M = len(sample)
        if self.obs_dtype != torch.uint8:
            raise TypeError("the pairwise-distance kernel reads uint8 rows")
        if M > _lib.PPO_REPLAY_MAX_PAIRWISE_ROWS:
            raise ValueError(f"at most {_lib.PPO_REPLAY_MAX_PAIRWISE_ROWS} rows, not {M}")
        if M == 0:
            return np.zeros((0, 0), np.int64)
        index = torch.from_numpy(sample.astype(np.int32)).to(self.device)
        _call(self.lib, "ppo_replay_pairwise_sqdist_u8", _p(self._data), self._size, self.row_bytes, _p(index), M, _p(self._d2))
        return self._d2[:M * M].cpu().numpy().reshape(M, M)

    def estimate_replay_diversity(self, max_samples=32):
        """rl/replay.py:84-124.  The sample is the reference's draw (the host RNG stream stays where the reference's
        would be); the distances are exact integers from the device, everything after them float64 on the host."""
        sample = np.random.choice(self.current_size, size=min(max_samples, self.current_size), replace=False)
        return diversity_from_sqdist(self.pairwise_sqdist(sample))

    def log_stats(self, log):
        """rl/replay.py:126-144, the reference's keys."""
        start_time = clock.time()
        if self.obs_dtype == torch.uint8:
            found = self.estimate_replay_diversity(_lib.PPO_REPLAY_MAX_PAIRWISE_ROWS)  # 128 rows, as the reference (:130)
            log.watch_mean(f"{self.name}_diversity", found["mean"], display_width=0)
            log.watch_mean(f"{self.name}_density", found["k1"], display_width=0)
            for k, v in found.items():
                log.watch_mean(f"{self.name}_diversity_{k}", v, display_width=0)
        elif not self._noted:
            self._noted = True
            log.info(f"{self.name}: the diversity estimate reads uint8 observations; not logged for {self.obs_dtype}")
        log.watch_mean(f"{self.name}_last_entries_added", self.stats_last_entries_added, display_width=0, history_length=1)
        log.watch_mean(f"{self.name}_size", self.current_size, display_width=0)
        # how evenly the buffer covers the run so far: the steps of its rows against a uniform distribution (:138-141)
        step = self.step.cpu().numpy()
        log.watch("rp_ks", ks_uniform(step / step.max()), display_width=0)
        log.watch_stats("rp_stats", step, display_width=0)
        log.watch_mean(f"{self.name}_log_time", clock.time() - start_time, display_width=0)

    # ------------------------------------------------------------------ checkpoint
    def save_state(self, force_copy=True):
        """rl/replay.py:65-74: the live rows as NumPy arrays (always a copy: they come off the device)."""
        return {"max_size": self.max_size, "experience_seen": self.experience_seen,
                "ring_buffer_location": self.ring_buffer_location, "data": self.data.cpu().numpy(),
                "aux": self.aux.cpu().numpy(), "name": self.name, "thinning": self.thinning}

    def load_state(self, state_dict: dict):
        """rl/replay.py:76-82.  The device arrays are allocated at max_size once, so a checkpoint of another size is
        refused."""
        if int(state_dict["max_size"]) != self.max_size:
            raise ValueError(f"the checkpoint's replay buffer holds {int(state_dict['max_size'])} entries, this run's "
                             f"{self.max_size}: --replay_size differs")
        data, aux = np.asarray(state_dict["data"]), np.asarray(state_dict["aux"], np.float32)
        size = len(data)
        if tuple(data.shape[1:]) != self.obs_shape or size > self.max_size or aux.shape != (size, self.N_AUX):
            raise ValueError(f"replay buffer of shape {data.shape} / {aux.shape} in the checkpoint does not fit "
                             f"[{self.max_size}, {self.obs_shape}]")
        self._data[:size].copy_(torch.from_numpy(np.ascontiguousarray(data)).to(self.obs_dtype))
        self._aux[:size].copy_(torch.from_numpy(np.ascontiguousarray(aux)))
        self._size = size
        self.experience_seen = int(state_dict["experience_seen"])
        self.ring_buffer_location = int(state_dict["ring_buffer_location"])
        self.thinning = state_dict["thinning"]


def smart_sample(x, n):
    """rl/replay.py:282-294: n samples of x without replacement; beyond len(x), whole passes first, so that every
    element is chosen at least once and counts differ by at most one."""
    if n <= len(x):
        return np.random.choice(x, size=[n], replace=False)
    return np.concatenate([smart_sample(x, len(x)), smart_sample(x, n - len(x))], axis=0)
