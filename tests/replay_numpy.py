"""NumPy restatements the replay tests compare against (no test in here): the reference's buffer semantics
(rl/replay.py:197-279) on host arrays that grow by concatenation and are written row by row in a loop - later writes to a
slot replace earlier ones, as in the reference - and the exact squared distances of uint8 rows.

`NumpyReplay.add` draws from np.random as the reference does (the thinning choice with replacement, the choice of entries,
the choice of slots for every mode but `sequential`), so a test seeds np.random, runs this and the code under test from the
same seed and compares arrays and counters.  tests/test_replay_cpu.py checks this file itself against the reference's
recorded results (tests/golden/replay_golden.npz)."""
import math

import numpy as np

N_AUX = 16


class NumpyReplay:
    def __init__(self, max_size, obs_shape, dtype, mode, thinning=1.0):
        self.max_size, self.mode, self.thinning = int(max_size), mode, thinning
        self.data = np.zeros((0, *obs_shape), dtype)
        self.aux = np.zeros((0, N_AUX), np.float32)
        self.seen = self.ring = self.added = self.submitted = 0

    def add(self, rows, aux):
        rows, aux = np.asarray(rows), np.asarray(aux)
        self.submitted = len(rows)
        if self.thinning < 1:
            pick = np.random.choice(len(rows), size=round(self.thinning * len(rows)))  # with replacement
            rows, aux = rows[pick], aux[pick]
        n = len(rows)
        k = n
        if self.mode == "uniform" and self.seen + n >= self.max_size:
            k = math.ceil(n / (self.seen + n) * self.max_size)
        elif self.mode not in ("uniform", "overwrite", "sequential"):
            raise ValueError(self.mode)
        chosen = np.sort(np.random.choice(n, size=[k], replace=False))
        self.added = 0
        room = min(self.max_size - len(self.data), len(chosen))
        if room > 0:  # the buffer grows first
            self.data = np.concatenate([self.data, rows[chosen[:room]]])
            self.aux = np.concatenate([self.aux, aux[chosen[:room]].astype(np.float32)])
            chosen = chosen[room:]
            self.ring += room
            self.added += room
        if len(chosen):
            size = len(self.data)
            if self.mode == "sequential":
                slots = (self.ring + np.arange(len(chosen))) % size
            else:
                slots = np.random.choice(size, size=[min(len(chosen), size)], replace=False)
            for s, d in zip(chosen, slots):  # in order: a slot written twice keeps the later row
                self.data[d] = rows[s]
                self.aux[d] = aux[s]
            self.ring += len(chosen)
            self.added += len(chosen)
        self.seen += n


def pairwise_sqdist(rows):
    """int64 [M, M]: sum_k (x_i[k] - x_j[k])^2 of uint8 rows [M, D], exact.  Formed as |x_i|^2 + |x_j|^2 - 2 x_i . x_j with
    the products summed by a float64 matrix product: every term is an integer, every partial sum an integer below
    255^2 D < 2^53 for D < 1.3e11, so float64 holds each of them exactly whatever the order of summation."""
    x = np.asarray(rows)
    assert x.dtype == np.uint8 and x.ndim == 2 and x.shape[1] < 2 ** 36
    f = x.astype(np.float64)
    gram = (f @ f.T).astype(np.int64)
    sq = np.diagonal(gram)
    return sq[:, None] + sq[None, :] - 2 * gram


def pairwise_sqdist_loop(rows):
    """The same by subtraction in int64, pair by pair (small inputs: what pairwise_sqdist is checked against)."""
    x = np.asarray(rows).astype(np.int64)
    return np.asarray([[((a - b) ** 2).sum() for b in x] for a in x], np.int64).reshape(len(x), len(x))
