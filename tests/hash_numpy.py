"""NumPy restatements the state-hashing tests compare against (no test in here): the hash input in float32 exactly as
rl/rollout.py:670-684 forms it, the projection in float64, the reference's per-step count loop (:758-762) and its bonus
(:898-924)."""
import numpy as np


def hash_input(obs, planes, mode="raw", quantize=0, mu=None, std=None, eps=0.0):
    """float32 [B, D] from uint8 [B, C, H, W]: planes == 1 reads channel 0, planes == C everything in memory order."""
    o = np.asarray(obs)
    assert o.dtype == np.uint8 and o.ndim == 4 and planes in (1, o.shape[1])
    if quantize:
        o = o - o % np.uint8(quantize)  # each byte rounded down to a multiple of the step
    B = o.shape[0]
    o = o[:, :planes].reshape(B, -1)
    if mode == "raw":
        return o.astype(np.float32)
    if mode == "raw_centered":
        return o.astype(np.float32) - np.float32(128)
    d = o.shape[1]
    m, s = (np.asarray(a, np.float32).reshape(-1)[:d] for a in (mu, std))
    x = np.clip((o.astype(np.float32) / np.float32(255) - m) / (s + np.float32(eps)), np.float32(-5), np.float32(5))
    assert x.dtype == np.float32
    return x if mode == "normed" else x + np.float32(3)


def project(x, w, b):
    """(hashes int32 [B], p float64 [B, bits], bound [B, bits]): the float64 projection and the largest error a float64
    sum of its D + 1 terms can have in any order, (D + 2) 2^-53 (sum |w x| + |b|)."""
    x, w, b = (np.asarray(a, np.float64) for a in (x, w, b))
    p = np.zeros((x.shape[0], w.shape[0]))
    mag = np.zeros_like(p)
    for i in range(w.shape[0]):  # (a [B, bits, D] temporary would be 100 MB at the product's geometry)
        t = x * w[i]
        p[:, i] = t.sum(-1) + b[i]
        mag[:, i] = np.abs(t).sum(-1) + abs(b[i])
    bound = (x.shape[1] + 2) * 2.0 ** -53 * mag
    hashes = ((p > 0) * (1 << np.arange(w.shape[0], dtype=np.int64))).sum(-1).astype(np.int32)
    return hashes, p, bound


def count_loop(hashes, decay, global_counts, recent_counts):
    """rl/rollout.py:758-762 over the rows of hashes [N, A], in place on float64 tables; entries outside the tables are
    skipped."""
    n = global_counts.shape[0]
    for t in range(hashes.shape[0]):
        recent_counts *= decay
        for h in hashes[t]:
            if 0 <= h < n:
                global_counts[h] += 1
                recent_counts[h] += 1


def bonus(rewards, hashes, recent, method, bonus_value, threshold=None):
    """rl/rollout.py:898-924: float32(float64(r) + bonus * g(recent[h]))."""
    c = np.asarray(recent, np.float64)[hashes]
    if method == "hyperbolic":
        g = 1 / c
    elif method == "quadratic":
        g = 1 / (c * c)
    else:
        g = np.where(c < threshold, 1.0, -1.0)
    return np.float32(np.asarray(rewards, np.float32).astype(np.float64) + bonus_value * g)
