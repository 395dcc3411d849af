"""GPU: the replay kernels (csrc/replay.hip) - the scatter of an add and the two-source gather of a sample against torch
indexing, the pairwise squared distances against exact int64 NumPy (tests/replay_numpy.py), and the buffer class on top of
them against the NumPy restatement of the reference's buffer.

Nothing here has a tolerance: rows are copied bytes, distances are integers.  Every scatter / gather case frames each of
its buffers (rows and aux records, source and destination) with a canary row on either side and finds them untouched."""
import numpy as np
import pytest

import replay_numpy as RN

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from ppo_amd import _lib, replay  # noqa: E402

N_AUX = 16
CANARY, AUX_CANARY = 0xA5, 12345.0
# 105: no multiple of 16 (byte path); 4096: one pass of 256 vectors; 28224: the product's 4x84x84 row; 36880: 2305 vectors,
# more than one pass of 256 x 8 plus a ragged tail
ROW_BYTES = (105, 4096, 28224, 36880)


def ptr(t):
    return None if t is None else t.data_ptr()


def call(name, *a):
    lib = _lib.load()
    rc = getattr(lib, name)(*a, _lib.current_stream())
    assert rc == 0, lib.ppo_last_error()


class Framed:
    """`rows` [n, row_bytes] uint8 on the device with a canary row before and after, optionally starting `offset` bytes
    into the allocation (offset 1: nothing is 16-byte aligned, the kernels must take their byte path)."""

    def __init__(self, rows, offset=0):
        n, rb = rows.shape
        self.flat = torch.full((offset + (n + 2) * rb,), CANARY, dtype=torch.uint8, device="cuda")
        self.lo, self.hi = offset + rb, offset + (n + 1) * rb
        self.rows = self.flat[self.lo:self.hi].view(n, rb)
        self.rows.copy_(torch.from_numpy(rows))

    def intact(self):
        return bool((self.flat[:self.lo] == CANARY).all() and (self.flat[self.hi:] == CANARY).all())


class FramedAux:
    def __init__(self, aux):
        n = aux.shape[0]
        self.whole = torch.full((n + 2, N_AUX), AUX_CANARY, dtype=torch.float32, device="cuda")
        self.rows = self.whole[1:n + 1]
        self.rows.copy_(torch.from_numpy(aux))

    def intact(self):
        return bool((self.whole[0] == AUX_CANARY).all() and (self.whole[-1] == AUX_CANARY).all())


def random_rows(rng, n, rb):
    return rng.integers(0, 256, (n, rb), dtype=np.uint8), rng.normal(size=(n, N_AUX)).astype(np.float32)


def dev_i32(a):
    return torch.from_numpy(np.asarray(a, np.int32)).cuda()


def run_scatter(rng, rb, n, offset=0, n_src=None, R=None, ids=None, spots=None):
    n_src, R = n_src or n + 7, R or n + 9
    src, dst = (Framed(random_rows(rng, k, rb)[0], offset) for k in (n_src, R))
    src_aux, dst_aux = (FramedAux(random_rows(rng, k, rb)[1]) for k in (n_src, R))
    if ids is None:
        ids = rng.integers(0, n_src, n)  # sources may repeat
        ids[0] = n_src - 1
        spots = rng.permutation(np.arange(1, R - 1))[:n]  # destinations are distinct, and include slots R - 1 and 0
        spots[0] = R - 1
        if n > 1:
            ids[1], spots[1] = 0, 0
    ids_t, spots_t = dev_i32(ids), dev_i32(spots)
    want, want_aux, src_before = dst.rows.clone(), dst_aux.rows.clone(), src.rows.clone()
    ci, cs = torch.from_numpy(np.clip(ids, 0, n_src - 1)).cuda(), torch.from_numpy(np.clip(spots, 0, R - 1)).cuda()
    want[cs] = src.rows[ci]
    want_aux[cs] = src_aux.rows[ci]
    call("ppo_replay_scatter_rows", ptr(src.rows), ptr(src_aux.rows), n_src, rb, ptr(ids_t), ptr(spots_t), n, ptr(dst.rows),
         ptr(dst_aux.rows), R)
    torch.cuda.synchronize()
    assert torch.equal(dst.rows, want) and torch.equal(dst_aux.rows, want_aux)
    assert torch.equal(src.rows, src_before)
    assert src.intact() and dst.intact() and src_aux.intact() and dst_aux.intact()


def run_gather(rng, rb, n, offset=0, n_a=11, n_b=6, samples=None):
    a, a_aux = random_rows(rng, n_a, rb)
    A, A_aux = Framed(a, offset), FramedAux(a_aux)
    if n_b:
        b, b_aux = random_rows(rng, n_b, rb)
        B, B_aux = Framed(b, offset), FramedAux(b_aux)
    total = n_a + n_b
    if samples is None:
        samples = rng.integers(0, total, n)
        edge = [n_a] if n == 1 else [n_a - 1, n_a, total - 1]  # the last row of a, the first and the last of b
        edge = [min(e, total - 1) for e in edge]
        samples[:len(edge)] = edge
    out, out_aux = Framed(np.zeros((n, rb), np.uint8), offset), FramedAux(np.zeros((n, N_AUX), np.float32))
    s_t = dev_i32(samples)
    cs = torch.from_numpy(np.clip(samples, 0, total - 1)).cuda()
    both = torch.cat([A.rows, B.rows]) if n_b else A.rows
    both_aux = torch.cat([A_aux.rows, B_aux.rows]) if n_b else A_aux.rows
    call("ppo_replay_gather_rows2", ptr(A.rows), ptr(A_aux.rows), n_a, ptr(B.rows) if n_b else None,
         ptr(B_aux.rows) if n_b else None, n_b, rb, ptr(s_t), n, ptr(out.rows), ptr(out_aux.rows))
    torch.cuda.synchronize()
    assert torch.equal(out.rows, both[cs]) and torch.equal(out_aux.rows, both_aux[cs])
    assert out.intact() and out_aux.intact() and A.intact() and A_aux.intact() and (not n_b or (B.intact() and B_aux.intact()))
    # without aux records: rows alone
    out2 = Framed(np.zeros((n, rb), np.uint8), offset)
    call("ppo_replay_gather_rows2", ptr(A.rows), None, n_a, ptr(B.rows) if n_b else None, None, n_b, rb, ptr(s_t), n,
         ptr(out2.rows), None)
    torch.cuda.synchronize()
    assert torch.equal(out2.rows, both[cs]) and out2.intact()


@pytest.mark.parametrize("n", [1, 3, 300])
@pytest.mark.parametrize("rb", ROW_BYTES)
def test_scatter_matches_torch_indexing(rb, n):
    run_scatter(np.random.default_rng(rb + n), rb, n)


@pytest.mark.parametrize("n", [1, 3, 300])
@pytest.mark.parametrize("rb", ROW_BYTES)
def test_gather_from_two_sources_matches_torch_indexing(rb, n):
    rng = np.random.default_rng(2 * rb + n)
    run_gather(rng, rb, n)
    run_gather(rng, rb, n, n_b=0)  # the buffer alone


@pytest.mark.parametrize("rb", [4096, 28224])
def test_views_offset_by_one_byte_take_the_byte_path(rb):
    rng = np.random.default_rng(rb)
    run_scatter(rng, rb, 3, offset=1)
    run_gather(rng, rb, 3, offset=1)
    run_gather(rng, rb, 3, offset=1, n_b=0)


def test_indices_outside_the_buffers_are_clamped_into_them():
    rng = np.random.default_rng(5)
    for rb in (105, 4096):
        run_scatter(rng, rb, 4, n_src=6, R=9, ids=np.asarray([-3, 2, 6, 2 ** 31 - 1]), spots=np.asarray([4, -1, 7, 2 ** 31 - 1]))
        run_gather(rng, rb, 4, n_a=5, n_b=3, samples=np.asarray([-7, 8, 2 ** 31 - 1, 4]))
        run_gather(rng, rb, 2, n_a=5, n_b=0, samples=np.asarray([5, -1]))


# ---------------------------------------------------------------- pairwise distances
_rows = {}


def distance_rows(D):
    """131 rows of D bytes, row 1 all 0 and row 2 all 255, and their exact distances, made once per D."""
    if D not in _rows:
        data = np.random.default_rng(D).integers(0, 256, (131, D), dtype=np.uint8)
        data[1], data[2] = 0, 255
        _rows[D] = (data, torch.from_numpy(data).cuda(), RN.pairwise_sqdist(data))
    return _rows[D]


@pytest.mark.parametrize("M", [1, 2, 17, 128])
@pytest.mark.parametrize("D", [1, 105, 28224, 70000])
def test_pairwise_distances_are_exact(D, M):
    data, dev, all_pairs = distance_rows(D)
    index = np.random.default_rng(M).permutation(131)[:M]
    index[:2] = (2, 1)[:M]  # the all-255 and the all-0 row
    if M > 2:
        index[2:] = [i if i not in (1, 2) else 0 for i in index[2:]]
    want = all_pairs[np.ix_(index, index)]
    if M >= 2:
        assert want[0, 1] == 255 * 255 * D and (D < 70000 or want[0, 1] > 2 ** 32)
    idx = dev_i32(index)
    out = torch.full((2, M * M + 1), -1, dtype=torch.int64, device="cuda")
    for k in range(2):
        call("ppo_replay_pairwise_sqdist_u8", ptr(dev), 131, D, ptr(idx), M, ptr(out[k]))
    torch.cuda.synchronize()
    got = out[0, :M * M].cpu().numpy().reshape(M, M)
    assert got.dtype == np.int64 and np.array_equal(got, want)
    assert np.array_equal(got, got.T) and not np.diagonal(got).any()
    assert torch.equal(out[0], out[1]) and int(out[0, -1]) == -1  # the same bits again, and nothing beyond M x M
    if D <= 105 and M <= 17:
        assert np.array_equal(want, RN.pairwise_sqdist_loop(data[index]))


def test_pairwise_distances_of_misaligned_rows_and_clamped_indices():
    D = 4096
    data, _dev, all_pairs = distance_rows(D)
    framed = Framed(data[:9], offset=1)
    idx = dev_i32([2, 1, 8, 0, -4, 99])  # the last two are clamped to rows 0 and 8
    out = torch.zeros(36, dtype=torch.int64, device="cuda")
    call("ppo_replay_pairwise_sqdist_u8", ptr(framed.rows), 9, D, ptr(idx), 6, ptr(out))
    torch.cuda.synchronize()
    picked = [2, 1, 8, 0, 0, 8]
    assert np.array_equal(out.cpu().numpy().reshape(6, 6), all_pairs[np.ix_(picked, picked)]) and framed.intact()


# ---------------------------------------------------------------- the buffer class
@pytest.mark.parametrize("mode,max_size,thinning", [("uniform", 24, 1.0), ("sequential", 24, 1.0), ("overwrite", 24, 0.5),
                                                    ("sequential", 7, 1.0), ("uniform", 7, 1.0)])
@pytest.mark.parametrize("kind", ["uint8", "float32"])
def test_buffer_equals_the_numpy_restatement(mode, max_size, thinning, kind):
    """Eight adds of ten rows, from device tensors and from NumPy arrays alternately; uint8 images [1, 5, 21] (105 bytes)
    and float32 vectors [8] (rows are opaque bytes)."""
    shape, dtype = ((1, 5, 21), np.uint8) if kind == "uint8" else ((8,), np.float32)
    rng = np.random.default_rng(3)
    buf = replay.ExperienceReplayBuffer(max_size, shape, dtype, mode=mode, thinning=thinning, device="cuda")
    want = RN.NumpyReplay(max_size, shape, dtype, mode, thinning)
    assert buf.current_size == 0 and tuple(buf.data.shape) == (0, *shape) and tuple(buf.aux.shape) == (0, 16)
    for j in range(8):
        rows = rng.integers(0, 256, (10, *shape)).astype(dtype) if kind == "uint8" else rng.normal(size=(10, *shape)).astype(dtype)
        aux = buf.create_aux_buffer((10,), reward=rng.normal(size=10), time=rng.integers(0, 99, 10), action=rng.integers(0, 6, 10),
                                    step=np.arange(10) + 10 * j)
        np.random.seed(40 + j)
        want.add(rows, aux)
        after = np.random.rand()
        np.random.seed(40 + j)
        if j % 2:
            buf.add_experience(rows, aux)
        else:
            buf.add_experience(torch.from_numpy(rows).cuda(), torch.from_numpy(aux).cuda())
        assert np.random.rand() == after  # the same draws
        torch.cuda.synchronize()
        assert (buf.current_size, buf.experience_seen, buf.ring_buffer_location, buf.stats_last_entries_added,
                buf.stats_last_entries_submitted) == (len(want.data), want.seen, want.ring, want.added, want.submitted)
        assert buf.data.cpu().numpy().tobytes() == want.data.tobytes() and buf.aux.cpu().numpy().tobytes() == want.aux.tobytes()
    assert buf.data.dtype == (torch.uint8 if kind == "uint8" else torch.float32) and buf.data.is_cuda
    assert np.array_equal(buf.step.cpu().numpy(), want.aux[:, 4]) and np.array_equal(buf.time.cpu().numpy(), want.aux[:, 1])
    with pytest.raises(AssertionError, match="shape"):
        buf.add_experience(np.zeros((2, 3), dtype), np.zeros((2, 16)))
    with pytest.raises(AssertionError, match="dtype"):
        buf.add_experience(np.zeros((2, *shape), np.int16), np.zeros((2, 16)))


def test_diversity_estimate_and_log_keys():
    from ppo_amd import logger
    rng = np.random.default_rng(9)
    buf = replay.ExperienceReplayBuffer(200, (4, 12, 12), np.uint8, mode="sequential", device="cuda")
    rows = rng.integers(0, 256, (150, 4, 12, 12), dtype=np.uint8)
    rows[3], rows[4] = 0, 255
    buf.add_experience(rows, buf.create_aux_buffer((150,), step=np.arange(150) * 3))
    host = buf.data.cpu().numpy().reshape(150, -1)
    for m in (32, 128):
        np.random.seed(m)
        got = buf.estimate_replay_diversity(m)
        after = np.random.rand()
        np.random.seed(m)
        sample = np.random.choice(150, size=m, replace=False)  # rl/replay.py:94-98
        assert np.random.rand() == after
        want = replay.diversity_from_sqdist(RN.pairwise_sqdist(host[sample]))
        assert got == want and set(got) == {"mean", "k1", "k2", "k3", "k4", "k5"} and 0 < got["k1"] <= got["k5"]
    log = logger.Logger(quiet=True)
    np.random.seed(1)
    buf.log_stats(log)
    np.random.seed(1)
    want = replay.diversity_from_sqdist(RN.pairwise_sqdist(host[np.random.choice(150, size=128, replace=False)]))
    assert log["replay_diversity"] == want["mean"] and log["replay_density"] == want["k1"]
    for k in ("mean", "k1", "k2", "k3", "k4", "k5"):
        assert log[f"replay_diversity_{k}"] == want[k]
    assert log["replay_size"] == 150 and log["replay_last_entries_added"] == 150 and log["replay_log_time"] >= 0
    steps = (np.arange(150) * 3).astype(np.float32)  # what the float32 aux record holds
    assert log["rp_ks"] == replay.ks_uniform(steps / steps.max()) and log["rp_stats_max"] == 447.0 and "rp_stats_mean" in log
    with pytest.raises(ValueError, match="at most 128"):
        buf.estimate_replay_diversity(129)
    # float observations: the diversity keys are skipped, the rest is logged
    fbuf = replay.ExperienceReplayBuffer(8, (3,), np.float32, mode="sequential", device="cuda")
    fbuf.add_experience(rng.normal(size=(4, 3)).astype(np.float32), fbuf.create_aux_buffer((4,), step=np.arange(4)))
    flog = logger.Logger(quiet=True)
    fbuf.log_stats(flog)
    assert "replay_diversity" not in flog and flog["replay_size"] == 4 and "rp_ks" in flog
