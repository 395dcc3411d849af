"""CPU: the replay buffer's host side - the index plan of an add against the reference's own buffer
(tests/golden/replay_golden.npz, written by tests/golden/make_replay_golden.py from rl.replay.ExperienceReplayBuffer), the
last-write-wins de-duplication, the two logged statistics against scipy / float64 NumPy values recorded there, the `replay`
flag group, the checkpoint layout, and the argument checks of the three C entry points (they run before any HIP call)."""
import json
import os

import numpy as np
import pytest

import replay_numpy as RN
from ppo_amd.config import Config


@pytest.fixture(scope="module")
def golden(golden_dir):
    meta = json.load(open(os.path.join(golden_dir, "replay_golden.json")))
    return meta, np.load(os.path.join(golden_dir, "replay_golden.npz"))


def run_plan(meta, g, c):
    """The fixture's adds of case c through plan_add + last_write_wins, applied to NumPy arrays allocated once at max_size
    (as the device buffer is).  Returns what the fixture records."""
    from ppo_amd import replay
    case = meta["cases"][c]
    rows, aux_in = g[f"rows_{c}"], g[f"aux_in_{c}"]
    data = np.zeros((case["max_size"], *meta["obs"]), np.uint8)
    aux = np.zeros((case["max_size"], replay.ExperienceReplayBuffer.N_AUX), np.float32)
    state, counters, steps, collided = (0, 0, 0), [], [], []
    np.random.seed(meta["seed"] + c)
    for j in range(meta["adds"]):
        src, dst, state, added = replay.plan_add(state, len(rows[j]), case["mode"], case["max_size"], case["thinning"])
        assert src.dtype == dst.dtype == np.int64 and len(src) == len(dst)
        assert len(dst) == 0 or (0 <= dst.min() and dst.max() < state[0] and 0 <= src.min() and src.max() < len(rows[j]))
        kept_src, kept_dst = replay.last_write_wins(src, dst)
        collided.append(len(kept_dst) < len(dst))
        assert len(np.unique(kept_dst)) == len(kept_dst)  # what the scatter kernel assumes
        data[kept_dst] = rows[j][kept_src]  # (any order: the destinations are distinct)
        aux[kept_dst] = aux_in[j][kept_src]
        counters.append((*state, added, len(rows[j])))
        steps.append(data.copy())
    return data[:state[0]], aux[:state[0]], np.asarray(counters), np.asarray(steps), collided, np.random.rand()


@pytest.mark.parametrize("c", range(5))
def test_the_plan_reproduces_the_reference_buffer(golden, c):
    meta, g = golden
    assert len(meta["cases"]) == 5
    data, aux, counters, steps, _collided, rand = run_plan(meta, g, c)
    assert data.tobytes() == g[f"data_{c}"].tobytes() and data.shape == g[f"data_{c}"].shape
    assert aux.tobytes() == g[f"aux_{c}"].tobytes() and g[f"aux_{c}"].dtype == np.float32
    assert np.array_equal(counters, g[f"counters_{c}"])  # size, seen, ring, last added, last submitted after every add
    assert steps.tobytes() == g[f"data_steps_{c}"].tobytes()
    assert np.float64(rand).tobytes() == g[f"rand_{c}"].tobytes()  # the number and order of the draws


@pytest.mark.parametrize("c", range(5))
def test_the_numpy_restatement_reproduces_the_reference_buffer(golden, c):
    """tests/replay_numpy.py is what the GPU tests compare with: it is itself checked here."""
    meta, g = golden
    case = meta["cases"][c]
    buf = RN.NumpyReplay(case["max_size"], meta["obs"], np.uint8, case["mode"], case["thinning"])
    np.random.seed(meta["seed"] + c)
    for j in range(meta["adds"]):
        buf.add(g[f"rows_{c}"][j], g[f"aux_in_{c}"][j])
        assert (len(buf.data), buf.seen, buf.ring, buf.added, buf.submitted) == tuple(g[f"counters_{c}"][j])
        assert np.array_equal(buf.data, g[f"data_steps_{c}"][j][:len(buf.data)])
    assert buf.data.tobytes() == g[f"data_{c}"].tobytes() and buf.aux.tobytes() == g[f"aux_{c}"].tobytes()
    assert np.float64(np.random.rand()).tobytes() == g[f"rand_{c}"].tobytes()


def test_a_slot_written_twice_keeps_the_last_source(golden):
    from ppo_amd.replay import last_write_wins
    src, dst = last_write_wins(np.asarray([5, 6, 7, 8, 9]), np.asarray([2, 0, 2, 1, 0]))
    assert src.tolist() == [7, 8, 9] and dst.tolist() == [2, 1, 0]
    src, dst = last_write_wins(np.asarray([3, 4]), np.asarray([1, 0]))
    assert src.tolist() == [3, 4] and dst.tolist() == [1, 0]
    src, dst = last_write_wins(np.zeros(0, np.int64), np.zeros(0, np.int64))
    assert len(src) == len(dst) == 0
    # the fixture's cases: `uniform 24` grows the buffer in its third add and draws a slot it has just filled;
    # `sequential 7` and `uniform 7` take ten rows into seven slots.  Keeping the FIRST write instead gives another buffer.
    meta, g = golden
    collided = {c: run_plan(meta, g, c)[4] for c in (0, 1, 3)}
    assert collided[0][2] and not collided[0][0] and not collided[0][1]
    assert not any(collided[1])
    assert all(collided[3])  # rows 7 .. 9 of every add wrap round onto slots the same add has written


def test_first_write_wins_would_not_match(golden):
    from ppo_amd import replay
    meta, g = golden
    case = meta["cases"][0]
    data = np.zeros((case["max_size"], *meta["obs"]), np.uint8)
    state = (0, 0, 0)
    np.random.seed(meta["seed"])
    for j in range(3):
        src, dst, state, _ = replay.plan_add(state, 10, case["mode"], case["max_size"], case["thinning"])
        first = np.sort(np.unique(dst, return_index=True)[1])
        data[dst[first]] = g["rows_0"][j][src[first]]
    assert not np.array_equal(data, g["data_steps_0"][2])


def test_ks_statistic_matches_scipy(golden):
    from ppo_amd.replay import ks_uniform
    _meta, g = golden
    assert g["ks_x"].dtype == np.float32 and 0 < float(g["ks"]) < 1
    assert abs(ks_uniform(g["ks_x"]) - float(g["ks"])) <= 4 * np.finfo(np.float64).eps
    # closed forms: n points at (i + 1/2) / n are as uniform as n points get, D = 1 / (2n); all mass at one end, D = 1
    n = 50
    assert abs(ks_uniform((np.arange(n) + 0.5) / n) - 1 / (2 * n)) < 1e-15
    assert ks_uniform(np.ones(7)) == 1.0 and ks_uniform(np.zeros(7)) == 1.0


def test_diversity_arithmetic_matches_the_recorded_values(golden):
    from ppo_amd.replay import diversity_from_sqdist
    _meta, g = golden
    assert np.array_equal(RN.pairwise_sqdist(g["div_rows"]), g["div_d2"])
    assert np.array_equal(RN.pairwise_sqdist_loop(g["div_rows"]), g["div_d2"])
    d2 = g["div_d2"].copy()
    got = diversity_from_sqdist(d2)
    assert np.array_equal(d2, g["div_d2"])  # the input is left alone
    got = np.asarray([got["mean"]] + [got[f"k{k}"] for k in (1, 2, 3, 4, 5)])
    assert got.tobytes() == g["div_f64"].tobytes()  # float64 NumPy, the same expressions: the same bits
    # the reference's own numbers come from a float32 cdist: they agree to float32 rounding
    assert np.abs(got - g["div_ref"]).max() <= 8 * np.finfo(np.float32).eps * np.abs(g["div_ref"]).max()
    assert got[1] <= got[2] <= got[3] <= got[4] <= got[5]


def test_numpy_distances_are_exact_beyond_32_bits():
    x = np.zeros((3, 70000), np.uint8)
    x[1] = 255
    x[2, ::2] = 7
    d = RN.pairwise_sqdist(x)
    assert d.dtype == np.int64 and d[0, 1] == 255 * 255 * 70000 > 2 ** 32 and d[0, 2] == 49 * 35000
    assert d[1, 2] == 248 * 248 * 35000 + 255 * 255 * 35000 and np.array_equal(d, d.T) and not np.diagonal(d).any()


def test_replay_flags_defaults_and_parsed_values():
    c = Config().setup([])
    r = c.replay  # rl/config.py:362-365
    assert (r.mode, r.size, r.mixing, r.thinning, r.enabled) == ("off", 0, False, 1.0, False)
    assert "replay_mode" not in c.flatten()
    on = Config().setup(["--replay_mode=uniform", "--replay_size=64"])
    assert on._ignored == [] and on.replay.enabled is True
    assert (on.replay.mode, on.replay.size, on.replay.mixing, on.replay.thinning) == ("uniform", 64, False, 1.0)
    flat = on.flatten()
    assert flat["replay_mode"] == "uniform" and flat["replay_size"] == 64 and flat["replay_mixing"] is False
    full = Config().setup(["--replay_mode", "sequential", "--replay_size=8", "--replay_mixing", "--replay_thinning=0.5",
                           "--distil_batch_size=32"])
    assert full._ignored == [] and full.distil.batch_size == 32
    assert (full.replay.mode, full.replay.size, full.replay.mixing, full.replay.thinning) == ("sequential", 8, True, 0.5)
    for mode in ("overwrite", "sequential", "uniform"):
        assert Config().setup([f"--replay_mode={mode}", "--replay_size=1"]).replay.enabled


def test_a_line_without_a_replay_mode_parses_as_before():
    for line in (["--replay_size=64", "--agents=8"], ["--replay_mode=off", "--replay_size=64", "--replay_mixing=True", "--agents=8"],
                 ["--replay_thinning=0.5", "--agents=8"]):
        c = Config().setup(line)
        assert c._ignored == [a for a in line if a != "--agents=8"] and c.agents == 8
        assert c.replay.enabled is False and c.replay.size == 0 and c.replay.mode == "off" and c.replay.thinning == 1.0
    # a Config that parsed a replay line and then a plain one holds the defaults again
    c = Config()
    c.setup(["--replay_mode=uniform", "--replay_size=64", "--replay_mixing=True"])
    assert c.replay.enabled and c.replay.mixing
    c.setup([])
    assert (c.replay.mode, c.replay.size, c.replay.mixing, c.replay.thinning, c.replay.enabled) == ("off", 0, False, 1.0, False)
    assert "replay_size" not in c.flatten()


@pytest.mark.parametrize("line,match", [(["--replay_mode=prioritised", "--replay_size=8"], "replay mode"),
                                        (["--replay_mode=uniform"], "replay_size"),
                                        (["--replay_mode=uniform", "--replay_size=0"], "replay_size"),
                                        (["--replay_mode=uniform", "--replay_size=-4"], "replay_size"),
                                        (["--replay_mode=uniform", "--replay_size=8", "--replay_thinning=0"], "thinning"),
                                        (["--replay_mode=uniform", "--replay_size=8", "--replay_thinning=1.5"], "thinning"),
                                        (["--replay_mode=uniform", "--replay_size=8", "--replay_thinning=-0.1"], "thinning")])
def test_verify_refuses_bad_replay_flags(line, match):
    with pytest.raises(ValueError, match=match):
        Config().setup(line)


def test_a_buffer_on_the_cpu_is_refused():
    from ppo_amd import _lib, replay
    for device in ("cpu", "meta"):
        with pytest.raises(_lib.PpoAmdError, match="no CPU path"):
            replay.ExperienceReplayBuffer(8, (1, 2, 2), np.uint8, device=device)


def test_names_the_reference_exposes():
    import rl.replay
    from ppo_amd import replay
    B = replay.ExperienceReplayBuffer
    assert rl.replay.ExperienceReplayBuffer is B and rl.replay.smart_sample is replay.smart_sample
    assert (B.N_AUX, B.AUX_HASH, B.AUX_TIME, B.AUX_REWARD, B.AUX_ACTION, B.AUX_STEP, B.AUX_VTARG) == (16, 0, 1, 2, 3, 4, 5)
    for name in ("add_experience", "create_aux_buffer", "save_state", "load_state", "estimate_replay_diversity", "log_stats",
                 "current_size", "step", "time", "data", "aux"):
        assert hasattr(B, name), name
    aux = B.create_aux_buffer((2, 3), reward=np.ones((2, 3)), time=np.full((2, 3), 4), action=np.full((2, 3, 2), 5),
                              step=np.arange(6).reshape(2, 3))
    assert aux.shape == (2, 3, 16) and aux.dtype == np.float64
    assert (aux[..., 2] == 1).all() and (aux[..., 1] == 4).all() and (aux[..., 3] == 5).all() and aux[1, 2, 4] == 5
    assert not aux[..., 0].any() and not aux[..., 5:].any()
    np.random.seed(0)
    s = replay.smart_sample(np.arange(5), 12)  # two whole passes, then two more
    assert len(s) == 12 and sorted(s[:5]) == sorted(s[5:10]) == [0, 1, 2, 3, 4] and len(set(s[10:])) == 2
    np.random.seed(0)
    again = np.concatenate([np.random.choice(np.arange(5), size=[k], replace=False) for k in (5, 5, 2)])
    assert np.array_equal(s, again)


def _HostBuffer(max_size, obs_shape):
    """An ExperienceReplayBuffer whose two arrays are host tensors, put together without its constructor (which wants a
    device): save_state / load_state touch nothing but the arrays and the counters, so they run here."""
    import torch
    from ppo_amd.replay import ExperienceReplayBuffer as B
    b = B.__new__(B)
    b.max_size, b.obs_shape, b.obs_dtype = max_size, tuple(obs_shape), torch.uint8
    b._data = torch.zeros((max_size, *obs_shape), dtype=torch.uint8)
    b._aux = torch.zeros((max_size, B.N_AUX), dtype=torch.float32)
    b._size = b.experience_seen = b.ring_buffer_location = 0
    b.name, b.thinning = "replay", 1.0
    return b


def test_checkpoint_round_trip_of_the_reference_layout(golden, tmp_path):
    import torch
    from ppo_amd import checkpoint
    meta, g = golden
    a = _HostBuffer(24, meta["obs"])
    n = len(g["data_0"])
    a._data[:n] = torch.from_numpy(g["data_0"])
    a._aux[:n] = torch.from_numpy(g["aux_0"])
    a._size, a.experience_seen, a.ring_buffer_location, a.thinning = n, 80, 37, 0.5
    state = a.save_state()
    assert set(state) == {"max_size", "experience_seen", "ring_buffer_location", "data", "aux", "name", "thinning"}  # rl/replay.py:65-74
    assert isinstance(state["data"], np.ndarray) and state["data"].dtype == np.uint8 and state["data"].shape == (n, 1, 2, 2)
    assert isinstance(state["aux"], np.ndarray) and state["aux"].dtype == np.float32 and state["aux"].shape == (n, 16)
    for compress in (False, True):
        path = checkpoint.save({"step": 3, "replay_buffer": state}, str(tmp_path / f"cp{int(compress)}.pt"), compress)
        back = checkpoint.load(path)["replay_buffer"]
        assert back["data"].tobytes() == g["data_0"].tobytes() and back["aux"].tobytes() == g["aux_0"].tobytes()
        assert (back["max_size"], back["experience_seen"], back["ring_buffer_location"], back["name"], back["thinning"]) == \
            (24, 80, 37, "replay", 0.5)
        b = _HostBuffer(24, meta["obs"])
        b.load_state(back)
        assert (b.current_size, b.experience_seen, b.ring_buffer_location, b.thinning) == (n, 80, 37, 0.5)
        assert torch.equal(b.data, a.data) and torch.equal(b.aux, a.aux) and tuple(b.data.shape) == (n, 1, 2, 2)
        assert torch.equal(b.step, a.aux[:, 4]) and torch.equal(b.time, a.aux[:, 1])
    with pytest.raises(ValueError, match="--replay_size"):
        _HostBuffer(32, meta["obs"]).load_state(state)


def test_argument_validation_needs_no_gpu(hip_lib):
    one = 1 << 12  # any non-null, 16-byte aligned address: the checks return before anything is read
    err = lambda: hip_lib.ppo_last_error()  # noqa: E731
    scatter = lambda src=one, aux=one, n_src=4, rb=16, ids=one, spot=one, n=2, dst=one, daux=one, n_dst=8: (  # noqa: E731
        src, aux, n_src, rb, ids, spot, n, dst, daux, n_dst, None)
    for kw in ({"rb": 0}, {"n": -1}, {"n_src": 0}, {"n_dst": 0}):
        assert hip_lib.ppo_replay_scatter_rows(*scatter(**kw)) == -1
        assert b"ppo_replay_scatter_rows" in err() and b"bad shape" in err()
    for kw in ({"src": None}, {"ids": None}, {"spot": None}, {"dst": None}, {"aux": None}, {"daux": None}):
        assert hip_lib.ppo_replay_scatter_rows(*scatter(**kw)) == -1 and b"null" in err()
    assert hip_lib.ppo_replay_scatter_rows(*scatter(aux=one + 2)) == -3 and b"aligned" in err()
    assert hip_lib.ppo_replay_scatter_rows(*scatter(n=0, src=None)) == 0  # nothing to move

    gather = lambda a=one, aa=one, n_a=4, b=one, ba=one, n_b=4, rb=16, s=one, n=2, dst=one, daux=one: (  # noqa: E731
        a, aa, n_a, b, ba, n_b, rb, s, n, dst, daux, None)
    for kw in ({"rb": 0}, {"n": -1}, {"n_a": -1}, {"n_b": -1}, {"n_a": 0, "n_b": 0}):
        assert hip_lib.ppo_replay_gather_rows2(*gather(**kw)) == -1
        assert b"ppo_replay_gather_rows2" in err() and b"bad shape" in err()
    for kw in ({"a": None}, {"b": None}, {"s": None}, {"dst": None}, {"aa": None}, {"ba": None}):
        assert hip_lib.ppo_replay_gather_rows2(*gather(**kw)) == -1 and b"null" in err()
    assert hip_lib.ppo_replay_gather_rows2(*gather(daux=one + 1)) == -3 and b"aligned" in err()
    assert hip_lib.ppo_replay_gather_rows2(*gather(n=0, a=None)) == 0

    pair = lambda data=one, rows=4, d=16, idx=one, m=2, out=one: (data, rows, d, idx, m, out, None)  # noqa: E731
    for kw in ({"rows": 0}, {"d": 0}, {"m": -1}, {"m": 129}):
        assert hip_lib.ppo_replay_pairwise_sqdist_u8(*pair(**kw)) == -1
        assert b"ppo_replay_pairwise_sqdist_u8" in err() and b"bad shape" in err()
    for kw in ({"data": None}, {"idx": None}, {"out": None}):
        assert hip_lib.ppo_replay_pairwise_sqdist_u8(*pair(**kw)) == -1 and b"null" in err()
    assert hip_lib.ppo_replay_pairwise_sqdist_u8(*pair(out=one + 4)) == -3 and b"aligned" in err()
    assert hip_lib.ppo_replay_pairwise_sqdist_u8(*pair(m=0, data=None)) == 0
