#!/usr/bin/env python3
"""Generate tests/golden/replay_golden.npz / .json: the REFERENCE's replay buffer on the CPU.

Build container only (needs the reference checkout; see ref_shim.py):  python tests/golden/make_replay_golden.py

Everything about the buffer comes from the reference's own rl.replay.ExperienceReplayBuffer: for each case a fresh buffer,
np.random.seed(seed + case), ADDS adds of ROWS rows of OBS uint8 observations with aux records from its create_aux_buffer
(reward, time, action, step), then one np.random.rand() - the position of the host RNG stream after the run, which pins
the number and order of the draws.  Cases (mode, max_size, thinning):
    uniform 24, sequential 24, overwrite 24 with thinning 0.5, sequential 7 and uniform 7 (fewer slots than rows per add).
Stored per case c: the submitted rows and aux records (`rows_c`, `aux_in_c`), the final `data_c` / `aux_c`, and after every
add the three counters, the buffer size and stats_last_entries_added (`counters_c` [ADDS, 5] = size, experience_seen,
ring_buffer_location, last_entries_added, last_entries_submitted), the buffer after every add (`data_steps_c`
[ADDS, max_size, *OBS], zero beyond the live rows), and `rand_c`.

The seed is the first from SEED upwards for which the `uniform 24` case writes a slot twice within one add (it grows the
buffer and then draws a slot it has just filled): the result then shows that the later write stands (writes_a_slot_twice reads it off
the buffer as it stands after the third add).

Also stored, for the two statistics of log_stats:
  * `ks_x` (the uniform-24 buffer's step / max(step)) and `ks` = scipy.stats.kstest(ks_x, uniform.cdf).statistic;
  * `div_rows` (uint8 [8, 4]: eight rows of that buffer drawn by estimate_replay_diversity(8) under np.random.seed(DIV_SEED)),
    `div_d2` their squared distances in int64, `div_f64` = (mean, k1 .. k5) in float64 NumPy from div_d2 - sqrt(d2) / 255,
    the mean with the diagonal, np.sort(d, axis=0)[:k].mean() with the diagonal at infinity - and `div_ref`, the same six
    numbers as the reference's own float32 torch.cdist gives them.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
SEED, DIV_SEED, ADDS, ROWS, OBS = 1, 77, 8, 10, (1, 2, 2)
CASES = (("uniform", 24, 1.0), ("sequential", 24, 1.0), ("overwrite", 24, 0.5), ("sequential", 7, 1.0), ("uniform", 7, 1.0))


def run_case(ref_replay, case, seed):
    mode, max_size, thinning = CASES[case]
    rng = np.random.default_rng(1000 * seed + case)
    rows = rng.integers(0, 256, (ADDS, ROWS, *OBS), dtype=np.uint8)
    buf = ref_replay.ExperienceReplayBuffer(max_size, OBS, np.uint8, mode=mode, thinning=thinning)
    aux_in = np.zeros((ADDS, ROWS, buf.N_AUX), np.float64)
    counters = np.zeros((ADDS, 5), np.int64)
    data_steps = np.zeros((ADDS, max_size, *OBS), np.uint8)
    np.random.seed(seed + case)
    for j in range(ADDS):
        aux_in[j] = buf.create_aux_buffer((ROWS,), reward=rng.normal(size=ROWS).astype(np.float32),
                                          time=rng.integers(0, 500, ROWS), action=rng.integers(0, 6, ROWS),
                                          step=np.arange(ROWS) + j * ROWS)
        buf.add_experience(rows[j], aux_in[j])
        data_steps[j, :buf.current_size] = buf.data
        counters[j] = (buf.current_size, buf.experience_seen, buf.ring_buffer_location, buf.stats_last_entries_added,
                       buf.stats_last_entries_submitted)
    return buf, {"rows": rows, "aux_in": aux_in, "data": buf.data.copy(), "aux": buf.aux.copy(), "counters": counters,
                 "data_steps": data_steps, "rand": np.float64(np.random.rand())}


def writes_a_slot_twice(rows, data_after_third_add):
    """Read off the result alone: in the `uniform 24` case the third add grows the buffer by four slots (20 .. 23), filled
    in ascending source order, and then places four more rows - later in source order - in drawn slots.  If the sources
    found in slots 20 .. 23 afterwards are not ascending, one of those slots was written twice and holds the later row."""
    third = rows[2].reshape(ROWS, -1)
    grown = data_after_third_add[20:24].reshape(4, -1)
    where = [int(np.flatnonzero((third == g).all(1))[0]) for g in grown]
    return where != sorted(where)


def main():
    from ref_shim import load_reference
    load_reference(["--device=cpu", "--output_folder=/tmp/ref_golden_out"])
    import scipy.stats
    from rl import replay as ref_replay

    for seed in range(SEED, SEED + 64):
        first, rec = run_case(ref_replay, 0, seed)
        if writes_a_slot_twice(rec["rows"], rec["data_steps"][2]):
            break
    else:
        raise SystemExit("no seed found")
    out = {}
    for c in range(len(CASES)):
        buf, rec = run_case(ref_replay, c, seed)
        for k, v in rec.items():
            out[f"{k}_{c}"] = v
        if c == 0:
            first = buf
    x = first.step / max(first.step)
    out["ks_x"] = np.asarray(x)
    out["ks"] = np.float64(scipy.stats.kstest(rvs=x, cdf=scipy.stats.uniform.cdf).statistic)
    np.random.seed(DIV_SEED)
    ref = first.estimate_replay_diversity(8)
    np.random.seed(DIV_SEED)
    sample = np.random.choice(first.current_size, size=8, replace=False)
    picked = first.data[sample].reshape(8, -1)
    wide = picked.astype(np.int64)
    d2 = ((wide[:, None, :] - wide[None, :, :]) ** 2).sum(-1)
    d = np.sqrt(d2.astype(np.float64)) / 255
    f64 = [d.mean()]
    np.fill_diagonal(d, np.inf)
    f64 += [np.sort(d, axis=0)[:k].mean() for k in (1, 2, 3, 4, 5)]
    out["div_sample"], out["div_rows"], out["div_d2"] = sample, picked, d2
    out["div_f64"] = np.asarray(f64, np.float64)
    out["div_ref"] = np.asarray([ref["mean"]] + [ref[f"k{k}"] for k in (1, 2, 3, 4, 5)], np.float64)
    meta = {"seed": seed, "div_seed": DIV_SEED, "adds": ADDS, "rows": ROWS, "obs": list(OBS),
            "cases": [{"mode": m, "max_size": s, "thinning": t} for m, s, t in CASES],
            "counters": ["size", "experience_seen", "ring_buffer_location", "last_entries_added", "last_entries_submitted"]}
    np.savez_compressed(os.path.join(HERE, "replay_golden.npz"), **out)
    with open(os.path.join(HERE, "replay_golden.json"), "w") as f:
        json.dump(meta, f, separators=(",", ":"))
    print(f"seed {seed}: {len(CASES)} cases, ks {float(out['ks']):.6f}, diversity f64 {out['div_f64']}, ref {out['div_ref']}, "
          f"{os.path.getsize(os.path.join(HERE, 'replay_golden.npz'))} + "
          f"{os.path.getsize(os.path.join(HERE, 'replay_golden.json'))} bytes")


if __name__ == "__main__":
    main()
