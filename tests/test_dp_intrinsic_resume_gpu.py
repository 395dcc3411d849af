"""GPU: checkpoints with RND and state hashing on, under data parallelism (two ranks sharing the one GPU over gloo, as in
tests/test_dp_gpu.py).

The hash tables, `ems_norm` and the `intrinsic_returns_rms` moments are global state - identical on every rank, written
once by rank 0 and restored on every rank - next to the replicas (policy net, predictor, their Adam moments); the env
columns, the reward bookkeeping and the host RNG stay per rank.  A run that is interrupted after its first iteration and
resumed from the checkpoint by a fresh pair of ranks (started from other seeds) must end its second iteration where the
uninterrupted run does, digest for digest, on both ranks.

A one-rank checkpoint keeps the key tree it had before data parallelism reached these modules: PARENT_KEYS is the nested
key set a one-rank run with these flags wrote at the parent commit, recorded here as a literal."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WORKER = r'''
import os, sys, hashlib, json
sys.path.insert(0, sys.argv[1])
import numpy as np, torch, torch.distributed as dist
from ppo_amd import envs, logger, models, rollout
from ppo_amd.config import args
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
torch.cuda.set_device(0)
if world > 1:
    dist.init_process_group("gloo", rank=rank, world_size=world)
# 16 envs in all: 8 per rank, or the one-rank run's 16 (its RND rows then fill one minibatch of 16, as the two ranks' do)
args.setup([f"--agents={16 // world}", "--n_steps=4", "--model_architecture=single", "--model_encoder=nature",
            "--env_type=synthetic", "--env_embed_time=False", "--seed=3", "--device=cuda", "--policy_opt_mini_batch_size=32",
            "--rnd_opt_mini_batch_size=16", "--disable_logging=True", "--rnd_enabled=True",
            "--observation_normalization=True", "--ir_normalize=True", "--ir_center=True", "--hash_enabled=True",
            "--hash_bonus=0.01", "--hash_bits=8", "--hash_input=raw", "--checkpoint_compression=False"])


def make_runner(seed):
    torch.manual_seed(seed + rank)
    np.random.seed(seed // 10 + rank)
    shape, nA = envs.get_env_spec()
    model = models.TVFModel("nature", input_dims=shape, actions=nA, device="cuda", architecture="single", hidden_units=256,
                            head_scale=0.1, head_bias=True, use_rnd=True, observation_normalization=True,
                            value_head_names=("ext", "int"))
    r = rollout.Runner(model, logger.Logger(quiet=True))
    r.vec_env = envs.create_envs_classic(rank=rank, world=world)
    r.reset()
    return r


def iteration(r):
    r.generate_rollout()
    r.calculate_returns()
    r.train()


def digests(r):
    torch.cuda.synchronize()

    def d(*arrays):
        h = hashlib.sha256()
        for a in arrays:
            if a is None:  # Adam moments that no step has allocated yet
                continue
            h.update(a.detach().cpu().contiguous().numpy().tobytes() if isinstance(a, torch.Tensor)
                     else np.ascontiguousarray(a).tobytes())
        return h.hexdigest()
    m = r.intrinsic_returns_rms
    return {"policy": d(r.net.flat, r.net.exp_avg, r.net.exp_avg_sq),
            "predictor": d(r.rnd.prediction_net.flat, r.rnd.exp_avg, r.rnd.exp_avg_sq, r.rnd.target_net.flat),
            "hash_tables": d(r.hash.global_counts, r.hash.recent_counts),
            "ems_norm": d(np.asarray(r.ems_norm, np.float64)),
            "intrinsic_returns_rms": d(np.asarray([m.mean, m.var, m.count], np.float64)),
            "int_rewards": d(r.int_rewards), "ems_len": len(r.ems_norm), "rnd_adam_steps": r.rnd.adam_steps,
            "step": r.step}


path = os.path.join(sys.argv[2], f"checkpoint-w{world}.pt")
a = make_runner(1000)
iteration(a)
written = a.save_checkpoint(path, a.step)   # a collective under world > 1: every rank calls it, rank 0 writes
assert (written == path) if rank == 0 else (written is None)
result = {"after_one": digests(a)}
if world > 1:
    iteration(a)
    result["uninterrupted"] = digests(a)
    dist.barrier()                          # the file stands before anyone reads it
    b = make_runner(5000)                   # other initial weights, another host RNG state
    result["fresh"] = digests(b)
    assert b.load_checkpoint(path) == 4 * 16
    b.sync_replicas()                       # as ppo.train does after a restore
    result["restored"] = digests(b)
    iteration(b)
    result["resumed"] = digests(b)
    dist.barrier(); dist.destroy_process_group()
with open(os.path.join(sys.argv[2], f"w{world}_r{rank}.json"), "w") as f:
    json.dump(result, f)
print("rank", rank, "ok")
'''

# the nested keys of a one-rank checkpoint written with the worker's flags at the parent commit ("a/b": key b of the
# dict under key a; "[i]": element i of a list that holds containers)
PARENT_KEYS = [
    "step", "ep_count", "batch_counter", "episode_length_buffer", "model_state_dict",
    "model_state_dict/policy_net.log_std", "model_state_dict/policy_net.encoder.conv1.weight",
    "model_state_dict/policy_net.encoder.conv1.bias", "model_state_dict/policy_net.encoder.conv2.weight",
    "model_state_dict/policy_net.encoder.conv2.bias", "model_state_dict/policy_net.encoder.conv3.weight",
    "model_state_dict/policy_net.encoder.conv3.bias", "model_state_dict/policy_net.encoder.fc.weight",
    "model_state_dict/policy_net.encoder.fc.bias", "model_state_dict/policy_net.policy_head.weight",
    "model_state_dict/policy_net.policy_head.bias", "model_state_dict/policy_net.value_head.weight",
    "model_state_dict/policy_net.value_head.bias", "model_state_dict/policy_net.advantage_head.weight",
    "model_state_dict/policy_net.advantage_head.bias", "model_state_dict/value_net.log_std",
    "model_state_dict/value_net.encoder.conv1.weight", "model_state_dict/value_net.encoder.conv1.bias",
    "model_state_dict/value_net.encoder.conv2.weight", "model_state_dict/value_net.encoder.conv2.bias",
    "model_state_dict/value_net.encoder.conv3.weight", "model_state_dict/value_net.encoder.conv3.bias",
    "model_state_dict/value_net.encoder.fc.weight", "model_state_dict/value_net.encoder.fc.bias",
    "model_state_dict/value_net.policy_head.weight", "model_state_dict/value_net.policy_head.bias",
    "model_state_dict/value_net.value_head.weight", "model_state_dict/value_net.value_head.bias",
    "model_state_dict/value_net.advantage_head.weight", "model_state_dict/value_net.advantage_head.bias",
    "model_state_dict/prediction_net.conv1.weight", "model_state_dict/prediction_net.conv1.bias",
    "model_state_dict/prediction_net.conv2.weight", "model_state_dict/prediction_net.conv2.bias",
    "model_state_dict/prediction_net.conv3.weight", "model_state_dict/prediction_net.conv3.bias",
    "model_state_dict/prediction_net.fc1.weight", "model_state_dict/prediction_net.fc1.bias",
    "model_state_dict/prediction_net.fc2.weight", "model_state_dict/prediction_net.fc2.bias",
    "model_state_dict/prediction_net.out.weight", "model_state_dict/prediction_net.out.bias",
    "model_state_dict/target_net.conv1.weight", "model_state_dict/target_net.conv1.bias",
    "model_state_dict/target_net.conv2.weight", "model_state_dict/target_net.conv2.bias",
    "model_state_dict/target_net.conv3.weight", "model_state_dict/target_net.conv3.bias",
    "model_state_dict/target_net.out.weight", "model_state_dict/target_net.out.bias", "reward_scale", "episode_score",
    "world", "sample_calls", "device_seed", "rank_state", "rank_state[0]/np_random", "rank_state[0]/ep_count",
    "rank_state[0]/time", "rank_state[0]/episode_score", "rank_state[0]/episode_len", "rank_state[0]/env_state",
    "rank_state[0]/env_state/SyntheticVecEnv", "rank_state[0]/env_state/SyntheticVecEnv/steps",
    "rank_state[0]/env_state/SyntheticVecEnv/time", "rank_state[0]/env_state/SyntheticVecEnv/score",
    "policy_optimizer_state_dict", "policy_optimizer_state_dict/state", "policy_optimizer_state_dict/state/1",
    "policy_optimizer_state_dict/state/1/step", "policy_optimizer_state_dict/state/1/exp_avg",
    "policy_optimizer_state_dict/state/1/exp_avg_sq", "policy_optimizer_state_dict/state/2",
    "policy_optimizer_state_dict/state/2/step", "policy_optimizer_state_dict/state/2/exp_avg",
    "policy_optimizer_state_dict/state/2/exp_avg_sq", "policy_optimizer_state_dict/state/3",
    "policy_optimizer_state_dict/state/3/step", "policy_optimizer_state_dict/state/3/exp_avg",
    "policy_optimizer_state_dict/state/3/exp_avg_sq", "policy_optimizer_state_dict/state/4",
    "policy_optimizer_state_dict/state/4/step", "policy_optimizer_state_dict/state/4/exp_avg",
    "policy_optimizer_state_dict/state/4/exp_avg_sq", "policy_optimizer_state_dict/state/5",
    "policy_optimizer_state_dict/state/5/step", "policy_optimizer_state_dict/state/5/exp_avg",
    "policy_optimizer_state_dict/state/5/exp_avg_sq", "policy_optimizer_state_dict/state/6",
    "policy_optimizer_state_dict/state/6/step", "policy_optimizer_state_dict/state/6/exp_avg",
    "policy_optimizer_state_dict/state/6/exp_avg_sq", "policy_optimizer_state_dict/state/7",
    "policy_optimizer_state_dict/state/7/step", "policy_optimizer_state_dict/state/7/exp_avg",
    "policy_optimizer_state_dict/state/7/exp_avg_sq", "policy_optimizer_state_dict/state/8",
    "policy_optimizer_state_dict/state/8/step", "policy_optimizer_state_dict/state/8/exp_avg",
    "policy_optimizer_state_dict/state/8/exp_avg_sq", "policy_optimizer_state_dict/state/9",
    "policy_optimizer_state_dict/state/9/step", "policy_optimizer_state_dict/state/9/exp_avg",
    "policy_optimizer_state_dict/state/9/exp_avg_sq", "policy_optimizer_state_dict/state/10",
    "policy_optimizer_state_dict/state/10/step", "policy_optimizer_state_dict/state/10/exp_avg",
    "policy_optimizer_state_dict/state/10/exp_avg_sq", "policy_optimizer_state_dict/state/11",
    "policy_optimizer_state_dict/state/11/step", "policy_optimizer_state_dict/state/11/exp_avg",
    "policy_optimizer_state_dict/state/11/exp_avg_sq", "policy_optimizer_state_dict/state/12",
    "policy_optimizer_state_dict/state/12/step", "policy_optimizer_state_dict/state/12/exp_avg",
    "policy_optimizer_state_dict/state/12/exp_avg_sq", "policy_optimizer_state_dict/param_groups",
    "policy_optimizer_state_dict/param_groups[0]/lr", "policy_optimizer_state_dict/param_groups[0]/betas",
    "policy_optimizer_state_dict/param_groups[0]/eps", "policy_optimizer_state_dict/param_groups[0]/weight_decay",
    "policy_optimizer_state_dict/param_groups[0]/amsgrad", "policy_optimizer_state_dict/param_groups[0]/maximize",
    "policy_optimizer_state_dict/param_groups[0]/foreach", "policy_optimizer_state_dict/param_groups[0]/capturable",
    "policy_optimizer_state_dict/param_groups[0]/params", "value_optimizer_state_dict",
    "value_optimizer_state_dict/state", "value_optimizer_state_dict/state/1", "value_optimizer_state_dict/state/1/step",
    "value_optimizer_state_dict/state/1/exp_avg", "value_optimizer_state_dict/state/1/exp_avg_sq",
    "value_optimizer_state_dict/state/2", "value_optimizer_state_dict/state/2/step",
    "value_optimizer_state_dict/state/2/exp_avg", "value_optimizer_state_dict/state/2/exp_avg_sq",
    "value_optimizer_state_dict/state/3", "value_optimizer_state_dict/state/3/step",
    "value_optimizer_state_dict/state/3/exp_avg", "value_optimizer_state_dict/state/3/exp_avg_sq",
    "value_optimizer_state_dict/state/4", "value_optimizer_state_dict/state/4/step",
    "value_optimizer_state_dict/state/4/exp_avg", "value_optimizer_state_dict/state/4/exp_avg_sq",
    "value_optimizer_state_dict/state/5", "value_optimizer_state_dict/state/5/step",
    "value_optimizer_state_dict/state/5/exp_avg", "value_optimizer_state_dict/state/5/exp_avg_sq",
    "value_optimizer_state_dict/state/6", "value_optimizer_state_dict/state/6/step",
    "value_optimizer_state_dict/state/6/exp_avg", "value_optimizer_state_dict/state/6/exp_avg_sq",
    "value_optimizer_state_dict/state/7", "value_optimizer_state_dict/state/7/step",
    "value_optimizer_state_dict/state/7/exp_avg", "value_optimizer_state_dict/state/7/exp_avg_sq",
    "value_optimizer_state_dict/state/8", "value_optimizer_state_dict/state/8/step",
    "value_optimizer_state_dict/state/8/exp_avg", "value_optimizer_state_dict/state/8/exp_avg_sq",
    "value_optimizer_state_dict/state/9", "value_optimizer_state_dict/state/9/step",
    "value_optimizer_state_dict/state/9/exp_avg", "value_optimizer_state_dict/state/9/exp_avg_sq",
    "value_optimizer_state_dict/state/10", "value_optimizer_state_dict/state/10/step",
    "value_optimizer_state_dict/state/10/exp_avg", "value_optimizer_state_dict/state/10/exp_avg_sq",
    "value_optimizer_state_dict/state/11", "value_optimizer_state_dict/state/11/step",
    "value_optimizer_state_dict/state/11/exp_avg", "value_optimizer_state_dict/state/11/exp_avg_sq",
    "value_optimizer_state_dict/state/12", "value_optimizer_state_dict/state/12/step",
    "value_optimizer_state_dict/state/12/exp_avg", "value_optimizer_state_dict/state/12/exp_avg_sq",
    "value_optimizer_state_dict/param_groups", "value_optimizer_state_dict/param_groups[0]/lr",
    "value_optimizer_state_dict/param_groups[0]/betas", "value_optimizer_state_dict/param_groups[0]/eps",
    "value_optimizer_state_dict/param_groups[0]/weight_decay", "value_optimizer_state_dict/param_groups[0]/amsgrad",
    "value_optimizer_state_dict/param_groups[0]/maximize", "value_optimizer_state_dict/param_groups[0]/foreach",
    "value_optimizer_state_dict/param_groups[0]/capturable", "value_optimizer_state_dict/param_groups[0]/params",
    "distil_optimizer_state_dict", "distil_optimizer_state_dict/state", "distil_optimizer_state_dict/param_groups",
    "distil_optimizer_state_dict/param_groups[0]/lr", "distil_optimizer_state_dict/param_groups[0]/betas",
    "distil_optimizer_state_dict/param_groups[0]/eps", "distil_optimizer_state_dict/param_groups[0]/weight_decay",
    "distil_optimizer_state_dict/param_groups[0]/amsgrad", "distil_optimizer_state_dict/param_groups[0]/maximize",
    "distil_optimizer_state_dict/param_groups[0]/foreach", "distil_optimizer_state_dict/param_groups[0]/capturable",
    "distil_optimizer_state_dict/param_groups[0]/params", "rnd_optimizer_state_dict", "rnd_optimizer_state_dict/state",
    "rnd_optimizer_state_dict/state/0", "rnd_optimizer_state_dict/state/0/step",
    "rnd_optimizer_state_dict/state/0/exp_avg", "rnd_optimizer_state_dict/state/0/exp_avg_sq",
    "rnd_optimizer_state_dict/state/1", "rnd_optimizer_state_dict/state/1/step",
    "rnd_optimizer_state_dict/state/1/exp_avg", "rnd_optimizer_state_dict/state/1/exp_avg_sq",
    "rnd_optimizer_state_dict/state/2", "rnd_optimizer_state_dict/state/2/step",
    "rnd_optimizer_state_dict/state/2/exp_avg", "rnd_optimizer_state_dict/state/2/exp_avg_sq",
    "rnd_optimizer_state_dict/state/3", "rnd_optimizer_state_dict/state/3/step",
    "rnd_optimizer_state_dict/state/3/exp_avg", "rnd_optimizer_state_dict/state/3/exp_avg_sq",
    "rnd_optimizer_state_dict/state/4", "rnd_optimizer_state_dict/state/4/step",
    "rnd_optimizer_state_dict/state/4/exp_avg", "rnd_optimizer_state_dict/state/4/exp_avg_sq",
    "rnd_optimizer_state_dict/state/5", "rnd_optimizer_state_dict/state/5/step",
    "rnd_optimizer_state_dict/state/5/exp_avg", "rnd_optimizer_state_dict/state/5/exp_avg_sq",
    "rnd_optimizer_state_dict/state/6", "rnd_optimizer_state_dict/state/6/step",
    "rnd_optimizer_state_dict/state/6/exp_avg", "rnd_optimizer_state_dict/state/6/exp_avg_sq",
    "rnd_optimizer_state_dict/state/7", "rnd_optimizer_state_dict/state/7/step",
    "rnd_optimizer_state_dict/state/7/exp_avg", "rnd_optimizer_state_dict/state/7/exp_avg_sq",
    "rnd_optimizer_state_dict/state/8", "rnd_optimizer_state_dict/state/8/step",
    "rnd_optimizer_state_dict/state/8/exp_avg", "rnd_optimizer_state_dict/state/8/exp_avg_sq",
    "rnd_optimizer_state_dict/state/9", "rnd_optimizer_state_dict/state/9/step",
    "rnd_optimizer_state_dict/state/9/exp_avg", "rnd_optimizer_state_dict/state/9/exp_avg_sq",
    "rnd_optimizer_state_dict/state/10", "rnd_optimizer_state_dict/state/10/step",
    "rnd_optimizer_state_dict/state/10/exp_avg", "rnd_optimizer_state_dict/state/10/exp_avg_sq",
    "rnd_optimizer_state_dict/state/11", "rnd_optimizer_state_dict/state/11/step",
    "rnd_optimizer_state_dict/state/11/exp_avg", "rnd_optimizer_state_dict/state/11/exp_avg_sq",
    "rnd_optimizer_state_dict/param_groups", "rnd_optimizer_state_dict/param_groups[0]/lr",
    "rnd_optimizer_state_dict/param_groups[0]/betas", "rnd_optimizer_state_dict/param_groups[0]/eps",
    "rnd_optimizer_state_dict/param_groups[0]/weight_decay", "rnd_optimizer_state_dict/param_groups[0]/amsgrad",
    "rnd_optimizer_state_dict/param_groups[0]/maximize", "rnd_optimizer_state_dict/param_groups[0]/foreach",
    "rnd_optimizer_state_dict/param_groups[0]/capturable", "rnd_optimizer_state_dict/param_groups[0]/params", "obs_rms",
    "obs_rms/mean", "obs_rms/var", "obs_rms/count", "ems_norm", "intrinsic_returns_rms", "intrinsic_returns_rms/mean",
    "intrinsic_returns_rms/var", "intrinsic_returns_rms/count", "hash_global_counts", "hash_recent_counts"
]


def key_paths(v, prefix=""):
    out = []
    if isinstance(v, dict):
        for k, x in v.items():
            p = f"{prefix}/{k}" if prefix else str(k)
            out.append(p)
            out += key_paths(x, p)
    elif isinstance(v, (list, tuple)) and any(isinstance(x, (dict, list, tuple)) for x in v):
        for i, x in enumerate(v):
            out += key_paths(x, f"{prefix}[{i}]")
    return out


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """(folder, one-rank record, [rank 0's, rank 1's]) - three fresh child processes on the one GPU, side by side."""
    import json
    tmp = tmp_path_factory.mktemp("dp_resume")
    script = tmp / "dp_resume_worker.py"
    script.write_text(WORKER)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29577")
    jobs = [dict(env, WORLD_SIZE="1", RANK="0")] + [dict(env, WORLD_SIZE="2", RANK=str(r)) for r in range(2)]
    procs = [subprocess.Popen([sys.executable, str(script), ROOT, str(tmp)], env=e, stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT, text=True) for e in jobs]
    try:
        outs = [p.communicate(timeout=300)[0] for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o[-3000:]
        assert "ok" in o
    load = lambda name: json.load(open(tmp / name))  # noqa: E731
    return tmp, load("w1_r0.json"), [load("w2_r0.json"), load("w2_r1.json")]


GLOBAL_STATE = ("policy", "predictor", "hash_tables", "ems_norm", "intrinsic_returns_rms")


def test_resumed_two_rank_run_ends_where_the_uninterrupted_one_does(runs):
    _tmp, _one, two = runs
    for rank, rec in enumerate(two):
        assert rec["uninterrupted"]["ems_len"] == 16 and rec["uninterrupted"]["rnd_adam_steps"] == 2
        for key in GLOBAL_STATE:
            assert rec["fresh"][key] != rec["after_one"][key], f"rank {rank}: the second pair of ranks did not start apart ({key})"
            assert rec["restored"][key] == rec["after_one"][key], f"rank {rank}: {key} was not restored"
            assert rec["resumed"][key] == rec["uninterrupted"][key], f"rank {rank}: {key} after the resumed iteration"
            assert rec["uninterrupted"][key] != rec["after_one"][key], f"rank {rank}: {key} did not move in the second iteration"
        # per-rank state came back too: the rank's own env columns produced the same intrinsic rewards
        assert rec["resumed"]["int_rewards"] == rec["uninterrupted"]["int_rewards"]
        assert rec["resumed"]["step"] == rec["uninterrupted"]["step"] == 2 * 4 * 8 * 2
        assert rec["resumed"]["rnd_adam_steps"] == 2
    for key in GLOBAL_STATE:  # global state: the same on both ranks
        assert two[0]["resumed"][key] == two[1]["resumed"][key], key
    assert two[0]["resumed"]["int_rewards"] != two[1]["resumed"]["int_rewards"], "both ranks stepped the same envs"


def test_one_rank_checkpoint_keeps_the_parents_key_tree(runs):
    from ppo_amd import checkpoint
    tmp, one, _two = runs
    assert one["after_one"]["ems_len"] == 16 and one["after_one"]["step"] == 4 * 16
    cp = checkpoint.load(str(tmp / "checkpoint-w1.pt"))
    got = key_paths(cp)
    assert len(PARENT_KEYS) > 20 and sorted(got) == sorted(PARENT_KEYS), (sorted(set(got) ^ set(PARENT_KEYS)))
